"""Build time and quality of the device graph builder (isl_index_build_rows) in its batched mode.
    python tools/build_perf.py [--nodes N] [--dim D] [--batch B] [--dataset G|M] [--select reference|diverse]
                               [--alpha A] [--no-keep-pruned] [--ef 128,256] [--nq Q] [--check-truth]
                               [--row-dtype f32|bf16[,...]]
Prints one JSON line per leg: build seconds, peak device memory during the build, recall@10 / evaluations /
hops per query at every ef, mean and minimum degree.  Dataset G = synth.make_rows (clustered, the headline
rows), M = synth.make_manifold.  --row-dtype names the legs, built one after the other in this process
(f32,bf16,f32,bf16 alternates them).  With a bf16 leg the generated rows are rounded to bf16 once and every
leg builds from those values -- the f32 legs from their widened images -- so all legs build the same graph
problem, and the truth is the brute force over the widened rows."""
import argparse, json, os, sys, threading, time
sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import numpy as np, torch
import islands_amd as ia
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--dataset", choices=["G", "M"], default="G")
ap.add_argument("--select", choices=["reference", "diverse"], default="reference")
ap.add_argument("--alpha", type=float, default=1.0)
ap.add_argument("--no-keep-pruned", action="store_true")
ap.add_argument("--ef", default="128,256", help="comma-separated ef values of the recall measurement")
ap.add_argument("--nq", type=int, default=512)
ap.add_argument("--qstart", type=int, default=0, help="dataset G: first row of the query stream (bench.py's batch b starts at 1024 b)")
ap.add_argument("--row-dtype", default="f32", help="comma-separated legs, each f32 or bf16")
ap.add_argument("--check-truth", action="store_true", help="also report how far torch's brute force agrees with the truth")
args = ap.parse_args()
N, d, nq = args.nodes, args.dim, args.nq
legs = args.row_dtype.split(",")
if any(leg not in ("f32", "bf16") for leg in legs):
    ap.error("--row-dtype takes f32 and bf16")
dev = torch.device("cuda:0")
if args.dataset == "G":
    x = synth.make_rows(N, d, 0, N, device=dev)
    q = synth.make_rows(N, d, args.qstart, nq, device=dev, query=True)
else:
    x = synth.make_manifold(N, d, 42, device=dev)
    q = synth.make_manifold(nq, d, 4300, device=dev)  # bench.py's first query batch
rounded = "bf16" in legs
if rounded:  # round to nearest even once; x becomes the widened values
    x = x.to(torch.bfloat16).to(torch.float32)
ti, _ = synth.brute_force_topk_native(x, q, 10)  # exact truth by the library's f32 brute force, as bench.py takes it
truth_check = None
if args.check_truth:  # share of the truth that torch's matmul brute force agrees with
    tt, _ = synth.brute_force_topk(x, q, 10)
    truth_check = float((ti[:, :, None] == tt[:, None, :]).any(2).float().mean().item())
    del tt
ti = ti.cpu().numpy()
xh, qh = x.cpu().numpy(), q.cpu().numpy()
xbits = (xh.view(np.uint32) >> 16).astype(np.uint16) if rounded else None  # exact: the low halves are zero
del x
torch.cuda.empty_cache()
cfg = ia.LeannConfig.paper_default()


def used_bytes():
    free, total = torch.cuda.mem_get_info(0)  # hipMemGetInfo: the whole device, whoever allocated
    return total - free


for leg in legs:
    before, peak, stop = used_bytes(), [0], threading.Event()

    def poll():
        while not stop.is_set():
            peak[0] = max(peak[0], used_bytes())
            time.sleep(0.02)

    th = threading.Thread(target=poll, daemon=True)
    th.start()
    t = time.time()
    if leg == "bf16":
        idx = ia.LeannIndex.build_bf16(xbits, cfg, batch=args.batch, select=args.select, alpha=args.alpha,
                                       keep_pruned=not args.no_keep_pruned)
    else:
        idx = ia.LeannIndex.build(xh, cfg, batch=args.batch, select=args.select, alpha=args.alpha,
                                  keep_pruned=not args.no_keep_pruned)
    dt = time.time() - t
    stop.set()
    th.join()
    out = {"what": "build_perf", "dataset": args.dataset, "nodes": N, "dim": d, "batch": args.batch,
           "row_dtype": leg, "rows_rounded_to_bf16": rounded,
           "select": args.select, "alpha": args.alpha, "keep_pruned": not args.no_keep_pruned,
           "m0": cfg.m0, "ef_construction": cfg.ef_construction, "build_s": round(dt, 2),
           "nodes_per_s": round(N / dt), "device_bytes_before": before,
           "device_bytes_peak_in_build": max(peak[0], before), "device_bytes_after": used_bytes(),
           "queries": nq, "qstart": args.qstart, "search": []}
    for ef in (int(e) for e in args.ef.split(",")):
        ids, dist, cnt = idx.search_batch(qh, 10, ef)
        hit = sum(len(set(ids[i, :cnt[i]].tolist()) & set(ti[i].tolist())) for i in range(nq))
        st = idx.last_stats()
        out["search"].append({"ef": ef, "recall_at_10": round(hit / (10.0 * nq), 4),
                              "evals_per_query": round(st["evals"] / nq, 1),
                              "hops_per_query": round(st["expansions"] / nq, 1)})
    # degrees of a sample of nodes (node 0 starts empty and only gains back links)
    sample = np.random.default_rng(0).integers(1, N, size=min(N - 1, 20000))
    degs = np.array([len(idx.get_neighbors(int(i))) for i in sample])
    if truth_check is not None:
        out["torch_truth_agreement"] = round(truth_check, 4)
    out["degree_sample"] = int(sample.size)
    out["mean_degree"] = round(float(degs.mean()), 2)
    out["min_degree"] = int(degs.min())
    print(json.dumps(out), flush=True)
    del idx
