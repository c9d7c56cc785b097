"""Entry seeds (isl_index_select_entry_seeds / the pick in front of a plain search): what they cost and buy.
    python tools/entry_seeds_perf.py select [--nodes N] [--dim D] [--seeds E] [--row-dtype f32,bf16]
    python tools/entry_seeds_perf.py search [--dataset G|M] [--nodes N] [--dim D] [--seeds 1024,4096]
                                            [--select reference|diverse] [--ef 128] [--windows 0:512,0:2048,...]
One JSON line per measurement.
  select: seconds of one selection of E seeds beside the bound of E - 1 passes over the row table at the HBM
          peak (8 TB/s); the rows' values do not matter for the rate (dataset M is generated).
  search: ONE graph built by the library (LeannIndex.build, 4096 nodes per step), searched without seeds and
          with each seed count on the same index object over windows of the query stream (dataset G: rows
          [a, b) of synth.make_rows' query stream, bench.py's batch i is 1024 i : 1024 (i + 1); dataset M:
          window a:b is batch a // 1024 onward of bench.py's manifold batches): recall@10 against the library's
          f32 brute force, evaluations and hops per query, and the rate of device-buffer calls of 1024 queries
          (wall clock over the window, one call at a time, and the calls' HIP-event kernel time, which
          includes the pick).  Every leg -- no seeds, each k-centre seed count, and `cover`
          (isl_index_cover_entry_seeds on the index without a table) -- also reports the seeds in use and
          reached / len of LeannIndex.reachability from the starts that leg's searches use."""
import argparse, json, os, sys, time
sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import numpy as np, torch
import islands_amd as ia
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth

HBM_PEAK = 8.0e12

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["select", "search"])
ap.add_argument("--dataset", choices=["G", "M"], default="G")
ap.add_argument("--nodes", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--seeds", default="1024")
ap.add_argument("--row-dtype", default="f32,bf16")
ap.add_argument("--select", choices=["reference", "diverse"], default="diverse")
ap.add_argument("--ef", type=int, default=128)
ap.add_argument("--windows", default="0:512,0:2048,0:8192,5120:9216,0:20480",
                help="query windows a:b (DESIGN.md 3.5: the first 512 / 2048 / 8192 queries, queries 5120-9215, "
                     "and the 20 batches of 1024 of the bench line)")
args = ap.parse_args()
N, d = args.nodes, args.dim
dev = torch.device("cuda:0")
seed_counts = [int(s) for s in args.seeds.split(",")]


def ring(n):
    off = np.arange(n + 1, dtype=np.uint64)
    nb = (np.arange(n, dtype=np.uint64) + 1) % n
    return ia.CsrGraph(node_offsets=off, neighbors=nb, levels=np.zeros(n, np.uint64), entry_point=0, num_nodes=n,
                       degree_counts=np.ones(n, np.uint64))


if args.what == "select":
    x = synth.make_manifold(N, d, 42, device=dev)
    for leg in args.row_dtype.split(","):
        idx = ia.LeannIndex.from_csr(ring(N), ia.LeannConfig.paper_default(), dimension=d).upload(0)
        if leg == "bf16":
            x16 = x.to(torch.bfloat16)
            idx.set_embeddings_bf16(None, device_ptr=x16.data_ptr(), n=N, d=d)
        else:
            idx.set_embeddings(None, device_ptr=x.data_ptr(), n=N, d=d)
        torch.cuda.synchronize()
        idx.select_entry_seeds(2)  # code object loaded
        for E in seed_counts:
            t = time.time()
            ids = idx.select_entry_seeds(E)
            dt = time.time() - t
            table = N * d * (2 if leg == "bf16" else 4)
            bound = (len(ids) - 1) * table / HBM_PEAK
            print(json.dumps({"what": "entry_seeds_select", "nodes": N, "dim": d, "row_dtype": leg, "seeds": len(ids),
                              "distinct": len(set(ids.tolist())), "seconds": round(dt, 4),
                              "hbm_bound_s": round(bound, 4), "of_bound": round(bound / dt, 3),
                              "row_bytes_per_s": round((len(ids) - 1) * table / dt)}), flush=True)
        del idx
    sys.exit(0)

nq_call = 1024
windows = [tuple(int(v) for v in w.split(":")) for w in args.windows.split(",")]
q_hi = max(b for _, b in windows)
if args.dataset == "G":
    x = synth.make_rows(N, d, 0, N, device=dev)
    q_all = synth.make_rows(N, d, 0, q_hi, device=dev, query=True)
else:
    x = synth.make_manifold(N, d, 42, device=dev)
    q_all = torch.cat([synth.make_manifold(nq_call, d, 4300 + b, device=dev) for b in range(-(-q_hi // nq_call))])[:q_hi]
truth = torch.cat([synth.brute_force_topk_native(x, q_all[a:a + nq_call], 10)[0] for a in range(0, q_hi, nq_call)])
truth = truth.cpu().numpy()
xh = x.cpu().numpy()
torch.cuda.empty_cache()
cfg = ia.LeannConfig.paper_default()
t = time.time()
idx = ia.LeannIndex.build(xh, cfg, batch=4096, select=args.select)
build_s = time.time() - t
del xh
ids_d = torch.zeros((nq_call, 10), dtype=torch.int64, device=dev)
dist_d = torch.zeros((nq_call, 10), dtype=torch.float32, device=dev)
cnt_d = torch.zeros(nq_call, dtype=torch.int32, device=dev)


def measure(tag, n_seeds, select_s):
    idx.prepare(nq_call, args.ef, 10, 2)
    reach = idx.reachability()
    for a, b in windows:
        hits = evals = hops = n = allocs = 0
        kernel_ms = 0.0
        torch.cuda.synchronize()
        t0 = time.time()
        outs = []
        for s in range(a, b, nq_call):
            m = min(nq_call, b - s)
            idx.search_batch_device(q_all[s:s + m].data_ptr(), m, d, 10, args.ef, ids_d.data_ptr(), dist_d.data_ptr(),
                                    cnt_d.data_ptr())
            st = idx.last_stats()
            evals += st["evals"]; hops += st["expansions"]; kernel_ms += st["kernel_ms"]; allocs += st["allocations"]
            outs.append((s, m, ids_d[:m].cpu().numpy(), cnt_d[:m].cpu().numpy()))
            n += m
        wall = time.time() - t0
        for s, m, ids, cnt in outs:
            for i in range(m):
                hits += len(set(ids[i, :cnt[i]].tolist()) & set(truth[s + i].tolist()))
        print(json.dumps({"what": "entry_seeds_search", "dataset": args.dataset, "nodes": N, "dim": d,
                          "select_rule": args.select, "build_s": round(build_s, 2), "leg": tag, "seeds": n_seeds,
                          "selection_s": select_s, "reached": reach["reached"],
                          "reached_of_len": round(reach["reached"] / N, 6), "ef": args.ef, "window": f"{a}:{b}", "queries": n,
                          "recall_at_10": round(hits / (10.0 * n), 4), "evals_per_query": round(evals / n, 1),
                          "hops_per_query": round(hops / n, 1),
                          "queries_per_s_wall_incl_copies": round(n / wall),
                          "queries_per_s_kernels": round(n / (kernel_ms / 1e3)), "kernel_ms_per_1024": round(kernel_ms / n * 1024, 4),
                          "allocations": allocs}), flush=True)


measure("unseeded", 0, None)
for E in seed_counts:
    t = time.time()
    got = idx.select_entry_seeds(E)
    measure("seeded", len(got), round(time.time() - t, 3))
idx.set_entry_seeds([])
t = time.time()
got = idx.cover_entry_seeds()
measure("cover", len(got["ids"]), round(time.time() - t, 3))
idx.set_entry_seeds([])
measure("unseeded_again", 0, None)
