"""Build time and quality of the device HnswGraph builder (isl_hnsw_build) in its batched mode.
    python tools/hnsw_build_perf.py [--nodes N] [--dim D] [--batch B] [--dataset G|M] [--select reference|diverse]
                                    [--ef 100,128] [--nq Q] [--flat] [--build-only] [--insert K]
Prints one JSON line: build seconds (host clock around the call, which ends in a device synchronise),
inserts per second, and per ef queries per second (1024-query batches, k 10) and recall@10 against the
library's brute force.  --flat measures the flat LeannIndex builder (m0 32, ef_construction 200, same rule and
step) on the same rows instead.  Dataset G = synth.make_rows, M = synth.make_manifold.  --build-only stops
after the build (the run to put under rocprofv3 --kernel-trace --stats).
--insert K measures isl_hnsw_insert instead and prints one JSON line of seconds: (a) the one-call build of N
rows, (b) build(N - K) and insert(K) separately -- (a) and (b) twice, alternating -- (c) insert of a single
further row, five times: the call's fixed cost (row copy, table import, compaction, swap) -- and the median of
(c) as a share of the median of (b)'s insert."""
import argparse, json, os, sys, time
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
ap.add_argument("--select", choices=["reference", "diverse"], default="diverse")
ap.add_argument("--ef", default="100,128")
ap.add_argument("--nq", type=int, default=1024)
ap.add_argument("--flat", action="store_true")
ap.add_argument("--build-only", action="store_true")
ap.add_argument("--insert", type=int, default=0)
args = ap.parse_args()
N, d, nq = args.nodes, args.dim, args.nq
dev = torch.device("cuda:0")
if args.dataset == "G":
    x = synth.make_rows(N, d, 0, N, device=dev)
    q = synth.make_rows(N, d, 0, nq, device=dev, query=True)
else:
    x = synth.make_manifold(N, d, 42, device=dev)
    q = synth.make_manifold(nq, d, 4300, device=dev)
if args.insert:
    K = args.insert
    extra = synth.make_rows(N + 5, d, 0, N + 5, device=dev)[N:] if args.dataset == "G" else synth.make_manifold(
        5, d, 4301, device=dev)
    kw = dict(batch=args.batch, select=args.select, level_seed=1)

    def timed(f):
        torch.cuda.synchronize()
        t = time.time()
        r = f()
        return r, time.time() - t

    ia.HnswGraph.build(x[:4096], **kw).insert(x[4096:8192], **kw)  # warm: code objects, allocator
    one_call, head, tail = [], [], []
    for _ in range(2):  # the two ways alternate, so that a drift of the machine shows in both
        g, dt = timed(lambda: ia.HnswGraph.build(x, **kw))
        one_call.append(round(dt, 3))
        del g
        g, dt = timed(lambda: ia.HnswGraph.build(x[:N - K], **kw))
        head.append(round(dt, 3))
        tail.append(round(timed(lambda: g.insert(x[N - K:], **kw))[1], 3))
    single = [round(timed(lambda i=i: g.insert(extra[i:i + 1], **kw))[1], 4) for i in range(5)]
    assert len(g) == N + 5
    print(json.dumps({"what": "hnsw_insert_perf", "dataset": args.dataset, "nodes": N, "dim": d, "batch": args.batch,
                      "select": args.select, "m": 16, "m0": 32, "ef_construction": 200, "inserted": K,
                      "one_call_build_s": one_call, "build_head_s": head, "insert_tail_s": tail,
                      "insert_one_row_s": single,
                      "one_row_share_of_insert": round(float(np.median(single)) / float(np.median(tail)), 3)}))
    sys.exit(0)
ti = None
if not args.build_only:
    ti, _ = synth.brute_force_topk_native(x, q, 10)
    ti = ti.cpu().numpy()
qh = q.cpu().numpy()
out = {"what": "hnsw_build_perf", "graph": "flat LeannIndex" if args.flat else "HnswGraph", "dataset": args.dataset,
       "nodes": N, "dim": d, "batch": args.batch, "select": args.select, "m": 16, "m0": 32, "ef_construction": 200}
if args.flat:
    xh = x.cpu().numpy()
    del x
    torch.cuda.empty_cache()
    cfg = ia.LeannConfig.paper_default()
    cfg.m0, cfg.ef_construction = 32, 200
    t = time.time()
    g = ia.LeannIndex.build(xh, cfg, batch=args.batch, select=args.select)
    dt = time.time() - t
else:
    torch.cuda.synchronize()
    t = time.time()
    g = ia.HnswGraph.build(x, batch=args.batch, select=args.select, level_seed=1)  # HnswConfig::default(), rows in place
    dt = time.time() - t
    out["max_level"] = g.max_level
out["build_s"] = round(dt, 2)
out["inserts_per_s"] = round(N / dt)
out["search"] = []
if not args.build_only:
    for ef in (int(e) for e in args.ef.split(",")):
        g.search_batch(qh, 10, ef)  # warm: workspaces, code objects
        t = time.time()
        r = g.search_batch(qh, 10, ef)
        ds = time.time() - t
        if args.flat:
            ids, _, cnt = r
            got = [ids[i, :cnt[i]].tolist() for i in range(nq)]
        else:
            got = [ids.tolist() for ids, _ in r]
        hit = sum(len(set(got[i]) & set(ti[i].tolist())) for i in range(nq))
        st = g.last_stats()
        out["search"].append({"ef": ef, "queries": nq, "queries_per_s": round(nq / ds),
                              "recall_at_10": round(hit / (10.0 * nq), 4),
                              "evals_per_query": round(st["evals"] / nq, 1)})
print(json.dumps(out))
