"""Build time and quality of the device HnswGraph builder (isl_hnsw_build) in its batched mode.
    python tools/hnsw_build_perf.py [--nodes N] [--dim D] [--batch B] [--dataset G|M] [--select reference|diverse]
                                    [--ef 100,128] [--nq Q] [--flat] [--build-only] [--insert K]
                                    [--rows f32|bf16|ab]
Prints one JSON line: build seconds (host clock around the call, which ends in a device synchronise),
inserts per second, and per ef queries per second (1024-query batches, k 10, five calls) and recall@10 against the
library's brute force.  --flat measures the flat LeannIndex builder (m0 32, ef_construction 200, same rule and
step) on the same rows instead.  Dataset G = synth.make_rows, M = synth.make_manifold.  --build-only stops
after the build (the run to put under rocprofv3 --kernel-trace --stats).
--insert K measures isl_hnsw_insert instead and prints one JSON line of seconds: (a) the one-call build of N
rows, (b) build(N - K) and insert(K) separately -- (a) and (b) twice, alternating -- (c) insert of a single
further row, five times: the call's fixed cost (row copy, table import, compaction, swap) -- and the median of
(c) as a share of the median of (b)'s insert.
--rows bf16 rounds the generated rows to bf16 on the device (the queries stay f32) and builds with build_bf16 /
inserts with insert_bf16; the JSON line carries row_bytes, the device bytes of the graph's row table
(row_storage()).  --rows ab is the comparison of the two row types in one process: the rows are rounded to bf16,
the f32 build of their widened values and the bf16 build of their bits alternate, twice each, and both graphs are
searched; one JSON line with a leg per type (build seconds of both repetitions, row_bytes, the search figures)."""
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
ap.add_argument("--rows", choices=["f32", "bf16", "ab"], default="f32")
args = ap.parse_args()
N, d, nq = args.nodes, args.dim, args.nq
dev = torch.device("cuda:0")
if args.dataset == "G":
    x = synth.make_rows(N, d, 0, N, device=dev)
    q = synth.make_rows(N, d, 0, nq, device=dev, query=True)
else:
    x = synth.make_manifold(N, d, 42, device=dev)
    q = synth.make_manifold(nq, d, 4300, device=dev)
bf16 = args.rows == "bf16"
if args.rows != "f32":  # the rows become bf16 values; x16 holds their bit patterns, x their exact f32 images
    x16 = x.to(torch.bfloat16)
    x = x16.to(torch.float32) if args.rows == "ab" else None
build = ia.HnswGraph.build_bf16 if bf16 else ia.HnswGraph.build
if bf16:
    x = x16
if args.insert:
    if args.rows == "ab":
        sys.exit("--insert takes --rows f32 or bf16")
    K = args.insert
    extra = synth.make_rows(N + 5, d, 0, N + 5, device=dev)[N:] if args.dataset == "G" else synth.make_manifold(
        5, d, 4301, device=dev)
    if bf16:
        extra = extra.to(torch.bfloat16)
    insert = (lambda g, rows, **kw: g.insert_bf16(rows, **kw)) if bf16 else (lambda g, rows, **kw: g.insert(rows, **kw))
    kw = dict(batch=args.batch, select=args.select, level_seed=1)

    def timed(f):
        torch.cuda.synchronize()
        t = time.time()
        r = f()
        return r, time.time() - t

    insert(build(x[:4096], **kw), x[4096:8192], **kw)  # warm: code objects, allocator
    one_call, head, tail = [], [], []
    for _ in range(2):  # the two ways alternate, so that a drift of the machine shows in both
        g, dt = timed(lambda: build(x, **kw))
        one_call.append(round(dt, 3))
        del g
        g, dt = timed(lambda: build(x[:N - K], **kw))
        head.append(round(dt, 3))
        tail.append(round(timed(lambda: insert(g, x[N - K:], **kw))[1], 3))
    single = [round(timed(lambda i=i: insert(g, extra[i:i + 1], **kw))[1], 4) for i in range(5)]
    assert len(g) == N + 5
    print(json.dumps({"what": "hnsw_insert_perf", "dataset": args.dataset, "nodes": N, "dim": d, "batch": args.batch,
                      "select": args.select, "m": 16, "m0": 32, "ef_construction": 200, "inserted": K,
                      "rows": args.rows, "row_bytes": g.row_storage()["block_bytes"],
                      "one_call_build_s": one_call, "build_head_s": head, "insert_tail_s": tail,
                      "insert_one_row_s": single,
                      "one_row_share_of_insert": round(float(np.median(single)) / float(np.median(tail)), 3)}))
    sys.exit(0)
ti = None
if not args.build_only:  # (the truth is over the rows the graph holds: the widened values where they were rounded)
    ti, _ = synth.brute_force_topk_native(x16.to(torch.float32) if bf16 else x, q, 10)
    ti = ti.cpu().numpy()
qh = q.cpu().numpy()


def searched(g, flat=False):
    """per ef: queries/s over five calls of the whole query batch after a warm one, recall@10, evaluations per query"""
    res = []
    for ef in (int(e) for e in args.ef.split(",")):
        g.search_batch(qh, 10, ef)  # warm: workspaces, code objects
        t = time.time()
        for _ in range(5):
            r = g.search_batch(qh, 10, ef)
        ds = (time.time() - t) / 5
        if flat:
            ids, _, cnt = r
            got = [ids[i, :cnt[i]].tolist() for i in range(nq)]
        else:
            got = [ids.tolist() for ids, _ in r]
        hit = sum(len(set(got[i]) & set(ti[i].tolist())) for i in range(nq))
        st = g.last_stats()
        res.append({"ef": ef, "queries": nq, "queries_per_s": round(nq / ds),
                    "recall_at_10": round(hit / (10.0 * nq), 4),
                    "evals_per_query": round(st["evals"] / nq, 1)})
    return res


out = {"what": "hnsw_build_perf", "graph": "flat LeannIndex" if args.flat else "HnswGraph", "dataset": args.dataset,
       "nodes": N, "dim": d, "batch": args.batch, "select": args.select, "m": 16, "m0": 32, "ef_construction": 200,
       "rows": args.rows}
if args.rows == "ab":
    if args.flat:
        sys.exit("--rows ab compares HnswGraph builds")
    kw = dict(batch=args.batch, select=args.select, level_seed=1)
    ia.HnswGraph.build(x[:4096], **kw)  # warm: code objects, allocator
    ia.HnswGraph.build_bf16(x16[:4096], **kw)
    legs = {"f32": {"build_s": []}, "bf16": {"build_s": []}}
    for rep_no in range(2):  # the two types alternate, so that a drift of the machine shows in both
        for name, fn, rows in (("f32", ia.HnswGraph.build, x), ("bf16", ia.HnswGraph.build_bf16, x16)):
            torch.cuda.synchronize()
            t = time.time()
            g = fn(rows, **kw)
            legs[name]["build_s"].append(round(time.time() - t, 2))
            if rep_no == 1:  # the second graph of each type is the one that is searched
                legs[name]["row_bytes"] = g.row_storage()["block_bytes"]
                legs[name]["max_level"] = g.max_level
                if not args.build_only:
                    legs[name]["search"] = searched(g)
            del g
    for leg in legs.values():
        leg["inserts_per_s"] = round(N / min(leg["build_s"]))
    out["legs"] = legs
    print(json.dumps(out))
    sys.exit(0)
if args.flat:
    if bf16:
        sys.exit("--flat takes --rows f32")
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
    g = build(x, batch=args.batch, select=args.select, level_seed=1)  # HnswConfig::default(), rows in place
    dt = time.time() - t
    out["max_level"] = g.max_level
    out["row_bytes"] = g.row_storage()["block_bytes"]
out["build_s"] = round(dt, 2)
out["inserts_per_s"] = round(N / dt)
out["search"] = [] if args.build_only else searched(g, args.flat)
print(json.dumps(out))
