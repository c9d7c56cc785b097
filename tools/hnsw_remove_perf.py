"""Time and quality of isl_hnsw_remove (HnswGraph.remove) against rebuilding the survivors.
    python tools/hnsw_remove_perf.py [--nodes N] [--dim D] [--batch B] [--remove 1,4096,65536] [--nq Q] [--ef 64]
                                     [--out profiles/hnsw_remove.json]
One graph of N rows of dataset M (synth.make_manifold), HnswConfig::default(), built with the diverse rule in the
batched mode.  The removals run one after the other on that graph, each taking random ids out of what the one
before left (the handle shrinks in place and cannot be copied); a count above 4096 is scaled by N / 1 000 000, so
that the largest stays the share of the graph the flat removal was measured with.  For each removal: seconds of
the call (host clock, the call ends in a device synchronise); seconds of HnswGraph.build of the survivors in the
same process, same rule and batch -- the yardstick for time and for quality; recall@10 at --ef of both graphs
against isl_bruteforce_topk over the survivors; the survivors not reachable from the entry point on layer 0
(HnswGraph.reachability), for both; and the call's ISL_DEBUG line (removed, touched lists per layer, candidates, repair-kernel ms), which the
library writes to stderr and this tool captures.  Prints one JSON document and writes it to --out."""
import argparse, json, os, sys, tempfile, time
sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import numpy as np, torch
import islands_amd as ia
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--remove", default="1,4096,65536")
ap.add_argument("--nq", type=int, default=1024)
ap.add_argument("--ef", type=int, default=64)
ap.add_argument("--out", default=os.path.join("profiles", "hnsw_remove.json"))
args = ap.parse_args()
N, d, nq, ef = args.nodes, args.dim, args.nq, args.ef
dev = torch.device("cuda:0")
kw = dict(batch=args.batch, select="diverse", level_seed=1)


def timed(f):
    torch.cuda.synchronize()
    t = time.time()
    r = f()
    torch.cuda.synchronize()
    return r, time.time() - t


def with_debug_line(f):
    """f() with ISL_DEBUG set and file descriptor 2 redirected: (result, seconds, the library's removal line)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["ISL_DEBUG"] = "1"
        try:
            r, dt = timed(f)
        finally:
            del os.environ["ISL_DEBUG"]
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        lines = [ln for ln in tmp.read().decode(errors="replace").splitlines() if "isl_hnsw_remove" in ln]
    return r, dt, (lines[-1] if lines else None)


def recall(g, rows, q):
    truth = synth.brute_force_topk_native(rows, q, 10)[0].cpu().numpy()
    qh = q.cpu().numpy()
    g.search_batch(qh, 10, ef)  # warm: workspaces, padded adjacency
    got = g.search_batch(qh, 10, ef)
    hit = sum(len(set(ids.tolist()) & set(truth[i].tolist())) for i, (ids, _) in enumerate(got))
    return round(hit / (10.0 * len(got)), 4)


HOST_WALK_UP_TO = 200_000  # nodes up to which the host walk (one ctypes call per node) runs beside the device's


def unreachable(g):
    """survivors a walk over layer 0 from the entry point does not meet: HnswGraph.reachability on the device,
    cross-checked against the host walk of tools/host_walk.py where that takes seconds"""
    if not len(g):
        return 0
    r = g.reachability(layer=0)
    missed = r["nodes"] - r["reached"]
    if len(g) <= HOST_WALK_UP_TO:
        import host_walk
        assert host_walk.hnsw_unreachable(g) == missed
    return missed


x = synth.make_manifold(N, d, 42, device=dev)
q = synth.make_manifold(nq, d, 4300, device=dev)
warm = ia.HnswGraph.build(x[:8192], **kw)  # code objects, allocator
warm.remove(np.arange(0, 8192, 16), select="diverse")
del warm
g, build_s = timed(lambda: ia.HnswGraph.build(x, **kw))
out = {"what": "hnsw_remove_perf", "dataset": "M", "nodes": N, "dim": d, "batch": args.batch, "select": "diverse",
       "m": 16, "m0": 32, "ef_construction": 200, "ef": ef, "queries": nq, "build_s": round(build_s, 3),
       "max_level": g.max_level, "removals": []}
print(f"built {N} rows in {build_s:.2f} s", file=sys.stderr, flush=True)
alive = np.arange(N)  # row of x behind every id of the handle
rng = np.random.default_rng(7)
for want in (int(c) for c in args.remove.split(",")):
    k = want if want <= 4096 else max(1, round(want * N / 1_000_000))
    n0 = len(g)
    ids = rng.choice(n0, k, replace=False).astype(np.uint64)
    remap, dt, line = with_debug_line(lambda: g.remove(ids, select="diverse"))
    alive = alive[remap != ia.REMOVED]
    rows = x[torch.from_numpy(alive).to(dev)].contiguous()
    rebuilt, rebuild_s = timed(lambda: ia.HnswGraph.build(rows, **kw))
    out["removals"].append({
        "len_before": n0, "removed": k, "asked": want, "remove_s": round(dt, 4), "rebuild_survivors_s": round(rebuild_s, 3),
        "rebuild_over_remove": round(rebuild_s / dt, 1), "max_level_after": g.max_level,
        "recall_at_10": {"shrunk": recall(g, rows, q), "rebuilt": recall(rebuilt, rows, q)},
        "unreachable_on_layer_0": {"shrunk": unreachable(g), "rebuilt": unreachable(rebuilt)},
        "debug_line": line})
    print(json.dumps(out["removals"][-1]), file=sys.stderr, flush=True)
    del rebuilt, rows
    torch.cuda.empty_cache()
text = json.dumps(out, indent=1)
print(text)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text + "\n")
