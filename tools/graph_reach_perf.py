"""Graph reachability on the device (LeannIndex.reachability / HnswGraph.reachability) and the covering entry seeds
(LeannIndex.cover_entry_seeds): what they cost beside the host walks they replace, and what they say about the graphs.
    python tools/graph_reach_perf.py [--nodes N] [--dim D] [--runs 5] [--ef 128] [--nq 1024]
                                     [--host-walk-up-to N] [--out profiles/graph_reach.json]
Three graphs of N rows: dataset M (synth.make_manifold) under LeannIndex.build, dataset G (synth.make_rows) under
LeannIndex.build, both with the diverse rule at 4096 nodes per step, and an HnswGraph over dataset M.  For each:
  reachability  after one warm call, the median of --runs calls of
                  walk    report NULL, depth into a device buffer: the level loop alone
                  report  report only: the level loop, the in-degree pass and the reduction
                  arrays  report, depth and in_degree into host arrays: plus two [len] read-backs
                so in_degree + reduction = report - walk and the read-backs = arrays - report; `levels`; the host
                walk it replaces in the same process (tools/host_walk.py: one ctypes call per node, then numpy), and
                the bound (4 edges + 16 len bytes) / 8 TB/s + levels x the measured cost of one level's launch and
                one-word read-back (a ring: (seconds of a ring of 4097 - seconds of one node) / 4096 levels)
  cover         (LeannIndex only) wall seconds on the index without a table, seeds added, and the scans and one-word
                read-backs of the call's ISL_DEBUG line
Dataset G, the open entry-seed question: for entry at node 0, 64 k-centre seeds and the cover, reached / len and
recall@10 at --ef against the f32 brute force; and of the true neighbours the unseeded search misses, how many are
not reachable from node 0 at all.  Prints one JSON document and writes it to --out."""
import argparse, ctypes as C, json, os, statistics, sys, tempfile, time
sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import numpy as np, torch
import islands_amd as ia
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_walk, synth

HBM_PEAK = 8.0e12
ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--ef", type=int, default=128)
ap.add_argument("--nq", type=int, default=1024)
ap.add_argument("--host-walk-up-to", type=int, default=1_000_000)
ap.add_argument("--out", default=os.path.join("profiles", "graph_reach.json"))
args = ap.parse_args()
N, d, nq = args.nodes, args.dim, args.nq
dev = torch.device("cuda:0")
lib = ia._ffi.lib()


def wall(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = f()
    return r, time.perf_counter() - t


def median_s(f):
    f()
    return statistics.median(wall(f)[1] for _ in range(max(args.runs, 5)))


def ring_index(n):
    g = ia.CsrGraph(node_offsets=np.arange(n + 1, dtype=np.uint64), neighbors=(np.arange(n, dtype=np.uint64) + 1) % n,
                    levels=np.zeros(n, np.uint64), entry_point=0, num_nodes=n, degree_counts=np.ones(n, np.uint64))
    return ia.LeannIndex.from_csr(g, ia.LeannConfig(), dimension=4).upload(0)


def level_cost():
    """seconds of one level with a frontier of one node: its launch and its one-word read-back"""
    one, ring = ring_index(1), ring_index(4097)
    t1, tr = median_s(lambda: one.reachability()), median_s(lambda: ring.reachability())
    assert ring.reachability()["levels"] == 4097
    return (tr - t1) / 4096, t1


def reach_timings(graph, n, call):
    """call(depth_ptr, in_degree_ptr, mem, report_ptr) -> status"""
    d_depth = torch.zeros(n, dtype=torch.int32, device=dev)
    h_depth, h_in = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    rep = ia._ffi.ReachReportC()

    def ok(st):
        assert st == 0, lib.isl_last_error_message().decode()

    walk = median_s(lambda: ok(call(C.c_void_p(d_depth.data_ptr()), None, ia.MEM_DEVICE, None)))
    report = median_s(lambda: ok(call(None, None, ia.MEM_HOST, C.byref(rep))))
    arrays = median_s(lambda: ok(call(h_depth.ctypes.data_as(C.c_void_p), h_in.ctypes.data_as(C.c_void_p), ia.MEM_HOST,
                                      C.byref(rep))))
    r = {f: int(getattr(rep, f)) for f, _ in ia._ffi.ReachReportC._fields_}
    bound = (4 * r["edges"] + 16 * n) / HBM_PEAK + r["levels"] * LEVEL_S
    return {"report": r, "reached_of_len": round(r["reached"] / n, 6),
            "seconds": {"walk": round(walk, 6), "report": round(report, 6), "arrays_to_host": round(arrays, 6),
                        "in_degree_and_reduction": round(report - walk, 6), "array_readbacks": round(arrays - report, 6)},
            "bound_s": round(bound, 6), "walk_over_bound": round(walk / bound, 2)}, h_depth


def debug_line(f, name):
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["ISL_DEBUG"] = "1"
        try:
            r, dt = wall(f)
        finally:
            del os.environ["ISL_DEBUG"]
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        lines = [ln for ln in tmp.read().decode(errors="replace").splitlines() if name in ln]
    return r, dt, (lines[-1] if lines else None)


def recall(idx, q, truth):
    qh = q.cpu().numpy()
    idx.search_batch(qh, 10, args.ef)
    ids, _, cnt = idx.search_batch(qh, 10, args.ef)
    found = [set(ids[i, :cnt[i]].tolist()) for i in range(len(qh))]
    hit = sum(len(found[i] & set(truth[i].tolist())) for i in range(len(qh)))
    return round(hit / (10.0 * len(qh)), 4), found


def flat_graph(name, x, q):
    truth = synth.brute_force_topk_native(x, q, 10)[0].cpu().numpy()
    xh = x.cpu().numpy()
    idx, build_s = wall(lambda: ia.LeannIndex.build(xh, ia.LeannConfig.paper_default(), batch=4096, select="diverse"))
    del xh
    call = lambda pd, pi, mem, rep: lib.isl_index_reachability(idx._h, None, 0, pd, pi, mem, rep)
    out, depth0 = reach_timings(idx, N, call)
    out.update({"graph": name, "kind": "LeannIndex.build diverse, batch 4096", "build_s": round(build_s, 2)})
    if N <= args.host_walk_up_to:
        missed, host_s = wall(lambda: host_walk.index_unreachable(idx))
        assert missed == N - out["report"]["reached"], (missed, out["report"])
        out["host_walk_s"] = round(host_s, 3)
        out["host_walk_over_device_walk"] = round(host_s / out["seconds"]["walk"], 1)
    else:
        out["host_walk_s"] = "not measured"
    legs = []
    r0, found0 = recall(idx, q, truth)
    legs.append({"leg": "entry at node %d" % idx.entry_point, "seeds": 0, "reached_of_len": out["reached_of_len"],
                 "recall_at_10": r0})
    lost = [int(t) for i in range(len(truth)) for t in truth[i] if int(t) not in found0[i]]
    out["true_neighbours_missed_unseeded"] = {"missed": len(lost),
                                              "not_reachable_from_the_entry": int(sum(depth0[t] == 0xFFFFFFFF for t in lost))}
    seeds, sel_s = wall(lambda: idx.select_entry_seeds(64))
    rr_ = idx.reachability()
    legs.append({"leg": "64 k-centre seeds", "seeds": len(seeds), "selection_s": round(sel_s, 3),
                 "reached_of_len": round(rr_["reached"] / N, 6), "recall_at_10": recall(idx, q, truth)[0]})
    idx.set_entry_seeds([])
    idx.cover_entry_seeds(1)  # code objects
    got, cover_s, line = debug_line(lambda: idx.cover_entry_seeds(), "isl_index_cover_entry_seeds")
    rr_ = idx.reachability()
    legs.append({"leg": "cover", "seeds": int(got["ids"].size), "unreached": got["unreached"], "cover_s": round(cover_s, 4),
                 "debug_line": line, "reached_of_len": round(rr_["reached"] / N, 6),
                 "recall_at_10": recall(idx, q, truth)[0] if got["ids"].size else r0})
    out["entry_legs"] = legs
    print(json.dumps(out), file=sys.stderr, flush=True)
    return out


LEVEL_S, CALL_S = level_cost()
doc = {"what": "graph_reach_perf", "nodes": N, "dim": d, "ef": args.ef, "queries": nq, "runs": max(args.runs, 5),
       "one_level_launch_and_readback_s": round(LEVEL_S, 7), "call_on_one_node_s": round(CALL_S, 6), "graphs": []}
print(json.dumps({k: v for k, v in doc.items() if k != "graphs"}), file=sys.stderr, flush=True)

x = synth.make_manifold(N, d, 42, device=dev)
q = synth.make_manifold(nq, d, 4300, device=dev)
doc["graphs"].append(flat_graph("M", x, q))
torch.cuda.empty_cache()

g, build_s = wall(lambda: ia.HnswGraph.build(x, batch=4096, select="diverse", level_seed=1))
layers = []
for layer in range(g.max_level + 1):
    call = lambda pd, pi, mem, rep, L=layer: lib.isl_hnsw_reachability(g._h, L, None, 0, pd, pi, mem, rep)
    t, _ = reach_timings(g, N, call)
    t["layer"] = layer
    layers.append(t)
h = {"graph": "M", "kind": "HnswGraph.build diverse, batch 4096", "build_s": round(build_s, 2), "max_level": g.max_level,
     "layers": layers}
if N <= args.host_walk_up_to:
    missed, host_s = wall(lambda: host_walk.hnsw_unreachable(g))
    assert missed == N - layers[0]["report"]["reached"], (missed, layers[0]["report"])
    h["host_walk_layer_0_s"] = round(host_s, 3)
    h["host_walk_over_device_walk"] = round(host_s / layers[0]["seconds"]["walk"], 1)
else:
    h["host_walk_layer_0_s"] = "not measured"
doc["graphs"].append(h)
print(json.dumps(h), file=sys.stderr, flush=True)
del g, x, q
torch.cuda.empty_cache()

x = synth.make_rows(N, d, 0, N, device=dev)
q = synth.make_rows(N, d, 0, nq, device=dev, query=True)
doc["graphs"].append(flat_graph("G", x, q))

text = json.dumps(doc, indent=1)
print(text)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text + "\n")
