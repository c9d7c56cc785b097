"""Refined search beside the plain search over narrow rows, on one graph, in one run: what re-scoring the candidates
against the f32 rows costs and buys, with those rows in HBM and in pinned host memory.
    python tools/refine_perf.py [--nodes 1000000] [--dim 768] [--steps 10] [--ef 128] [--repeats 3]
                                [--out profiles/refine_rows.json]
Dataset M of tools/synth.py.  ONE graph, built by the library from the f32 rows.  Legs: fp8 rows, plain search (k =
10); fp8 rows + f32 refine table on the device; fp8 rows + f32 refine table in pinned host memory; bf16 rows + f32
refine table in pinned host memory -- the refined legs with candidates 32 and 128.  Every leg runs `steps`
device-buffer calls of 1024 queries (fresh manifold batches, k = 10, ef = 128) after two warm-up calls on a prepared
index; the legs alternate and repeat, and the JSON keeps every repeat beside the median.  Per leg: queries/s (wall
clock over the timed calls, synchronised per call), the rescoring kernel's milliseconds per call of 1024 queries by
HIP events around isl_rescore_device alone (over the candidates of the last timed batch), recall@10 against the
library's f32 brute force over the f32 rows, and what the refine table costs where."""
import argparse, json, math, os, statistics, sys, time
sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import numpy as np, torch
import islands_amd as ia
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--ef", type=int, default=128)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--candidates", default="32,128")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                               "refine_rows.json"))
args = ap.parse_args()
N, d, k, nq, ef = args.nodes, args.dim, 10, 1024, args.ef
cands = [int(c) for c in args.candidates.split(",")]
dev = torch.device("cuda:0")

x = synth.make_manifold(N, d, 42, device=dev)
warm_q = [synth.make_manifold(nq, d, 4200 + b, device=dev) for b in range(2)]
queries = [synth.make_manifold(nq, d, 4300 + b, device=dev) for b in range(args.steps)]
truth = [synth.brute_force_topk_native(x, q, k)[0].cpu().numpy() for q in queries]
t0 = time.time()
idx = ia.LeannIndex.build(x.cpu().numpy(), ia.LeannConfig.paper_default(), batch=4096, select="diverse")
build_s = time.time() - t0

top = float(x.abs().max())
scale_exp = max(-32, min(32, math.ceil(math.log2(top / 448.0)))) if top > 0 else -32
while scale_exp < 32 and top * 2.0 ** -scale_exp > 448.0:
    scale_exp += 1
while scale_exp > -32 and top * 2.0 ** -(scale_exp - 1) <= 448.0:
    scale_exp -= 1
stored = {
    "bf16": x.to(torch.bfloat16),
    "fp8": (x * 2.0 ** -scale_exp).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8),
}
torch.cuda.synchronize()
cmax = max(cands)
ids_d = torch.zeros((nq, k), dtype=torch.int64, device=dev)
dist_d = torch.zeros((nq, k), dtype=torch.float32, device=dev)
cnt_d = torch.zeros(nq, dtype=torch.int32, device=dev)
cand_ids = torch.zeros((nq, cmax), dtype=torch.int64, device=dev)
cand_dist = torch.zeros((nq, cmax), dtype=torch.float32, device=dev)
cand_cnt = torch.zeros(nq, dtype=torch.int32, device=dev)
state = {"rows": None, "refine": None}


def attach(rows, refine):
    if state["rows"] != rows:
        p = stored[rows].data_ptr()
        if rows == "bf16":
            idx.set_embeddings_bf16(None, device_ptr=p, n=N, d=d)
        else:
            idx.set_embeddings_fp8(None, scale_exp, device_ptr=p, n=N, d=d)
        state["rows"] = rows
    if state["refine"] != refine:
        t = time.time()
        if refine is None:
            idx.set_refine_rows(None)
        else:
            idx.set_refine_rows(None, placement=refine, device_ptr=x.data_ptr(), n=N, d=d, dtype="f32")
        state["refine"], state["set_s"] = refine, round(time.time() - t, 3)
    idx.prepare(nq, ef, cmax, 2)


def call(q, c):
    if c is None:
        idx.search_batch_device(q.data_ptr(), nq, d, k, ef, ids_d.data_ptr(), dist_d.data_ptr(), cnt_d.data_ptr())
    else:
        idx.search_refined_batch_ptr(q.data_ptr(), nq, d, k, ef, c, ids_d.data_ptr(), dist_d.data_ptr(), cnt_d.data_ptr())
    return idx.last_stats()


def rescore_ms(q, c, rounds=5):
    """HIP-event time of the rescoring kernel alone over the plain search's c candidates of batch q"""
    idx.search_batch_device(q.data_ptr(), nq, d, c, ef, cand_ids.data_ptr(), cand_dist.data_ptr(), cand_cnt.data_ptr())
    ms = []
    for _ in range(rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        idx.rescore_ptr(q.data_ptr(), nq, d, cand_ids.data_ptr(), cand_cnt.data_ptr(), c, k, ids_d.data_ptr(),
                        dist_d.data_ptr(), cnt_d.data_ptr())
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(statistics.median(ms[1:]), 4)  # (the first launch loads the code object)


def run(rows, refine, c):
    attach(rows, refine)
    for q in warm_q:
        call(q, c)
    kernel_ms, hits, outs, allocations = 0.0, 0, [], 0
    torch.cuda.synchronize()
    t = time.time()
    for q in queries:
        st = call(q, c)
        kernel_ms += st["kernel_ms"]
        allocations += st["allocations"]
        outs.append((ids_d.cpu().numpy(), cnt_d.cpu().numpy()))
    wall = time.time() - t
    for (ids, cnt), tr in zip(outs, truth):
        for i in range(nq):
            hits += len(set(ids[i, :cnt[i]].tolist()) & set(tr[i].tolist()))
    n = nq * len(queries)
    out = {"queries_per_s_wall_incl_copies": round(n / wall), "search_kernels_ms_per_call": round(kernel_ms / len(queries), 3),
           "recall_at_10": round(hits / (10.0 * n), 4), "allocations": allocations, "row_storage": idx.row_storage(),
           "refine_storage": idx.refine_storage()}
    if c is not None:
        out["rescore_kernel_ms_per_call"] = rescore_ms(queries[-1], c)
        out["set_refine_rows_s"] = state["set_s"]
    return out


legs = [("fp8 plain", "fp8", None, None)]
for c in cands:
    legs += [(f"fp8 + f32 refine on the device, candidates {c}", "fp8", "device", c),
             (f"fp8 + f32 refine on the host, candidates {c}", "fp8", "host", c),
             (f"bf16 + f32 refine on the host, candidates {c}", "bf16", "host", c)]
legs.sort(key=lambda l: (l[1], str(l[2])))  # (few provider / table swaps per repeat)
reps = {l[0]: [] for l in legs}
for _ in range(args.repeats):
    for name, rows, refine, c in legs:
        reps[name].append(run(rows, refine, c))
result = {"what": "refine_perf", "dataset": "M", "nodes": N, "dim": d, "ef": ef, "k": k, "steps": args.steps,
          "queries_per_step": nq, "repeats": args.repeats, "graph": "LeannIndex.build, paper_default, diverse, batch 4096",
          "build_s": round(build_s, 2), "fp8_scale_exp": scale_exp, "legs": {}}
for name in reps:
    med = dict(reps[name][0])
    for f in ("queries_per_s_wall_incl_copies", "search_kernels_ms_per_call", "rescore_kernel_ms_per_call"):
        if f in med:
            med[f] = statistics.median(r[f] for r in reps[name])
    result["legs"][name] = {"median": med, "repeats": reps[name]}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(json.dumps(result), flush=True)
