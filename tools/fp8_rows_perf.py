"""fp8 e4m3 rows beside bf16 and f32 rows on one graph, in one run: what a byte per element costs and buys.
    python tools/fp8_rows_perf.py [--nodes 1000000] [--dim 768] [--steps 20] [--ef 128] [--repeats 3]
                                  [--out profiles/fp8_rows.json]
Dataset M of tools/synth.py.  ONE graph, built by the library from the f32 rows; the same rows are then attached
as f32, as bf16 (torch's round-to-nearest cast) and as fp8 (quantised on the device: the smallest power-of-two
scale that brings max|x| under 448, a clamp, torch's cast to float8_e4m3fn; the codes go in by device pointer).
Every leg runs `steps` device-buffer calls of 1024 queries (fresh manifold batches, k = 10) after two warm-up
calls on a prepared index; the legs alternate and repeat, and the JSON keeps every repeat beside the median.
Per type: queries/s (wall clock over the timed calls, and from the calls' HIP-event kernel time), evaluations V
per query, the algorithmic bytes of SURVEY.md section 8d with s = 4 / 2 / 1 and their fraction of the 8 TB/s HBM
peak over the kernel time, and recall@10 against the library's f32 brute force over the f32 rows."""
import argparse, json, math, os, statistics, sys, time
sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import numpy as np, torch
import islands_amd as ia
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth

HBM_PEAK = 8.0e12
ELEM = {"f32": 4, "bf16": 2, "fp8": 1}

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--ef", type=int, default=128)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--types", default="f32,bf16,fp8")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                               "fp8_rows.json"))
args = ap.parse_args()
N, d, k, nq = args.nodes, args.dim, 10, 1024
dev = torch.device("cuda:0")

x = synth.make_manifold(N, d, 42, device=dev)
warm_q = [synth.make_manifold(nq, d, 4200 + b, device=dev) for b in range(2)]
queries = [synth.make_manifold(nq, d, 4300 + b, device=dev) for b in range(args.steps)]
truth = [synth.brute_force_topk_native(x, q, k)[0].cpu().numpy() for q in queries]
t0 = time.time()
idx = ia.LeannIndex.build(x.cpu().numpy(), ia.LeannConfig.paper_default(), batch=4096, select="diverse")
build_s = time.time() - t0

# the three stored forms of the same rows, on the device
top = float(x.abs().max())
scale_exp = max(-32, min(32, math.ceil(math.log2(top / 448.0)))) if top > 0 else -32
while scale_exp < 32 and top * 2.0 ** -scale_exp > 448.0:
    scale_exp += 1
while scale_exp > -32 and top * 2.0 ** -(scale_exp - 1) <= 448.0:
    scale_exp -= 1
stored = {
    "f32": x,
    "bf16": x.to(torch.bfloat16),
    "fp8": (x * 2.0 ** -scale_exp).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8),
}
torch.cuda.synchronize()
ids_d = torch.zeros((nq, k), dtype=torch.int64, device=dev)
dist_d = torch.zeros((nq, k), dtype=torch.float32, device=dev)
cnt_d = torch.zeros(nq, dtype=torch.int32, device=dev)


def attach(leg):
    p = stored[leg].data_ptr()
    if leg == "f32":
        idx.set_embeddings(None, device_ptr=p, n=N, d=d)
    elif leg == "bf16":
        idx.set_embeddings_bf16(None, device_ptr=p, n=N, d=d)
    else:
        idx.set_embeddings_fp8(None, scale_exp, device_ptr=p, n=N, d=d)
    idx.prepare(nq, args.ef, k, 2)


def call(q):
    idx.search_batch_device(q.data_ptr(), nq, d, k, args.ef, ids_d.data_ptr(), dist_d.data_ptr(), cnt_d.data_ptr())
    return idx.last_stats()


def run(leg):
    attach(leg)
    for q in warm_q:
        call(q)
    tot = {f: 0 for f in ("queries", "expansions", "edges", "evals", "exact_path", "replayed", "allocations")}
    kernel_ms, hits, outs = 0.0, 0, []
    torch.cuda.synchronize()
    t = time.time()
    for q in queries:
        st = call(q)
        for f in tot:
            tot[f] += st[f]
        kernel_ms += st["kernel_ms"]
        outs.append((ids_d.cpu().numpy(), cnt_d.cpu().numpy()))
    wall = time.time() - t
    for (ids, cnt), tr in zip(outs, truth):
        for i in range(nq):
            hits += len(set(ids[i, :cnt[i]].tolist()) & set(tr[i].tolist()))
    n = nq * len(queries)
    alg = tot["evals"] * d * ELEM[leg] + 4 * tot["edges"] + 8 * tot["expansions"] + n * (4 * d + 12 * k)
    return {"queries_per_s_wall_incl_copies": round(n / wall), "queries_per_s_kernels": round(n / (kernel_ms / 1e3)),
            "evals_per_query": round(tot["evals"] / n, 1), "hops_per_query": round(tot["expansions"] / n, 1),
            "algorithmic_bytes_per_query": round(alg / n), "hbm_frac_kernels": round(alg / (kernel_ms / 1e3) / HBM_PEAK, 4),
            "recall_at_10": round(hits / (10.0 * n), 4), "exact_path": tot["exact_path"], "replayed": tot["replayed"],
            "allocations": tot["allocations"], "row_storage": idx.row_storage()}


legs = args.types.split(",")
reps = {leg: [] for leg in legs}
for _ in range(args.repeats):
    for leg in legs:
        reps[leg].append(run(leg))
result = {"what": "fp8_rows_perf", "dataset": "M", "nodes": N, "dim": d, "ef": args.ef, "k": k, "steps": args.steps,
          "queries_per_step": nq, "repeats": args.repeats, "graph": "LeannIndex.build, paper_default, diverse, batch 4096",
          "build_s": round(build_s, 2), "fp8_scale_exp": scale_exp, "hbm_peak_bytes_per_s": HBM_PEAK, "types": {}}
for leg in legs:
    med = dict(reps[leg][0])
    for f in ("queries_per_s_wall_incl_copies", "queries_per_s_kernels", "hbm_frac_kernels"):
        med[f] = statistics.median(r[f] for r in reps[leg])
    result["types"][leg] = {"median": med, "repeats": reps[leg]}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(json.dumps(result), flush=True)
