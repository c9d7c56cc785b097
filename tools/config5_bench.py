"""BASELINE config 5 end to end: 10M x 4096 bf16 rows, query batch 4096 -- the MFMA distance-GEMM
stress (benches/vector_ops.rs batch_calculate as ONE query x row GEMM on the bf16 matrix cores),
PQ distance tables + codes (benches/pq_compression.rs shapes: build_distance_tables,
table_distance), the two-level re-rank search over them and the plain traversal over the bf16 rows.

    python tools/config5_bench.py [--nodes 10000000] [--dim 4096] [--nq 4096] [--graph harness|product]

One JSON line with both rooflines: `mfma` for the distance GEMM (flops / kernel time against the
2.5 PFLOP/s dense bf16 peak), `hbm` for the traversal (SURVEY 8d bytes with s = 2 / wall time
against 8 TB/s).  Rows are generated and kept in bf16 only (82 GB at 10M x 4096; never a 164 GB
float32 copy): the harness of tools/synth.py builds the graph on the bf16 rows, ground truth is
the exact top-k under the library's own bf16 distance GEMM.  --graph product takes the index from the
library's own builder instead (LeannIndex.build_bf16 on the resident bf16 rows, the diverse rule)."""
import argparse
import ctypes as C
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
os.environ.setdefault("GPU_MAX_HW_QUEUES", "32")

import numpy as np
import torch

import islands_amd as ia
from islands_amd import _check, _ffi
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth


def log(msg):
    print(f"[config5 {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=4096)
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--ef", type=int, default=128)
    ap.add_argument("--pq-m", type=int, default=64)
    ap.add_argument("--ratio", type=float, default=0.3, help="re-rank ratio of the two-level search's headline point")
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--distinct-batches", type=int, default=0,
                    help="query batches the steps cycle through, each with its own ground truth (0 = steps + warmup: "
                         "no two launches of the run traverse the same queries)")
    ap.add_argument("--tl-steps", type=int, default=8, help="batches per operating point of the two-level sweep")
    ap.add_argument("--tl-ratios", default="0.3,0.5,0.7,0.85,1.0")
    ap.add_argument("--tl-efs", default="128,256")
    ap.add_argument("--skip-two-level", action="store_true")
    ap.add_argument("--graph", choices=["harness", "product"], default="harness",
                    help="harness: synth.build_graph; product: the library's builder over the bf16 rows (diverse rule)")
    ap.add_argument("--build-batch", type=int, default=4096, help="--graph product: nodes inserted per step")
    ap.add_argument("--graph-only", action="store_true", help="stop after the graph (harness check)")
    a = ap.parse_args()
    N, d, nq, k, ef = a.nodes, a.dim, a.nq, a.k, a.ef
    dev = torch.device("cuda:0")
    lib = _ffi.lib()

    # ---- rows: bf16 only, generated chunk by chunk
    t0 = time.time()
    x16 = torch.empty((N, d), dtype=torch.bfloat16, device=dev)
    step = synth.CHUNK * 4
    for o in range(0, N, step):
        c = min(step, N - o)
        x16[o:o + c] = synth.make_rows(N, d, o, c, device=dev).to(torch.bfloat16)
    torch.cuda.synchronize()
    log(f"{N} x {d} bf16 rows ({N * d * 2 / 1e9:.1f} GB) in {time.time() - t0:.1f}s")
    nb_batches = a.distinct_batches if a.distinct_batches > 0 else a.steps + a.warmup
    q16s, qfs = [], []
    for b in range(nb_batches):
        qb = synth.make_rows(N, d, b * nq, nq, device=dev, query=True).to(torch.bfloat16).contiguous()
        q16s.append(qb)
        qfs.append(qb.to(torch.float32).contiguous())  # the queries' exact f32 images (what the traversal takes)

    # ---- the dense side: every (query, row) distance as a bf16 GEMM, block by block, + exact top-k
    # (one pass per distinct query batch: it is also that batch's ground truth)
    t0 = time.time()
    block = 65536
    out = torch.empty((nq, block), dtype=torch.float32, device=dev)
    gemm_ms = 0.0
    truths = []
    # the rows are resident: their sums of squares are computed ONCE (isl_row_sumsq_bf16) and handed to every
    # block call (round 3 recomputed them per call: a tenth of it).  Round 4: the blocks are ENQUEUED
    # (isl_distance_matrix_bf16_enqueue) on the stream the top-k runs on -- GEMM, top-k, GEMM, ... with no host
    # synchronisation in between; each block's GEMM is timed by its own pair of events and the pairs are read
    # once per batch.  (Round 3 synchronised around every block call: the chip idled between blocks and every
    # GEMM started on dropped clocks.)
    row_ss = torch.empty(N, dtype=torch.float32, device=dev)
    _check(lib.isl_row_sumsq_bf16(C.c_void_p(x16.data_ptr()), N, d, C.c_void_p(row_ss.data_ptr()), ia.MEM_DEVICE, 0, None))
    q_ss = torch.empty(nq, dtype=torch.float32, device=dev)
    nblocks = (N + block - 1) // block
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(nblocks)]
    for b, q16 in enumerate(q16s):
        _check(lib.isl_row_sumsq_bf16(C.c_void_p(q16.data_ptr()), nq, d, C.c_void_p(q_ss.data_ptr()), ia.MEM_DEVICE, 0, None))
        best_d = torch.full((nq, k), float("inf"), device=dev)
        best_i = torch.zeros((nq, k), dtype=torch.int64, device=dev)
        for bi, o in enumerate(range(0, N, block)):
            c = min(block, N - o)
            ev0, ev1 = evs[bi]
            ev0.record()
            _check(lib.isl_distance_matrix_bf16_enqueue(0, C.c_void_p(q16.data_ptr()), nq, C.c_void_p(x16[o:o + c].data_ptr()), c, d,
                                                        C.c_void_p(q_ss.data_ptr()), C.c_void_p(row_ss[o:o + c].data_ptr()),
                                                        C.c_void_p(out.data_ptr()), 0, None))
            ev1.record()
            dd, ii = torch.topk(out.view(-1)[:nq * c].view(nq, c), k, dim=1, largest=False)  # [nq][c], dense
            cat_d = torch.cat([best_d, dd], 1)
            cat_i = torch.cat([best_i, ii + o], 1)
            sel = torch.topk(cat_d, k, dim=1, largest=False).indices
            best_d, best_i = torch.gather(cat_d, 1, sel), torch.gather(cat_i, 1, sel)
        torch.cuda.synchronize()
        gemm_ms += sum(e0.elapsed_time(e1) for e0, e1 in evs)
        truths.append(best_i)
        if b % 4 == 0:
            log(f"ground truth of batch {b + 1} / {nb_batches} ({time.time() - t0:.0f}s)")
    gemm_flops = 2.0 * nq * N * d * nb_batches
    gemm_tflops = gemm_flops / (gemm_ms * 1e-3) / 1e12
    log(f"distance GEMM over all rows, {nb_batches} query batches: {gemm_ms:.1f} ms of kernels = {gemm_tflops:.0f} TFLOP/s; "
        f"with top-k {time.time() - t0:.1f}s")
    del out

    # ---- graph (harness) on the bf16 rows
    t0 = time.time()
    # (every harness GEMM on float32 operands and every per-chunk tensor within 1 GiB: round 2 lost a box
    # to a GPU memory access fault inside this builder on bf16 operands at d = 4096 -- tools/synth.py,
    # _CHUNK_BYTES, has what is known about it)
    if a.graph == "product":
        # isl_index_build_rows: the graph is built over the bf16 rows and the index keeps its own copy of them
        idx = ia.LeannIndex.build_bf16(config=ia.LeannConfig.paper_default(), batch=a.build_batch, select="diverse",
                                       device_ptr=x16.view(torch.int16).data_ptr(), n=N, d=d)
        sample = np.random.default_rng(0).integers(1, N, size=min(N - 1, 20000))
        degs = np.array([len(idx.get_neighbors(int(i))) for i in sample])
        gst = {"builder": "LeannIndex.build_bf16, diverse rule", "nodes_per_step": a.build_batch,
               "build_s": round(time.time() - t0, 1), "mean_degree_of_sample": round(float(degs.mean()), 2),
               "min_degree_of_sample": int(degs.min())}
        log(f"graph: {gst}")
        if a.graph_only:
            return
    else:
        off, nb, entry = synth.build_graph(x16, m0=60, precise=True)
        torch.cuda.synchronize()
        gst = synth.graph_stats(off)
        gst["build_s"] = round(time.time() - t0, 1)
        log(f"graph in {time.time() - t0:.1f}s: {gst}")
        if a.graph_only:
            return
        idx = ia.LeannIndex.from_device_csr(off.data_ptr(), nb.data_ptr(), N, entry, d, ia.LeannConfig.paper_default(), device=0)
        del off, nb
        idx.set_embeddings_bf16(None, device_ptr=x16.view(torch.int16).data_ptr(), n=N, d=d)
    torch.cuda.synchronize()
    log("index resident (its own copy of the bf16 rows)")

    # ---- PQ side: codebooks + codes (harness training), tables in the timed search
    res_tl = None
    if not a.skip_two_level:
        t0 = time.time()
        cb, codes = synth.train_pq(x16, a.pq_m)
        pq = ia.ProductQuantizer(d, cb.cpu().numpy())
        idx.set_pq_codes(pq, None, device_ptr=codes.data_ptr(), n=N)
        del codes
        torch.cuda.synchronize()
        log(f"PQ m={a.pq_m} K=256 trained and {N} rows encoded in {time.time() - t0:.1f}s")
    del x16
    torch.cuda.empty_cache()

    depth = a.depth
    idx.prepare(nq, max(ef, max(int(e) for e in a.tl_efs.split(","))), k, depth)
    outs = [(torch.zeros((nq, k), dtype=torch.int64, device=dev), torch.zeros((nq, k), dtype=torch.float32, device=dev),
             torch.zeros(nq, dtype=torch.int32, device=dev)) for _ in range(depth)]

    def pipelined(first, count, submit):
        """`count` steps with `depth` calls in flight; step s answers query batch s % nb_batches; returns the summed
        counters and the recall over every step's answers against that batch's own ground truth."""
        agg = {"expansions": 0, "edges": 0, "evals": 0, "pushes": 0, "queries": 0, "kernel_ms": 0.0, "exact_path": 0}
        hits, pend = [], []

        def finish():
            s_, tok = pend.pop(0)
            st = idx.wait_stats(tok)
            for f in agg:
                agg[f] += st[f]
            o = outs[s_ % depth]
            hits.append(synth.recall_at_k(o[0], o[2], truths[s_ % nb_batches]))

        for s_ in range(first, first + count):
            o = outs[s_ % depth]
            pend.append((s_, submit(qfs[s_ % nb_batches], o)))
            if len(pend) >= depth:
                finish()
        while pend:
            finish()
        return agg, float(np.mean(hits))

    # ---- traversal over the bf16 rows (LeannIndex::search), `depth` batches in flight
    def plain(efv):
        return lambda q_, o: idx.search_batch_device_async(q_.data_ptr(), nq, d, k, efv, o[0].data_ptr(), o[1].data_ptr(),
                                                           o[2].data_ptr())

    gc.collect()
    gc.disable()  # (a full collection of the interpreter takes tens of milliseconds with torch imported)
    pipelined(0, a.warmup, plain(ef))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    agg, rec = pipelined(a.warmup, a.steps, plain(ef))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    bytes_total = agg["evals"] * d * 2 + 4 * agg["edges"] + 8 * agg["expansions"] + agg["queries"] * (4 * d + 12 * k)
    hbm_gbs = bytes_total / dt / 1e9
    log(f"traversal: {a.steps * nq / dt:.0f} q/s, recall {rec:.4f}, {hbm_gbs:.0f} GB/s algorithmic")

    if not a.skip_two_level:
        # Operating points of the PQ re-rank path (build_distance_tables for the batch + two-level search,
        # extension), `depth` calls in flight like the plain traversal, every step its own queries.
        # Algorithmic bytes per query: promoted rows V * d * 2 + codes A * m * 2 + 4 E + 8 H + 4 d + 12 k.
        def two_level(efv, ratio):
            return lambda q_, o: idx.search_two_level_batch_device_async(q_.data_ptr(), nq, d, k, efv, ratio, o[0].data_ptr(),
                                                                         o[1].data_ptr(), o[2].data_ptr())

        points = []
        for efv in [int(e) for e in a.tl_efs.split(",")]:
            for ratio in [float(r) for r in a.tl_ratios.split(",")]:
                pipelined(0, 2, two_level(efv, ratio))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ag, rc = pipelined(2, a.tl_steps, two_level(efv, ratio))
                torch.cuda.synchronize()
                dtl = time.perf_counter() - t0
                nqq = ag["queries"]
                by = ag["evals"] * d * 2 + ag["pushes"] * a.pq_m * 2 + 4 * ag["edges"] + 8 * ag["expansions"] + nqq * (4 * d + 12 * k)
                pt = {"ef": efv, "rerank_ratio": ratio, "value": round(nqq / dtl, 1), "unit": "queries/s",
                      "recall_at_10": round(rc, 4), "exact_evals_per_query": round(ag["evals"] / nqq, 1),
                      "approx_evals_per_query": round(ag["pushes"] / nqq, 1),
                      "hops_per_query": round(ag["expansions"] / nqq, 1),
                      "algorithmic_gbs": round(by / dtl / 1e9, 1), "hbm_frac": round(by / dtl / 1e9 / 8000.0, 4)}
                points.append(pt)
                log(f"two-level {pt}")
        good = [p_ for p_ in points if p_["recall_at_10"] >= 0.95]
        best = max(good, key=lambda p_: p_["value"]) if good else None
        head = next((p_ for p_ in points if p_["ef"] == ef and abs(p_["rerank_ratio"] - a.ratio) < 1e-6), points[0])
        res_tl = dict(head)
        res_tl.update({"pq": {"m": a.pq_m, "K": 256, "dsub": d // a.pq_m}, "calls_in_flight": depth,
                       "steps_per_point": a.tl_steps, "operating_points": points,
                       "fastest_point_with_recall_at_least_0.95": best,
                       "plain_traversal_for_comparison": {"value": round(a.steps * nq / dt, 1), "recall_at_10": round(rec, 4),
                                                          "evals_per_query": round(agg["evals"] / agg["queries"], 1)},
                       "note": "build_distance_tables for the batch + two-level traversal (extension, DESIGN 3.6), pipelined "
                               "through isl_search_two_level_batch_device_async"})

    print(json.dumps({
        "metric": "BASELINE config 5: 10M x 4096 bf16, query batch 4096 (distance GEMM + PQ re-rank + traversal)",
        "graph_source": a.graph,
        "value": round(a.steps * nq / dt, 1), "unit": "queries/s", "recall_at_10": round(rec, 4),
        "config": {"workload": f"{N} x {d} bf16 rows resident in HBM, query batch {nq}, k={k}, ef={ef}, cosine, "
                               f"{depth} batches in flight", "graph": gst, "distinct_batches": nb_batches,
                   "per_query": {"expansions": round(agg["expansions"] / agg["queries"], 1),
                                 "edges": round(agg["edges"] / agg["queries"], 1),
                                 "evals": round(agg["evals"] / agg["queries"], 1)},
                   "exact_path_queries": agg["exact_path"]},
        "roofline": {"bound": "hbm", "achieved": round(hbm_gbs, 1), "peak": 8000.0, "unit": "GB/s",
                     "frac": round(hbm_gbs / 8000.0, 4), "kernel": "leann_search_fast<2,cosine,bf16 rows>",
                     "per_launch_kernel_ms": round(agg["kernel_ms"] / a.steps, 3)},
        "roofline_mfma": {"bound": "mfma", "achieved": round(gemm_tflops, 1), "peak": 2500.0, "unit": "TFLOP/s",
                          "frac": round(gemm_tflops / 2500.0, 4), "kernel": "gemm_tn_bf16_ph8<cosine> 256x256 (isl_distance_matrix_bf16_enqueue)",
                          "flops": gemm_flops, "kernel_ms_total": round(gemm_ms, 1),
                          "note": f"every (query, row) cosine distance of {nb_batches} query batches: {nq} x {N} x {d} each, in "
                                  f"blocks of {block} rows, enqueued back to back with the top-k between them (no host synchronisation "
                                  f"inside a batch); the time is the sum of the per-block event pairs around the GEMM launches"},
        "two_level": res_tl,
    }))


if __name__ == "__main__":
    main()
