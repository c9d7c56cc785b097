"""Build time and quality of the device graph builder (isl_index_build_rows) in its batched mode.
    python tools/build_perf.py [build|insert|remove] [--nodes N] [--dim D] [--batch B] [--dataset G|M] [--select reference|diverse]
                               [--alpha A] [--no-keep-pruned] [--ef 128,256] [--nq Q] [--check-truth]
                               [--row-dtype f32|bf16[,...]] [--reserve ROWS]
Prints one JSON line per leg: build seconds, peak device memory during the build, recall@10 / evaluations /
hops per query at every ef, mean and minimum degree.  Dataset G = synth.make_rows (clustered, the headline
rows), M = synth.make_manifold.  --row-dtype names the legs, built one after the other in this process
(f32,bf16,f32,bf16 alternates them).  With a bf16 leg the generated rows are rounded to bf16 once and every
leg builds from those values -- the f32 legs from their widened images -- so all legs build the same graph
problem, and the truth is the brute force over the widened rows.

`insert` measures isl_index_insert instead (f32 rows; defaults: dataset M, diverse rule, 1024 queries, recall at
the first --ef): an index of N - K rows (--insert-rows K, default 65536) takes the last K rows in one call; a second
copy of it takes them in --insert-calls calls (default 16); then one more row goes into that copy -- the fixed
cost of a call -- and the one-call build of all N rows stands beside them.  One JSON line: seconds per call and
rows/s, and recall@10 of the two grown graphs and of the one-call graph against isl_bruteforce_topk.

`remove` measures isl_index_remove (same defaults): K random rows (--insert-rows) leave an index of N rows in one
call; a copy of it loses them in --insert-calls calls; one more row leaves that copy -- the fixed cost of a call.
Beside them stand the one-call build of the survivors (the yardstick for time and for recall) and the same graph
with the removed ids merely dropped from the lists.  A third copy repeats the one-call removal under ISL_DEBUG for
the number of touched nodes, the sum of |C(p)| and the repair kernel's time, with the device's memory polled.  The
truth is isl_bruteforce_topk over the survivors.

--reserve ROWS (insert, remove): every index that grows or shrinks first reserves room for ROWS rows
(LeannIndex.reserve), so that the calls append and compact in place.  Either way the line carries, for every measured
call, the device bytes in use before and after it and the handle's row_allocations, and for the one-row call its
split into phases as the library times them under ISL_DEBUG (rows: fill or copy; list_import; construction or
repair; csr_export; padded_adjacency; rows_in_place: the compaction of a reserved table; adopt), in milliseconds."""
import argparse, json, os, sys, threading, time
sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import numpy as np, torch
import islands_amd as ia
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth

ap = argparse.ArgumentParser()
ap.add_argument("mode", nargs="?", choices=["build", "insert", "remove"], default="build")
ap.add_argument("--insert-rows", type=int, default=65536)
ap.add_argument("--insert-calls", type=int, default=16)
ap.add_argument("--nodes", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--dataset", choices=["G", "M"], default=None, help="default G (build), M (insert)")
ap.add_argument("--select", choices=["reference", "diverse"], default=None, help="default reference (build), diverse (insert)")
ap.add_argument("--alpha", type=float, default=1.0)
ap.add_argument("--no-keep-pruned", action="store_true")
ap.add_argument("--ef", default="128,256", help="comma-separated ef values of the recall measurement")
ap.add_argument("--nq", type=int, default=None, help="default 512 (build), 1024 (insert)")
ap.add_argument("--qstart", type=int, default=0, help="dataset G: first row of the query stream (bench.py's batch b starts at 1024 b)")
ap.add_argument("--row-dtype", default="f32", help="comma-separated legs, each f32 or bf16")
ap.add_argument("--reserve", type=int, default=0, help="insert / remove: reserve room for this many rows first")
ap.add_argument("--check-truth", action="store_true", help="also report how far torch's brute force agrees with the truth")
args = ap.parse_args()
removing = args.mode == "remove"
inserting = args.mode == "insert" or removing
args.dataset = args.dataset or ("M" if inserting else "G")
args.select = args.select or ("diverse" if inserting else "reference")
args.nq = args.nq or (1024 if inserting else 512)
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


def recall_at_10(idx, ef):
    ids, dist, cnt = idx.search_batch(qh, 10, ef)
    hit = sum(len(set(ids[i, :cnt[i]].tolist()) & set(ti[i].tolist())) for i in range(nq))
    return round(hit / (10.0 * nq), 4)


def used_bytes():
    free, total = torch.cuda.mem_get_info(0)  # hipMemGetInfo: the whole device, whoever allocated
    return total - free


def reserved(idx):
    return idx.reserve(args.reserve) if args.reserve else idx


def accounted(idx, f):
    """(f(), seconds, {device bytes before / after the call, row_allocations after it})"""
    before = used_bytes()
    t = time.time()
    r = f()
    dt = time.time() - t
    return r, dt, {"seconds": round(dt, 4), "device_bytes_before": before, "device_bytes_after": used_bytes(),
                   "capacity": idx.capacity}


def phases_of(f):
    """f() under ISL_DEBUG (read by the call itself) with stderr to a file: (f(), the stderr text, the phases in ms)"""
    import re, tempfile
    with tempfile.TemporaryFile() as tmp:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        os.environ["ISL_DEBUG"] = "1"
        try:
            r = f()
        finally:
            del os.environ["ISL_DEBUG"]
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    m = re.search(r"phases:((?: \w+=[0-9.]+)*)", text)
    return r, text, ({k: float(v) for k, v in (kv.split("=") for kv in m.group(1).split())} if m else None)


def insert_mode():
    K, calls = args.insert_rows, args.insert_calls
    if legs != ["f32"] or not 0 < K < N or K % calls:
        ap.error("insert: f32 rows, 0 < --insert-rows < --nodes, a multiple of --insert-calls")
    n0, ef = N - K, int(args.ef.split(",")[0])
    kw = dict(batch=args.batch, select=args.select, alpha=args.alpha, keep_pruned=not args.no_keep_pruned)

    def timed(f):
        t = time.time()
        r = f()
        return r, time.time() - t

    one, base_s = timed(lambda: ia.LeannIndex.build(xh[:n0], cfg, **kw))
    reserved(one)
    _, one_s, one_acc = accounted(one, lambda: one.insert(xh[n0:], **kw))
    assert len(one) == N
    recall_one = recall_at_10(one, ef)
    del one
    many = reserved(ia.LeannIndex.build(xh[:n0], cfg, **kw))
    step, per_call = K // calls, []
    for c in range(calls):
        first, dt = timed(lambda: many.insert(xh[n0 + c * step:n0 + (c + 1) * step], **kw))
        assert first == n0 + c * step
        per_call.append(round(dt, 3))
    recall_many = recall_at_10(many, ef)
    extra = synth.make_manifold(1, d, 977, device=dev).cpu().numpy() if args.dataset == "M" else xh[:1] * np.float32(0.5)
    _, single_s, single_acc = accounted(many, lambda: many.insert(extra, **kw))
    assert len(many) == N + 1
    _, _, single_phases = phases_of(lambda: many.insert(extra * np.float32(0.75), **kw))  # one more, timed inside
    del many
    whole, whole_s = timed(lambda: ia.LeannIndex.build(xh, cfg, **kw))
    print(json.dumps({
        "what": "build_perf insert", "dataset": args.dataset, "nodes": N, "dim": d, "batch": args.batch,
        "select": args.select, "alpha": args.alpha, "keep_pruned": not args.no_keep_pruned, "m0": cfg.m0,
        "ef_construction": cfg.ef_construction, "inserted_rows": K, "build_base_s": round(base_s, 2),
        "one_call": {"seconds": round(one_s, 3), "rows_per_s": round(K / one_s)},
        "many_calls": {"calls": calls, "rows_per_call": step, "seconds_per_call": per_call,
                       "seconds": round(sum(per_call), 3), "rows_per_s": round(K / sum(per_call))},
        "one_row_call_s": round(single_s, 3),
        "reserve_rows": args.reserve, "one_call_account": one_acc, "one_row_call_account": single_acc,
        "one_row_call_phases_ms": single_phases,
        "one_call_build": {"seconds": round(whole_s, 2), "nodes_per_s": round(N / whole_s)},
        "queries": nq, "ef": ef,
        "recall_at_10": {"grown_one_call": recall_one, "grown_many_calls": recall_many,
                         "one_call_build": recall_at_10(whole, ef)}}), flush=True)


def remove_mode():
    import re
    global ti
    K, calls = args.insert_rows, args.insert_calls
    if legs != ["f32"] or not 0 < K < N or K % calls:
        ap.error("remove: f32 rows, 0 < --insert-rows < --nodes, a multiple of --insert-calls")
    ef = int(args.ef.split(",")[0])
    kw = dict(batch=args.batch, select=args.select, alpha=args.alpha, keep_pruned=not args.no_keep_pruned)
    rule = dict(select=args.select, alpha=args.alpha, keep_pruned=not args.no_keep_pruned)
    gone = np.sort(np.random.default_rng(7).choice(N, K, replace=False)).astype(np.uint64)
    mask = np.ones(N, bool)
    mask[gone] = False
    xs = np.ascontiguousarray(xh[mask])
    xd = torch.from_numpy(xs).to(dev)
    ti = synth.brute_force_topk_native(xd, q, 10)[0].cpu().numpy()  # the truth over the survivors, in their new ids
    del xd
    torch.cuda.empty_cache()

    def timed(f):
        t = time.time()
        r = f()
        return r, time.time() - t

    def copy_of(blob, rows):
        return reserved(ia.LeannIndex.from_bytes(blob).upload(0).set_embeddings(rows))

    scratch, scratch_s = timed(lambda: ia.LeannIndex.build(xs, cfg, **kw))
    recall_scratch = recall_at_10(scratch, ef)
    del scratch
    one, whole_s = timed(lambda: ia.LeannIndex.build(xh, cfg, **kw))
    blob = one.to_bytes()
    # the old graph with the removed ids merely dropped from the lists
    remap0 = np.full(N, -1, np.int64)
    remap0[mask] = np.arange(N - K)
    lists = [one.get_neighbors(int(p)) for p in np.flatnonzero(mask)]
    touched_host = sum(1 for r in lists if r.size and (remap0[r.astype(np.int64)] < 0).any())
    kept = [remap0[r.astype(np.int64)] for r in lists]
    kept = [r[r >= 0].astype(np.uint64) for r in kept]
    off = np.zeros(N - K + 1, np.uint64)
    off[1:] = np.cumsum([r.size for r in kept])
    g = ia.CsrGraph(node_offsets=off, neighbors=np.concatenate(kept), levels=np.zeros(N - K, np.uint64),
                    entry_point=max(int(remap0[one.entry_point]), 0), num_nodes=N - K,
                    degree_counts=np.diff(off.astype(np.int64)).astype(np.uint64))
    dropped = ia.LeannIndex.from_csr(g, cfg, dimension=d).upload(0).set_embeddings(xs)
    recall_dropped = recall_at_10(dropped, ef)
    del dropped, lists, kept, g
    reserved(one)
    remap, one_s, one_acc = accounted(one, lambda: one.remove(gone, **rule))
    assert len(one) == N - K and (remap[mask] == np.arange(N - K, dtype=np.uint64)).all()
    recall_one = recall_at_10(one, ef)
    del one
    many = copy_of(blob, xh)
    step, per_call, left = K // calls, [], gone.copy()
    for c in range(calls):
        r, dt = timed(lambda: many.remove(left[:step], **rule))
        left = r[left[step:]]  # the ids still to go, in the numbering the call left
        per_call.append(round(dt, 3))
    assert len(many) == N - K
    recall_many = recall_at_10(many, ef)
    _, single_s, single_acc = accounted(many, lambda: many.remove([(N - K) // 2], **rule))
    _, _, single_phases = phases_of(lambda: many.remove([(N - K) // 3], **rule))  # one more, timed inside
    del many
    # once more under ISL_DEBUG (read by the call itself), stderr to a file, the device's memory polled
    dbg = copy_of(blob, xh)
    before, peak, stop = used_bytes(), [0], threading.Event()

    def poll():
        while not stop.is_set():
            peak[0] = max(peak[0], used_bytes())
            time.sleep(0.005)

    th = threading.Thread(target=poll, daemon=True)
    th.start()
    _, text, _ = phases_of(lambda: dbg.remove(gone, **rule))
    stop.set()
    th.join()
    m = re.search(r"touched (\d+), candidates (\d+), repair kernel ([0-9.]+) ms", text)
    touched, cands, kernel_ms = (int(m.group(1)), int(m.group(2)), float(m.group(3))) if m else (None, None, None)
    after = used_bytes()
    del dbg
    row_bytes = None if not m else cands * d * 4
    print(json.dumps({
        "what": "build_perf remove", "dataset": args.dataset, "nodes": N, "dim": d, "batch": args.batch,
        "select": args.select, "alpha": args.alpha, "keep_pruned": not args.no_keep_pruned, "m0": cfg.m0,
        "ef_construction": cfg.ef_construction, "removed_rows": K, "build_all_s": round(whole_s, 2),
        "one_call": {"seconds": round(one_s, 3), "rows_per_s": round(K / one_s)},
        "many_calls": {"calls": calls, "rows_per_call": step, "seconds_per_call": per_call,
                       "seconds": round(sum(per_call), 3), "rows_per_s": round(K / sum(per_call))},
        "one_row_call_s": round(single_s, 3),
        "reserve_rows": args.reserve, "one_call_account": one_acc, "one_row_call_account": single_acc,
        "one_row_call_phases_ms": single_phases,
        "one_call_build_of_survivors": {"seconds": round(scratch_s, 2), "nodes_per_s": round((N - K) / scratch_s)},
        "queries": nq, "ef": ef,
        "recall_at_10": {"repaired_one_call": recall_one, "repaired_many_calls": recall_many,
                         "build_of_survivors": recall_scratch, "removed_ids_merely_dropped": recall_dropped},
        "touched_nodes": touched, "touched_nodes_counted_on_host": touched_host, "sum_candidates": cands,
        "mean_candidates": None if not touched else round(cands / touched, 2),
        "repair_kernel_ms": kernel_ms, "repair_row_bytes": row_bytes,
        "repair_row_gbytes_per_s": None if not kernel_ms else round(row_bytes / kernel_ms / 1e6, 1),
        "device_bytes_before": before, "device_bytes_peak_in_remove": max(peak[0], before),
        "device_bytes_after": after}), flush=True)


if inserting:
    remove_mode() if removing else insert_mode()
    sys.exit(0)


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
