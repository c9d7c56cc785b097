"""Refined search on the device: the rescoring kernel alone, the refined search over fp8 and bf16 rows with the f32
originals as the refine table, and the table's lifecycle.  Ids, distance BITS and counts are compared exactly with
tests/_refine_ref.py (numpy over oracle.batch_distance); nothing here has a tolerance."""
import functools
import threading

import numpy as np
import pytest

import islands_amd as ia
import _entry_seeds_ref as ref
import _refine_ref as rref
from _data import uniform_vectors

pytestmark = pytest.mark.gpu

METRICS = [ia.DistanceMetric.Cosine, ia.DistanceMetric.Euclidean, ia.DistanceMetric.DotProduct,
           ia.DistanceMetric.Manhattan]
N_ROWS = 600
TWIN_A, TWIN_B, NAN_ROW, ZERO_ROW = 5, 9, 11, 13
GARBAGE = 0xDEADBEEFCAFEF00D


def ring_index(n, d, metric):
    """n nodes on a ring: the rescoring reads no graph and no provider rows"""
    g = ia.CsrGraph()
    for i in range(n):
        g.add_node([(i + 1) % n], 0)
    g.entry_point = 0
    return ia.LeannIndex.from_csr(g, ia.LeannConfig(metric=metric), dimension=d).upload(0)


def csr_index(csr, metric, d):
    g = ia.CsrGraph(node_offsets=csr.node_offsets, neighbors=csr.neighbors, levels=csr.levels,
                    entry_point=csr.entry_point, max_level=csr.max_level, num_nodes=csr.num_nodes,
                    degree_counts=csr.degree_counts)
    return ia.LeannIndex.from_csr(g, ia.LeannConfig(metric=metric), dimension=d).upload(0)


@functools.lru_cache(maxsize=None)
def table(d):
    """y [600, d] with two identical rows, a row with a NaN element and a zero row (DotProduct scores it -0.0, which
    ties with +0.0; Cosine takes the zero-norm branch), and 70 queries.  Read-only."""
    y = uniform_vectors(N_ROWS, d, 40 + d).astype(np.float32).copy()
    y[TWIN_B] = y[TWIN_A]
    y[NAN_ROW, d // 2] = np.nan
    y[ZERO_ROW] = 0.0
    q = uniform_vectors(70, d, 90 + d).astype(np.float32).copy()
    q[3] = 0.0  # a zero query
    y.setflags(write=False)
    q.setflags(write=False)
    return y, q


@functools.lru_cache(maxsize=None)
def candidates(c):
    """[70, c] ids and [70] counts: every row starts with the special rows (when it has room), holds a repeated id and
    an id that names no row; odd rows are short, with garbage behind their count."""
    r = np.random.default_rng(1000 + c)
    ids = r.integers(0, N_ROWS, (70, c)).astype(np.uint64)
    special = [TWIN_B, ZERO_ROW, NAN_ROW, TWIN_A, N_ROWS + 7, TWIN_B, 1 << 40, ZERO_ROW]
    for qi in range(70):
        for j, v in enumerate(special[:c]):
            ids[qi, (j * 7 + qi) % c if c >= 64 else j] = v
    cnt = np.full(70, c, np.uint32)
    for qi in range(1, 70, 2):
        cnt[qi] = max(1, c - 1 - qi % 9)
        ids[qi, cnt[qi]:] = GARBAGE
    ids[69, :] = N_ROWS  # a row in which no candidate names a row: count 0
    ids.setflags(write=False)
    cnt.setflags(write=False)
    return ids, cnt


# ---------------------------------------------------------------- rescore alone
# d = 1: no multiple of a quad; 24: a padded pitch for bf16 (and 1.5 steps of 16); 50: padded for both types; 832: 52
# steps of 16 floats, longer than one ring of loads (12) with the reload loop, and 26 bf16 steps
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [1, 24, 50, 832])
def test_rescore_matches_the_definition(orc, metric, d):
    y, q = table(d)
    tables = {"f32": (y, y), "bf16": (ref.bf16_bits(y), ref.bf16_image(ref.bf16_bits(y)))}
    want = {}  # the reference, once per (dtype, c, k, nq), shared by the placements
    for placement in ("device", "host"):
        for dtype, (stored, image) in tables.items():
            idx = ring_index(N_ROWS, d, metric)
            idx.set_refine_rows(stored, placement=placement)
            st = idx.refine_storage()
            assert (st["rows"], st["placement"], st["dtype"]) == (N_ROWS, placement, 0 if dtype == "f32" else 1)
            for c in (1, 63, 64, 65, 200, 512):
                ids, cnt = candidates(c)
                for k in sorted({1, c}):
                    for nq in (1, 70):
                        key = (dtype, c, k, nq)
                        if key not in want:
                            want[key] = rref.rescore(orc, int(metric), q[:nq], image, ids[:nq], cnt[:nq], k)
                        got = idx.rescore(q[:nq], ids[:nq], cnt[:nq], k)
                        try:
                            rref.same(got, want[key])
                        except AssertionError as e:
                            raise AssertionError(f"{placement} {dtype} c={c} k={k} nq={nq}: {e}") from None


def test_rescore_ties_nan_zero_and_ids_without_a_row(orc):
    """The cases the table and the candidate lists were made for, checked by hand on one query each."""
    d = 24
    y, q = table(d)
    for metric in METRICS:
        idx = ring_index(N_ROWS, d, metric)
        idx.set_refine_rows(y, placement="host")
        # two identical rows: equal scores, the earlier POSITION wins whichever id is smaller
        for pair in ([TWIN_B, TWIN_A], [TWIN_A, TWIN_B]):
            ids, dist, cnt = idx.rescore(q[:1], np.array([pair], np.uint64), [2], 2)
            assert cnt[0] == 2 and ids[0].tolist() == pair and dist[0, 0].tobytes() == dist[0, 1].tobytes()
        # a NaN score goes last, an id >= n is neither scored nor counted, a repeat appears twice
        cand = np.array([[NAN_ROW, N_ROWS, 20, 1 << 63, 20, 21]], np.uint64)
        ids, dist, cnt = idx.rescore(q[:1], cand, [6], 6)
        assert cnt[0] == 4 and ids[0, 3] == NAN_ROW and np.isnan(dist[0, 3]) and not np.isnan(dist[0, :3]).any()
        assert sorted(ids[0, :3].tolist()) == [20, 20, 21]
        print(f"NaN score {metric}: device {dist[0, 3].view(np.uint32):#x} "
              f"oracle {orc.batch_distance(int(metric), q[0], y[NAN_ROW:NAN_ROW + 1]).view(np.uint32)[0]:#x}")
        rref.same((ids, dist, cnt), rref.rescore(orc, int(metric), q[:1], y, cand, [6], 6))
    # DotProduct: a zero row scores -0.0, which is neither below the negative scores nor above +0.0
    idx = ring_index(N_ROWS, d, ia.DistanceMetric.DotProduct)
    idx.set_refine_rows(y)
    s = orc.batch_distance(2, q[0], y)
    neg, pos = int(np.flatnonzero(s < 0)[0]), int(np.flatnonzero(s > 0)[0])
    cand = np.array([[pos, ZERO_ROW, neg]], np.uint64)
    ids, dist, cnt = idx.rescore(q[:1], cand, [3], 3)
    assert ids[0].tolist() == [neg, ZERO_ROW, pos] and dist[0, 1].view(np.uint32) == 0x80000000
    # ... and the zero query scores every row -0.0: all equal, so the order is the candidates'
    cand = np.array([[40, 30, ZERO_ROW, 50, 30]], np.uint64)
    ids, dist, cnt = idx.rescore(q[3:4], cand, [5], 4)
    assert ids[0].tolist() == [40, 30, ZERO_ROW, 50] and (dist[0].view(np.uint32) == 0x80000000).all()


def test_rescore_behind_a_search_on_one_stream(orc):
    """isl_rescore_device composes with a search in stream order; the refined call is that pair."""
    import torch
    metric = ia.DistanceMetric.Euclidean
    idx, x, q, _ = refined_case(orc, metric, "clustered", "fp8")
    dev = torch.device("cuda:0")
    nq, d, k, cand, ef = q.shape[0], q.shape[1], 10, 32, 64
    dq = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    ci = torch.zeros((nq, cand), dtype=torch.int64, device=dev)
    cd = torch.zeros((nq, cand), dtype=torch.float32, device=dev)
    cc = torch.zeros(nq, dtype=torch.int32, device=dev)
    oi = torch.zeros((nq, k), dtype=torch.int64, device=dev)
    od = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    oc = torch.zeros(nq, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    idx.search_batch_device(dq.data_ptr(), nq, d, cand, ef, ci.data_ptr(), cd.data_ptr(), cc.data_ptr())
    idx.rescore_ptr(dq.data_ptr(), nq, d, ci.data_ptr(), cc.data_ptr(), cand, k, oi.data_ptr(), od.data_ptr(),
                    oc.data_ptr())
    torch.cuda.synchronize()
    pair = (oi.cpu().numpy().astype(np.uint64), od.cpu().numpy(), oc.cpu().numpy().astype(np.uint32))
    rref.same(pair, rref.rescore(orc, int(metric), q, x, ci.cpu().numpy().astype(np.uint64), cc.cpu().numpy(), k))
    oi2, od2, oc2 = torch.zeros_like(oi), torch.zeros_like(od), torch.zeros_like(oc)
    idx.search_refined_batch_ptr(dq.data_ptr(), nq, d, k, ef, cand, oi2.data_ptr(), od2.data_ptr(), oc2.data_ptr())
    assert torch.equal(oi, oi2) and torch.equal(od.view(torch.int32), od2.view(torch.int32)) and torch.equal(oc, oc2)
    ids, dist, cnt = idx.search_refined_batch(q, k, ef, cand)
    assert ids.tolist() == pair[0].tolist() and dist.tobytes() == pair[1].tobytes() and cnt.tolist() == pair[2].tolist()


# --------------------------------------------------------------- refined search
@functools.lru_cache(maxsize=None)
def rows_of(kind):
    if kind == "clustered":
        return ref.fixture()  # 2000 x 16 and 64 queries beside rows
    x = uniform_vectors(300, 50, 5).astype(np.float32)
    q = uniform_vectors(40, 50, 6).astype(np.float32)
    x.setflags(write=False)
    q.setflags(write=False)
    return x, q


def refined_case(orc, metric, kind, stored, placement="device"):
    """(index over fp8 / bf16 rows with the f32 originals as its refine table, x, q, the stored rows' images)"""
    x, q = rows_of(kind)
    csr = ref.knn_csr(orc, int(metric), x, tag=("refine", kind))
    idx = csr_index(csr, metric, x.shape[1])
    if stored == "fp8":
        codes, e = ia.quantize_fp8_e4m3(x)
        idx.set_embeddings_fp8(codes, e)
        images = ia.fp8_e4m3_to_f32(codes, e)
    else:
        idx.set_embeddings_bf16(ref.bf16_bits(x))
        images = ref.bf16_image(ref.bf16_bits(x))
    idx.set_refine_rows(x, placement=placement)
    return idx, x, q, images


def check_refined(orc, idx, metric, x, q, k, ef, cand):
    """the refined answer = the definition applied to what search_batch(q, cand, ef) returns on the same handle,
    with the inner search's counters; every distance has the bits of the ORIGINAL rows' distance"""
    cids, _, ccnt = idx.search_batch(q, cand, ef)
    inner = idx.last_stats()
    got = idx.search_refined_batch(q, k, ef, cand)
    st = idx.last_stats()
    for f in ("queries", "expansions", "edges", "evals", "pushes", "exact_path", "replayed"):
        assert st[f] == inner[f], f
    rref.same(got, rref.rescore(orc, int(metric), q, x, cids, ccnt, k))
    ids, dist, cnt = got
    for i in range(q.shape[0]):
        m = int(cnt[i])
        want = orc.batch_distance(int(metric), q[i], np.ascontiguousarray(x[ids[i, :m].astype(np.int64)]))
        assert dist[i, :m].view(np.uint32).tolist() == np.asarray(want, np.float32).view(np.uint32).tolist(), i
    return got


@pytest.mark.parametrize("stored", ["fp8", "bf16"])
@pytest.mark.parametrize("kind", ["clustered", "uniform"])
@pytest.mark.parametrize("metric", METRICS)
def test_refined_search_is_the_search_then_the_rescoring(orc, metric, kind, stored):
    idx, x, q, _ = refined_case(orc, metric, kind, stored, "host" if kind == "uniform" else "device")
    k, ef = 10, 64
    for cand in (10, 32, 64):
        ids, dist, cnt = check_refined(orc, idx, metric, x, q, k, ef, cand)
        assert (cnt == k).all()
    # recall@k against the exact f32 top-k is at least the plain search's: a true neighbour among the candidates
    # cannot rank below k under exact scores (rows without equal distances)
    pids, _, pcnt = idx.search_batch(q, k, ef)
    plain = ref.recall_at(orc, int(metric), q, x, pids, pcnt, k)
    refined = ref.recall_at(orc, int(metric), q, x, ids, cnt, k)
    print(f"recall@{k} {kind} {stored} {metric}: plain {plain:.4f} refined (candidates 64) {refined:.4f}")
    assert refined >= plain


def test_refined_search_with_entry_seeds(orc):
    metric = ia.DistanceMetric.Cosine
    x, q = rows_of("clustered")
    csr = ref.knn_csr(orc, int(metric), x, tag=("refine", "clustered"))
    idx = csr_index(csr, metric, x.shape[1])
    idx.set_embeddings_bf16(ref.bf16_bits(x))
    idx.set_refine_rows(x)
    ids0, _, _ = idx.search_refined_batch(q, 5, 16, 16)
    idx.select_entry_seeds(64)
    assert idx.refine_storage()["rows"] == x.shape[0]  # the seed setters keep the table
    ids1, _, _ = check_refined(orc, idx, metric, x, q, 5, 16, 16)  # the candidates are the seeded search's
    assert ids1.tolist() != ids0.tolist()


def test_small_graph_counts_below_k_and_scratch_reuse(orc):
    metric = ia.DistanceMetric.Euclidean
    x = uniform_vectors(5, 8, 3).astype(np.float32)
    g = ia.CsrGraph()
    for i in range(5):
        g.add_node([(i + 1) % 5, (i + 2) % 5], 0)
    g.entry_point = 0
    idx = ia.LeannIndex.from_csr(g, ia.LeannConfig(metric=metric), dimension=8).upload(0)
    idx.set_embeddings(x)
    idx.set_refine_rows(x, placement="host")
    q = uniform_vectors(3, 8, 4).astype(np.float32)
    ids, dist, cnt = idx.search_refined_batch(q, 7, 16, candidates=8)
    assert cnt.tolist() == [5, 5, 5]
    rref.same((ids, dist, cnt), rref.rescore(orc, int(metric), q, x, np.tile(np.arange(5, dtype=np.uint64), (3, 1)),
                                             [5, 5, 5], 7))
    assert (ids[:, 5:] == 0).all()
    # the first call of a shape may have had to allocate; the next one of the same shape reports none
    idx.search_refined_batch(q, 7, 16, candidates=8)
    assert idx.last_stats()["allocations"] == 0
    big = uniform_vectors(64, 8, 5).astype(np.float32)
    idx.search_refined_batch(big, 4, 32, candidates=5)
    assert idx.last_stats()["allocations"] > 0  # the scratch had to grow
    idx.search_refined_batch(big, 4, 32, candidates=5)
    assert idx.last_stats()["allocations"] == 0


def test_refusals_on_the_device(orc):
    metric = ia.DistanceMetric.Euclidean
    idx, x, q, _ = refined_case(orc, metric, "uniform", "bf16")
    n, d = x.shape

    def kind(call):
        with pytest.raises(ia.CoreError) as e:
            call()
        return e.value

    # the setter, after the residency check: row count (both named), d == 0, the dimension
    e = kind(lambda: idx.set_refine_rows(x[:-1]))
    assert e.kind == "InvalidArgument" and str(n - 1) in str(e) and str(n) in str(e)
    assert kind(lambda: idx.set_refine_rows(np.zeros((n, d + 1), np.float32))).kind == "DimensionMismatch"
    lib, h = ia._ffi.lib(), idx._h
    assert lib.isl_index_set_refine_rows(h, x.ctypes.data, n - 1, 0, 0, 0, 0) == 101  # the row count before d == 0
    assert lib.isl_index_set_refine_rows(h, x.ctypes.data, n, 0, 0, 0, 0) == 2  # EmptyCollection before the dimension
    assert idx.refine_storage()["rows"] == n  # refused calls leave the table alone
    # the searches, in the stated order
    assert kind(lambda: idx.search_refined_batch(q, 0, 16, 8)).kind == "InvalidArgument"
    assert kind(lambda: idx.search_refined_batch(q, 9, 16, 8)).kind == "InvalidArgument"
    assert kind(lambda: idx.search_refined_batch(q, 4, 16, 17)).kind == "InvalidArgument"
    assert kind(lambda: idx.search_refined_batch(q, 600, 512, 513)).kind == "InvalidArgument"  # k > candidates first
    assert kind(lambda: idx.search_refined_batch(q, 4, 600, 513)).kind == "Unsupported"
    e = kind(lambda: idx.search_refined_batch(np.zeros((2, d + 3), np.float32), 4, 16, 8))
    assert e.kind == "DimensionMismatch" and (e.expected, e.actual) == (d, d + 3)
    assert kind(lambda: idx.rescore(q, np.zeros((q.shape[0], 513), np.uint64), np.zeros(q.shape[0], np.uint32), 4)).kind \
        == "Unsupported"
    assert kind(lambda: idx.rescore(q, np.zeros((q.shape[0], 8), np.uint64), np.zeros(q.shape[0], np.uint32), 9)).kind \
        == "InvalidArgument"
    ids, dist, cnt = idx.search_refined_batch(np.zeros((0, d), np.float32), 4, 16, 8)
    assert ids.shape == (0, 4) and cnt.size == 0


# ------------------------------------------------------------------- lifecycle
def test_table_lifecycle(orc):
    metric = ia.DistanceMetric.Euclidean
    x = uniform_vectors(300, 24, 11).astype(np.float32)
    q = uniform_vectors(16, 24, 12).astype(np.float32)
    idx = ia.LeannIndex.build(x, ia.LeannConfig(m=8, m0=16, ef_construction=40, metric=metric), batch=16)
    idx.set_refine_rows(x, placement="host")
    st = idx.refine_storage()
    assert st == {"dtype": 0, "placement": "host", "rows": 300, "block_bytes": (300 * 24 + 256) * 4}
    before = idx.to_bytes()
    # convert_rows, set_embeddings_fp8 and reserve keep it (the intended flow: build, set, narrow)
    idx.convert_rows("fp8")
    assert idx.row_storage()["dtype"] == 2 and idx.refine_storage() == st
    a = check_refined(orc, idx, metric, x, q, 5, 32, 16)
    codes, e = ia.quantize_fp8_e4m3(x)
    idx.set_embeddings_fp8(codes, e)
    assert idx.refine_storage() == st
    b = idx.search_refined_batch(q, 5, 32, 16)
    assert a[0].tolist() == b[0].tolist() and a[1].tobytes() == b[1].tobytes()
    idx.convert_rows("f32")
    idx.reserve(400)
    assert idx.refine_storage() == st
    assert idx.to_bytes() == before  # the table is not part of the serialised index
    # a second table replaces the first, in the other placement and type
    idx.set_refine_rows(ref.bf16_bits(x), placement="device")
    assert idx.refine_storage() == {"dtype": 1, "placement": "device", "rows": 300, "block_bytes": (300 * 24 + 512) * 2}
    check_refined(orc, idx, metric, ref.bf16_image(ref.bf16_bits(x)), q, 5, 32, 16)
    # insert and remove change the node count: the table goes

    def gone():
        assert idx.refine_storage()["rows"] == 0
        with pytest.raises(ia.CoreError) as err:
            idx.search_refined_batch(q, 5, 32, 16)
        assert err.value.kind == "InvalidArgument"

    more = uniform_vectors(10, 24, 13).astype(np.float32)
    idx.insert(more, batch=10)
    gone()
    allx = np.concatenate([x, more])
    idx.set_refine_rows(allx)
    assert idx.refine_storage()["rows"] == 310
    idx.remove([3, 4])
    gone()
    idx.set_refine_rows(np.delete(allx, [3, 4], axis=0), placement="host")
    check_refined(orc, idx, metric, np.delete(allx, [3, 4], axis=0), q, 5, 32, 16)
    idx.set_refine_rows(None)  # n == 0 drops it
    gone()


def test_four_threads_agree_with_one(orc):
    metric = ia.DistanceMetric.Cosine
    idx, x, q, _ = refined_case(orc, metric, "clustered", "fp8", "host")
    want = [idx.search_refined_batch(q[t * 16:(t + 1) * 16], 10, 64, 32 + 8 * t) for t in range(4)]
    got, errors = [None] * 4, []

    def work(t):
        try:
            for _ in range(3):
                got[t] = idx.search_refined_batch(q[t * 16:(t + 1) * 16], 10, 64, 32 + 8 * t)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for t in range(4):
        assert got[t][0].tolist() == want[t][0].tolist() and got[t][1].tobytes() == want[t][1].tobytes()
        assert got[t][2].tolist() == want[t][2].tolist()
