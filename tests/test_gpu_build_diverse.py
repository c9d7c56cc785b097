"""GPU: the diverse (occlusion) selection rule of the device builder (isl_index_build_ex with
ISL_SELECT_DIVERSE, isl_select_neighbors) against its definition in tests/_diverse_ref.py: the
primitive id for id, the sequential build byte for byte, and the recall it exists for."""
import ctypes as C
import itertools

import numpy as np
import pytest

import islands_amd as ia
from islands_amd import _ffi

import _diverse_ref as ref
from _data import clustered_vectors, random_levels, uniform_vectors

pytestmark = pytest.mark.gpu

METRICS = [ia.DistanceMetric.Cosine, ia.DistanceMetric.Euclidean, ia.DistanceMetric.DotProduct,
           ia.DistanceMetric.Manhattan]


def rows_on_device(v, metric):
    """An index without edges that carries the rows: what isl_select_neighbors needs."""
    n = v.shape[0]
    g = ia.CsrGraph(node_offsets=np.zeros(n + 1, np.uint64), levels=np.zeros(n, np.uint64), entry_point=0,
                    num_nodes=n, degree_counts=np.zeros(n, np.uint64))
    return ia.LeannIndex.from_csr(g, ia.LeannConfig(metric=metric), dimension=v.shape[1]).upload(0)


def with_rows(idx, v):
    return idx.set_embeddings(v)


# ---------------------------------------------------------------- 4. the primitive, bit for bit
@pytest.mark.parametrize("d", [3, 24, 768])
@pytest.mark.parametrize("metric", METRICS)
def test_select_neighbors_equals_the_definition(orc, metric, d):
    n = 640
    v = uniform_vectors(n, d, 40 + d) if d == 3 else clustered_vectors(n, d, 40 + d, per_cluster=80)
    idx = with_rows(rows_on_device(v, metric), v)
    rng = np.random.default_rng(1000 + d)
    checked = 0
    for count in (1, 17, 61, 129, 512):
        bases = rng.choice(n, size=2, replace=False)
        cand = np.stack([rng.choice(np.setdiff1d(np.arange(n), [b]), size=count, replace=False) for b in bases])
        for cap, alpha, keep in itertools.product((1, 16, 60, 128), (1.0, 1.2), (False, True)):
            ids, cnt = idx.select_neighbors(bases, cand, cap, alpha=alpha, keep_pruned=keep)
            for r, b in enumerate(bases):
                want = ref.select(orc, v, metric, b, cand[r], cap, alpha, keep)
                assert ids[r, :cnt[r]].tolist() == want, (int(metric), d, count, cap, alpha, keep, int(b))
                checked += 1
    assert checked == 5 * 16 * 2


@pytest.mark.parametrize("metric", METRICS)
def test_select_neighbors_with_duplicated_rows(orc, metric):
    """Equal rows: zero and equal distances everywhere; the order among ties is the stable sort's."""
    base = uniform_vectors(40, 24, 9)
    v = np.concatenate([base, base, base[:20]]).astype(np.float32)
    idx = with_rows(rows_on_device(v, metric), v)
    rng = np.random.default_rng(5)
    bases = np.array([3, 47, 99], dtype=np.uint64)
    cand = np.stack([rng.permutation(100)[:90] for _ in bases])  # may hold the base and its twins
    for cap, alpha, keep in itertools.product((16, 128), (1.0, 1.2), (False, True)):
        ids, cnt = idx.select_neighbors(bases, cand, cap, alpha=alpha, keep_pruned=keep)
        for r, b in enumerate(bases):
            assert ids[r, :cnt[r]].tolist() == ref.select(orc, v, metric, b, cand[r], cap, alpha, keep)
    # a repeated id among the candidates is a second entry, occluded by the first
    twice = np.array([[7, 12, 7, 30, 12, 55]], dtype=np.uint64)
    for keep in (False, True):
        ids, cnt = idx.select_neighbors([1], twice, 6, keep_pruned=keep)
        assert ids[0, :cnt[0]].tolist() == ref.select(orc, v, metric, 1, twice[0], 6, 1.0, keep)


def test_select_neighbors_zero_vector_under_cosine(orc):
    v = clustered_vectors(200, 24, 3)
    v[17] = 0.0  # cosine distance 1 to everything (distance.rs:82-85)
    v[90] = 0.0
    idx = with_rows(rows_on_device(v, ia.DistanceMetric.Cosine), v)
    rng = np.random.default_rng(2)
    cand = np.stack([np.concatenate([[17, 90], rng.choice(np.arange(100, 200), 60, replace=False)]),
                     np.concatenate([[90, 5], rng.choice(np.arange(100, 200), 60, replace=False)])])
    bases = [4, 17]  # a zero vector among the candidates, and as the base
    for cap, keep in itertools.product((16, 60), (False, True)):
        ids, cnt = idx.select_neighbors(bases, cand, cap, keep_pruned=keep)
        for r, b in enumerate(bases):
            assert ids[r, :cnt[r]].tolist() == ref.select(orc, v, 0, b, cand[r], cap, 1.0, keep)


def test_select_neighbors_errors():
    v = uniform_vectors(50, 8, 1)
    idx = with_rows(rows_on_device(v, ia.DistanceMetric.Cosine), v)
    with pytest.raises(ia.CoreError) as ex:
        idx.select_neighbors([3], [[1, 2, 50]], 2)
    assert ex.value.kind == "NodeNotFound" and ex.value.node == 50
    with pytest.raises(ia.CoreError) as ex:
        idx.select_neighbors([77], [[1, 2]], 2)
    assert ex.value.kind == "NodeNotFound" and ex.value.node == 77
    bf = rows_on_device(v, ia.DistanceMetric.Cosine).set_embeddings_bf16((v.view(np.uint32) >> 16).astype(np.uint16))
    with pytest.raises(ia.CoreError) as ex:
        bf.select_neighbors([3], [[1, 2]], 2)
    assert ex.value.kind == "Unsupported"


# ---------------------------------------------------------------- 5. the sequential build, bytes
def definition_bytes(orc, v, cfg, levels=None, alpha=1.0, keep_pruned=True):
    csr = ref.build(orc, v, cfg.m0, cfg.ef_construction, int(cfg.metric), alpha, keep_pruned, levels)
    g = ia.CsrGraph(node_offsets=csr.node_offsets, neighbors=csr.neighbors, levels=csr.levels,
                    entry_point=csr.entry_point, max_level=csr.max_level, num_nodes=csr.num_nodes,
                    degree_counts=csr.degree_counts)
    return ia.LeannIndex.from_csr(g, cfg, dimension=v.shape[1]).to_bytes(), csr


@pytest.mark.parametrize("metric", METRICS)
def test_sequential_diverse_build_is_the_definition(orc, metric):
    n, d = 500, 24
    v = clustered_vectors(n, d, 7)
    cfg = ia.LeannConfig(m=8, m0=16, ef_construction=40, metric=metric)
    levels = random_levels(n, 8, 3)
    want, _ = definition_bytes(orc, v, cfg, levels)
    idx = ia.LeannIndex.build(v, cfg, levels=levels, batch=1, select="diverse")
    assert idx.to_bytes() == want


@pytest.mark.parametrize("keep_pruned", [True, False])
def test_sequential_diverse_build_uniform_rows(orc, keep_pruned):
    n, d = 700, 16
    v = uniform_vectors(n, d, 11)
    cfg = ia.LeannConfig(m=6, m0=12, ef_construction=48)
    want, csr = definition_bytes(orc, v, cfg, keep_pruned=keep_pruned)
    idx = ia.LeannIndex.build(v, cfg, batch=1, select="diverse", keep_pruned=keep_pruned)
    assert idx.to_bytes() == want
    degs = np.diff(csr.node_offsets.astype(np.int64))
    print(f"keep_pruned={keep_pruned}: mean degree {degs.mean():.2f}, min {degs[1:].min()}")
    if not keep_pruned:
        assert degs.mean() < 12  # the case prunes: short rows stay short
    # the finished index is an ordinary one: it answers like the oracle over the same graph
    q = uniform_vectors(12, d, 12)
    ids, dist, cnt = idx.search_batch(q, 5, 30)
    for i in range(12):
        r = orc.leann_search(csr, v, q[i], 5, 30)
        assert ids[i, :cnt[i]].tolist() == r.ids.tolist()
    # and so are its bytes
    assert ia.LeannIndex.from_bytes(want).to_bytes() == want


def test_sequential_diverse_build_paper_default(orc):
    v = uniform_vectors(210, 32, 5)
    cfg = ia.LeannConfig.paper_default()  # m0 = 60, ef_construction = 128
    want, csr = definition_bytes(orc, v, cfg)
    idx = ia.LeannIndex.build(v, cfg, batch=1, select="diverse")
    assert idx.to_bytes() == want
    assert max(len(idx.get_neighbors(i)) for i in range(210)) == 60  # rows did overflow


def test_sequential_diverse_build_wide_rows(orc):
    n, d = 420, 12
    v = uniform_vectors(n, d, 127)
    cfg = ia.LeannConfig.accurate()
    cfg.m, cfg.m0, cfg.ef_construction = 48, 96, 400
    want, _ = definition_bytes(orc, v, cfg)
    idx = ia.LeannIndex.build(v, cfg, batch=1, select="diverse")
    assert idx.to_bytes() == want
    assert max(len(idx.get_neighbors(i)) for i in range(n)) > 64  # the case is what it claims to be


# ---------------------------------------------------------------- 6. the reference rule did not move
def test_default_options_are_the_reference_build(orc):
    n, d = 500, 24
    v = clustered_vectors(n, d, 7)
    cfg = ia.LeannConfig(m=8, m0=16, ef_construction=40)
    levels = random_levels(n, 8, 3)
    csr = orc.leann_build(v, m=8, m0=16, ef_construction=40, metric=0, high_degree_pruning=True,
                          hub_percentile=cfg.hub_percentile, levels=levels)
    g = ia.CsrGraph(node_offsets=csr.node_offsets, neighbors=csr.neighbors, levels=csr.levels,
                    entry_point=csr.entry_point, max_level=csr.max_level, num_nodes=csr.num_nodes,
                    degree_counts=csr.degree_counts)
    want = ia.LeannIndex.from_csr(g, cfg, dimension=d).to_bytes()
    l, c = _ffi.lib(), cfg._to_c()
    lv = np.ascontiguousarray(levels, dtype=np.uint64)
    vp, lp = v.ctypes.data_as(C.c_void_p), lv.ctypes.data_as(C.c_void_p)
    h_old, h_new = C.c_void_p(), C.c_void_p()
    assert l.isl_index_build(C.byref(c), vp, n, d, lp, 1, 0, 0, C.byref(h_old)) == 0
    o = _ffi.BuildOptionsC()
    l.isl_build_options_default(C.byref(o))
    assert l.isl_index_build_ex(C.byref(c), C.byref(o), vp, n, d, lp, 0, 0, C.byref(h_new)) == 0
    old, new = ia.LeannIndex(_handle=h_old), ia.LeannIndex(_handle=h_new)
    assert old.to_bytes() == want and new.to_bytes() == want
    h_null = C.c_void_p()
    assert l.isl_index_build_ex(C.byref(c), None, vp, n, d, lp, 0, 0, C.byref(h_null)) == 0
    assert ia.LeannIndex(_handle=h_null).to_bytes() == want
    assert ia.LeannIndex.build(v, cfg, levels=levels, batch=1, select="reference").to_bytes() == want


# ---------------------------------------------------------------- 7. what it is for
def recall_at_10(idx, q, truth, ef=128):
    ids, dist, cnt = idx.search_batch(q, 10, ef)
    hits = sum(len(set(ids[i, :cnt[i]].tolist()) & set(truth[i].tolist())) for i in range(q.shape[0]))
    return hits / (10.0 * q.shape[0]), idx.last_stats()["evals"] / q.shape[0]


def test_diverse_rule_rescues_clustered_rows(orc):
    n, d = 4000, 16
    v = clustered_vectors(n, d, 21)
    rng = np.random.default_rng(1)
    q = (v[rng.integers(0, n, 200)] + 0.05 * rng.standard_normal((200, d))).astype(np.float32)
    vn = v.astype(np.float64) / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)
    qn = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)
    truth = np.argsort(1.0 - qn @ vn.T, axis=1, kind="stable")[:, :10]
    cfg = ia.LeannConfig(m=8, m0=16, ef_construction=64)

    csr = orc.leann_build(v, m=8, m0=16, ef_construction=64)
    g = ia.CsrGraph(node_offsets=csr.node_offsets, neighbors=csr.neighbors, levels=csr.levels,
                    entry_point=csr.entry_point, max_level=csr.max_level, num_nodes=csr.num_nodes,
                    degree_counts=csr.degree_counts)
    before = ia.LeannIndex.from_csr(g, cfg, dimension=d).upload(0).set_embeddings(v)
    r_ref, e_ref = recall_at_10(before, q, truth)

    seq = ia.LeannIndex.build(v, cfg, batch=1, select="diverse")
    r_seq, e_seq = recall_at_10(seq, q, truth)
    bat = ia.LeannIndex.build(v, cfg, batch=256, select="diverse")
    r_bat, e_bat = recall_at_10(bat, q, truth)
    for name, idx in (("batch=1", seq), ("batch=256", bat)):
        degs = np.array([len(idx.get_neighbors(i)) for i in range(n)])
        print(f"diverse {name}: mean degree {degs.mean():.2f}, min degree (nodes 1..) {degs[1:].min()}")
    print(f"recall@10 ef 128: reference {r_ref:.4f} ({e_ref:.0f} evals/query), diverse batch=1 {r_seq:.4f} "
          f"({e_seq:.0f}), diverse batch=256 {r_bat:.4f} ({e_bat:.0f})")
    assert r_ref <= 0.05   # the input is the one the reference rule fails on
    assert r_seq >= 0.95
    assert r_bat >= r_seq - 0.02


# ---------------------------------------------------------------- 8. the batched graph
@pytest.mark.parametrize("keep_pruned", [True, False])
def test_batched_diverse_build_keeps_the_invariants(keep_pruned):
    n, d = 3000, 16
    v = uniform_vectors(n, d, 21)
    cfg = ia.LeannConfig(m=8, m0=16, ef_construction=64)
    idx = ia.LeannIndex.build(v, cfg, batch=256, select="diverse", keep_pruned=keep_pruned)
    assert len(idx) == n and idx.dimension() == d and idx.entry_point == 0
    rows = [idx.get_neighbors(i).tolist() for i in range(n)]
    degs = np.array([len(r) for r in rows])
    print(f"keep_pruned={keep_pruned}: mean degree {degs.mean():.2f}, min degree (nodes 1..) {degs[1:].min()}")
    assert degs.max() <= 16 and degs[1:].min() >= 1
    for i, r in enumerate(rows):
        assert len(set(r)) == len(r) and i not in r and all(x < n for x in r)
    ids, dist, cnt = idx.search_batch(v[::30], 1, 64)  # reported, not asserted: the issue sets no bound here
    print(f"self-query recall@1 at ef 64: {(ids[:, 0] == np.arange(0, n, 30)).mean():.3f}")
