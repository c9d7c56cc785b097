"""isl_hnsw_build on the device.  Reference rule, one node per step: the bytes of the built graph equal
the bincode image of the oracle's graph (every list, levels, entry point, max level) and it searches like
the oracle's.  Diverse rule: every list equals the Python definition (tests/_hnsw_build_ref.py).  Batched:
structural invariants, and for the diverse rule reachability and recall.  Every comparison is exact."""
import ctypes as C
import struct

import numpy as np
import pytest

import islands_amd as ia
import _hnsw_build_ref as ref
from islands_amd import _ffi
from _data import clustered_vectors, random_levels, uniform_vectors
from test_gpu_hnsw import assert_same
from test_hnsw_bytes import hnsw_to_bincode

pytestmark = pytest.mark.gpu

METRICS = [ia.DistanceMetric.Cosine, ia.DistanceMetric.Euclidean, ia.DistanceMetric.DotProduct,
           ia.DistanceMetric.Manhattan]


def check_reference(orc, v, lv, m, m0, efc, metric, queries=None, k=10, ef=50):
    """build on the device == the oracle's inserts, byte for byte; then both answer alike"""
    n = v.shape[0]
    h = orc.Hnsw(m=m, m0=m0, ef_construction=efc, metric=int(metric))
    for i in range(n):
        st, idx = h.insert(v[i], int(lv[i]))
        assert st == 0 and idx == i
    g = ia.HnswGraph.build(v, m=m, m0=m0, ef_construction=efc, metric=metric, ml=1.0 / np.log(m), levels=lv)
    assert len(g) == n and g.entry_point == h.entry_point and g.max_level == h.max_level
    assert g.levels().tolist() == [int(x) for x in lv]
    for i in range(n):  # (first, for a readable failure; the bytes below say the same)
        for L in range(int(lv[i]) + 1):
            assert g.neighbors(i, L) == list(h.neighbors(i, L) or []), (i, L)
        assert g.neighbors(i, int(lv[i]) + 1) is None
    layers = [[(h.neighbors(i, L) or []) for i in range(n)] for L in range(h.max_level + 1)]
    want = hnsw_to_bincode(v, layers, [int(x) for x in lv], h.entry_point, h.max_level, m=m, m0=m0,
                           ef_construction=efc, metric=int(metric))
    assert g.to_bytes() == want
    q = uniform_vectors(24, v.shape[1], 99) if queries is None else queries
    assert_same(h, g, q, k, ef)
    assert_same(h, g, v[:8], min(3, n), 3)
    return h, g


@pytest.mark.parametrize("metric", METRICS)
def test_reference_rule_is_the_oracle(orc, metric):
    h, g = check_reference(orc, uniform_vectors(600, 24, 11), random_levels(600, 16, 14), 16, 32, 200, metric)
    assert h.max_level >= 1


def test_reference_rule_d768(orc):
    check_reference(orc, uniform_vectors(400, 768, 5), random_levels(400, 8, 8), 8, 16, 40, 0)


def test_reference_rule_ties(orc):
    base = uniform_vectors(60, 8, 3)
    v = np.concatenate([base, base, base[:30], base[:60]]).astype(np.float32)
    h, g = check_reference(orc, v, random_levels(v.shape[0], 6, 24), 6, 12, 30, ia.DistanceMetric.Euclidean,
                           queries=base[:20], k=10, ef=40)
    g.search_batch(base[:20], 10, 40)
    assert g.last_stats()["exact_path"] > 0  # equal distances: the heap-exact kernel decides


@pytest.mark.parametrize("shape", [(12, 24, 100, 0, "fast"), (32, 64, 400, 0, "accurate"), (64, 128, 256, 1, "widest")])
def test_reference_rule_presets(orc, shape):
    # HnswConfig::fast() is 12 / 24 / 100 (hnsw.rs:52-59), accurate() 32 / 64 / 400 (a list under re-selection
    # holds 65 ids); widest: 129 ids, the limit
    m, m0, efc, metric, _ = shape
    check_reference(orc, uniform_vectors(400, 12, 33), random_levels(400, m, 5), m, m0, efc, metric)


def test_reference_rule_rising_top_layer(orc):
    lv = np.zeros(300, np.uint64)
    lv[5], lv[40], lv[100], lv[101], lv[200] = 3, 1, 5, 5, 2
    h, g = check_reference(orc, uniform_vectors(300, 16, 9), lv, 8, 16, 64, 0)
    assert g.entry_point == 100 and g.max_level == 5
    assert g.neighbors(101, 5) == [100, 5] and g.level(5) == 3  # a list may name a node that lacks the layer


@pytest.mark.parametrize("n", [1, 2])
def test_reference_rule_tiny(orc, n):
    check_reference(orc, uniform_vectors(n, 8, 2), np.asarray([1, 0][:n], np.uint64), 4, 8, 16, 1,
                    queries=uniform_vectors(3, 8, 4), k=2, ef=4)


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("alpha", [1.0, 1.2])
@pytest.mark.parametrize("rows", [("uniform", 0), ("clustered", 1)])
def test_diverse_rule_is_the_definition(orc, rows, alpha, keep):
    kind, metric = rows
    v = uniform_vectors(500, 24, 7) if kind == "uniform" else clustered_vectors(500, 16, 7)
    lv = random_levels(500, 8, 4)
    want = ref.build(orc, v, lv, 8, 16, 64, metric, "diverse", alpha, keep)
    g = ia.HnswGraph.build(v, m=8, m0=16, ef_construction=64, metric=metric, levels=lv, select="diverse",
                           alpha=alpha, keep_pruned=keep)
    assert g.entry_point == want.entry and g.max_level == want.max_level and want.max_level >= 1
    for i in range(500):
        for L in range(int(lv[i]) + 1):
            assert g.neighbors(i, L) == list(want.conn[i][L]), (i, L)


def list_counts(blob):
    """connections.len() of every node, read out of the bincode image (layout: hnsw.hip)"""
    n = struct.unpack_from("<Q", blob, 44)[0]
    pos, out = 52, []
    for _ in range(n):
        _, _, vlen = struct.unpack_from("<QQQ", blob, pos)
        pos += 24 + 4 * vlen
        nl = struct.unpack_from("<Q", blob, pos)[0]
        pos += 8
        for _ in range(nl):
            pos += 8 + 8 * struct.unpack_from("<Q", blob, pos)[0]
        out.append((nl, struct.unpack_from("<Q", blob, pos)[0]))
        pos += 8
    return out


def raw_neighbors(g, node, layer):
    """isl_hnsw_get_neighbors itself: (has_layer, count)"""
    out = np.zeros(129, dtype=np.uint64)
    cnt, has = C.c_uint64(), C.c_int32(-1)
    st = _ffi.lib().isl_hnsw_get_neighbors(g._h, node, layer, out.ctypes.data_as(C.c_void_p), out.size, C.byref(cnt),
                                           C.byref(has))
    assert st == 0
    return has.value, cnt.value


def structure(g, n, lv, m, m0):
    # a node's list count is its level + 1: in the bytes and in what the library answers above the level
    assert list_counts(g.to_bytes()) == [(int(x) + 1, int(x)) for x in lv]
    for i in range(0, n, 7):
        assert raw_neighbors(g, i, int(lv[i]) + 1) == (0, 0) and raw_neighbors(g, i, int(lv[i]))[0] == 1
    layer0 = []
    for i in range(n):
        for L in range(int(lv[i]) + 1):
            row = g.neighbors(i, L)
            assert row is not None and len(row) <= (m0 if L == 0 else m), (i, L)
            assert i not in row and len(set(row)) == len(row) and all(0 <= x < n for x in row), (i, L, row)
            if L == 0:
                layer0.append(row)
        assert g.neighbors(i, int(lv[i]) + 1) is None
    return layer0


@pytest.mark.parametrize("kind", ["uniform", "clustered"])
@pytest.mark.parametrize("rule", ["reference", "diverse"])
def test_batched_build(kind, rule):
    n, d, m, m0, efc = 3000, 16, 8, 16, 64
    v = uniform_vectors(n, d, 21) if kind == "uniform" else clustered_vectors(n, d, 21)
    metric = 0 if kind == "uniform" else 1
    lv = random_levels(n, m, 3)
    g = ia.HnswGraph.build(v, m=m, m0=m0, ef_construction=efc, metric=metric, levels=lv, select=rule, batch=256)
    assert len(g) == n and g.levels().tolist() == [int(x) for x in lv]
    # entry point and max level are the sequential ones: the first node of the highest level
    top = int(lv.max())
    assert g.max_level == top and g.entry_point == int(np.argmax(lv == top))
    layer0 = structure(g, n, lv, m, m0)
    if rule == "diverse":
        lost = ref.no_inbound(layer0)
        probes = list(range(0, n, 30))
        got = g.search_batch(v[probes], 1, 64)
        hits = sum(1 for i, (ids, _) in zip(probes, got) if ids.tolist()[:1] == [i])
        print(f"{kind}: nodes without an inbound layer-0 edge {lost} of {n}; self-query recall@1 {hits}/{len(probes)}")
        assert lost <= 0.01 * n
        assert hits >= 0.95 * len(probes)


def test_round_trip_and_device_rows(orc):
    torch = pytest.importorskip("torch")
    v = clustered_vectors(800, 32, 3)
    lv = random_levels(800, 8, 6)
    kw = dict(m=8, m0=16, ef_construction=64, metric=ia.DistanceMetric.Euclidean, levels=lv, select="diverse")
    g = ia.HnswGraph.build(v, **kw)
    blob = g.to_bytes()
    g2 = ia.HnswGraph.from_bytes(blob)
    assert g2.to_bytes() == blob and g2.entry_point == g.entry_point and g2.max_level == g.max_level
    q = uniform_vectors(30, 32, 8)
    for (a, da), (b, db) in zip(g.search_batch(q, 10, 50), g2.search_batch(q, 10, 50)):
        assert a.tolist() == b.tolist() and da.view(np.uint32).tolist() == db.view(np.uint32).tolist()
    assert g.get_vector(17).view(np.uint32).tolist() == v[17].view(np.uint32).tolist()
    assert g2.get_vector(799).view(np.uint32).tolist() == v[799].view(np.uint32).tolist()
    assert g.neighbors(17, 0) == g2.neighbors(17, 0)
    t = torch.from_numpy(v).to("cuda:0")
    g3 = ia.HnswGraph.build(t, **kw)
    assert g3.to_bytes() == blob
    # levels drawn from the seed: the same graph as with those levels handed over
    kw.pop("levels")
    a = ia.HnswGraph.build(v, level_seed=5, **kw)
    b = ia.HnswGraph.build(v, levels=ia.HnswGraph.random_levels(800, seed=5), **kw)
    assert a.to_bytes() == b.to_bytes() and a.max_level >= 1
