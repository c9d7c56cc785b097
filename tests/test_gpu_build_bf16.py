"""GPU: LeannIndex::build from bf16 rows on the device (isl_index_build_rows with ISL_DTYPE_BF16).  A bf16
value is exactly representable in f32 and every distance of the builder goes through the strictly ordered f32
chain, so the index built from bf16 rows is the one the reference builds from the widened rows, byte for byte:
the oracle's restatement of the reference builder (reference rule) and tests/_diverse_ref.py (diverse rule)
over widen(bits) give the expected bytes."""
import ctypes as C
import os

import numpy as np
import pytest

import islands_amd as ia
from islands_amd import _ffi

import _diverse_ref as ref
from _data import clustered_vectors, random_levels, uniform_vectors

pytestmark = pytest.mark.gpu

METRICS = [ia.DistanceMetric.Cosine, ia.DistanceMetric.Euclidean, ia.DistanceMetric.DotProduct,
           ia.DistanceMetric.Manhattan]


def to_bf16_bits(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def widen(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def csr_bytes(csr, cfg, d):
    g = ia.CsrGraph(node_offsets=csr.node_offsets, neighbors=csr.neighbors, levels=csr.levels,
                    entry_point=csr.entry_point, max_level=csr.max_level, num_nodes=csr.num_nodes,
                    degree_counts=csr.degree_counts)
    return ia.LeannIndex.from_csr(g, cfg, dimension=d).to_bytes()


def reference_bytes(orc, v, cfg, levels):
    csr = orc.leann_build(v, m=cfg.m, m0=cfg.m0, ef_construction=cfg.ef_construction,
                          metric=int(cfg.metric), high_degree_pruning=cfg.high_degree_pruning,
                          hub_percentile=cfg.hub_percentile, levels=levels)
    return csr_bytes(csr, cfg, v.shape[1]), csr


def definition_bytes(orc, v, cfg, levels=None, alpha=1.0, keep_pruned=True):
    csr = ref.build(orc, v, cfg.m0, cfg.ef_construction, int(cfg.metric), alpha, keep_pruned, levels)
    return csr_bytes(csr, cfg, v.shape[1]), csr


def same_answers(orc, idx, csr, rows, q, k, ef, metric=0):
    ids, dist, cnt = idx.search_batch(q, k, ef)
    for i in range(q.shape[0]):
        r = orc.leann_search(csr, rows, q[i], k, ef, metric=int(metric))
        m = int(cnt[i])
        assert ids[i, :m].tolist() == r.ids.tolist(), i
        assert dist[i, :m].view(np.uint32).tolist() == r.dist.view(np.uint32).tolist(), i


# ---------------------------------------------------------------- 1. reference rule, four metrics
@pytest.mark.parametrize("metric", METRICS)
def test_reference_rule_is_the_reference_graph_of_the_widened_rows(orc, metric):
    n, d = 500, 24
    bits = to_bf16_bits(clustered_vectors(n, d, 7))
    cfg = ia.LeannConfig(m=8, m0=16, ef_construction=40, metric=metric)
    levels = random_levels(n, 8, 3)
    want, _ = reference_bytes(orc, widen(bits), cfg, levels)
    assert ia.LeannIndex.build_bf16(bits, cfg, levels=levels, batch=1).to_bytes() == want
    # and the f32 builder over the widened rows makes the same index
    assert ia.LeannIndex.build(widen(bits), cfg, levels=levels, batch=1).to_bytes() == want


# ---------------------------------------------------------------- 2. dimensions around the loads and steps
@pytest.mark.parametrize("metric", [ia.DistanceMetric.Cosine, ia.DistanceMetric.Euclidean])
@pytest.mark.parametrize("n,d", [(200, 3), (200, 100), (200, 768), (160, 4096)])
def test_dimensions(orc, metric, n, d):
    """d 3: one guarded load; d 100: a multiple of 4 but not of 8, the stride is padded; d 768; d 4096:
    BASELINE config 5's row."""
    bits = to_bf16_bits(uniform_vectors(n, d, 50 + d) if d == 3 else clustered_vectors(n, d, 50 + d))
    cfg = ia.LeannConfig(m=8, m0=16, ef_construction=40, metric=metric)
    want, _ = reference_bytes(orc, widen(bits), cfg, None)
    assert ia.LeannIndex.build_bf16(bits, cfg, batch=1).to_bytes() == want


# ---------------------------------------------------------------- 3. hub rule, and the index answers
@pytest.mark.parametrize("hub_percentile,high_degree", [(0.25, True), (0.02, False)])
def test_hub_rule_and_searches(orc, hub_percentile, high_degree):
    n, d = 700, 16
    bits = to_bf16_bits(uniform_vectors(n, d, 11))
    rows = widen(bits)
    cfg = ia.LeannConfig(m=6, m0=12, ef_construction=48, hub_percentile=hub_percentile,
                         high_degree_pruning=high_degree)
    want, csr = reference_bytes(orc, rows, cfg, None)
    idx = ia.LeannIndex.build_bf16(bits, cfg, batch=1)
    assert idx.to_bytes() == want
    # the rows it keeps are the bf16 rows: it answers like the oracle over its graph and the widened rows
    same_answers(orc, idx, csr, rows, uniform_vectors(12, d, 12), 5, 30)                       # f32 queries
    same_answers(orc, idx, csr, rows, widen(to_bf16_bits(uniform_vectors(12, d, 13))), 5, 30)  # bf16-valued ones


# ---------------------------------------------------------------- 4. ties
def test_paper_default_config_and_duplicates(orc):
    """Equal rows tie everywhere: the heap-exact kernel decides construction searches over bf16 rows."""
    base = to_bf16_bits(uniform_vectors(150, 32, 5))
    bits = np.concatenate([base, base[:60]])
    cfg = ia.LeannConfig.paper_default()  # m0 = 60, ef_construction = 128
    want, _ = reference_bytes(orc, widen(bits), cfg, None)
    assert ia.LeannIndex.build_bf16(bits, cfg, batch=1).to_bytes() == want


# ---------------------------------------------------------------- 5. rows past 64 ids
@pytest.mark.parametrize("m,m0,efc", [(48, 96, 400), (64, 128, 256), (33, 65, 100)])
def test_wide_rows(orc, m, m0, efc):
    """The wide bf16 search instantiation, and a re-sort over up to 129 entries in three slices."""
    n, d = 420, 12
    bits = to_bf16_bits(uniform_vectors(n, d, 31 + m0))
    cfg = ia.LeannConfig.accurate()
    cfg.m, cfg.m0, cfg.ef_construction = m, m0, efc
    levels = random_levels(n, m, 5)
    want, _ = reference_bytes(orc, widen(bits), cfg, levels)
    idx = ia.LeannIndex.build_bf16(bits, cfg, levels=levels, batch=1)
    assert idx.to_bytes() == want
    assert max(len(idx.get_neighbors(i)) for i in range(n)) > 64  # the case is what it claims to be


# ---------------------------------------------------------------- 6. diverse rule
@pytest.mark.parametrize("metric", METRICS)
def test_diverse_rule_is_the_definition_on_the_widened_rows(orc, metric):
    n, d = 300, 24
    bits = to_bf16_bits(clustered_vectors(n, d, 7))
    cfg = ia.LeannConfig(m=8, m0=16, ef_construction=40, metric=metric)
    levels = random_levels(n, 8, 3)
    want, _ = definition_bytes(orc, widen(bits), cfg, levels)
    assert ia.LeannIndex.build_bf16(bits, cfg, levels=levels, batch=1, select="diverse").to_bytes() == want
    assert ia.LeannIndex.build(widen(bits), cfg, levels=levels, batch=1, select="diverse").to_bytes() == want


@pytest.mark.parametrize("case", ["alpha", "no_fill", "wide", "d768", "long_lists"])
def test_diverse_rule_variants(orc, case):
    alpha, keep = 1.0, True
    if case == "alpha":
        n, d, m, m0, efc, alpha = 300, 24, 8, 16, 40, 1.2
    elif case == "no_fill":
        n, d, m, m0, efc, keep = 300, 24, 8, 16, 40, False
    elif case == "wide":
        n, d, m, m0, efc = 420, 12, 48, 96, 400
    elif case == "d768":
        n, d, m, m0, efc = 200, 768, 8, 16, 40
    else:  # candidate lists longer than 64: several passes of 64 per kept candidate
        n, d, m, m0, efc = 300, 24, 8, 16, 200
    v = uniform_vectors(n, d, 127) if case == "wide" else clustered_vectors(n, d, 9)
    bits = to_bf16_bits(v)
    cfg = ia.LeannConfig(m=m, m0=m0, ef_construction=efc)
    want, _ = definition_bytes(orc, widen(bits), cfg, alpha=alpha, keep_pruned=keep)
    idx = ia.LeannIndex.build_bf16(bits, cfg, batch=1, select="diverse", alpha=alpha, keep_pruned=keep)
    assert idx.to_bytes() == want
    if case == "wide":
        assert max(len(idx.get_neighbors(i)) for i in range(n)) > 64


# ---------------------------------------------------------------- 7. rows resident on the device
@pytest.mark.parametrize("select", ["reference", "diverse"])
def test_rows_resident_on_the_device(select):
    import torch

    n, d = 300, 100
    bits = to_bf16_bits(clustered_vectors(n, d, 17))
    cfg = ia.LeannConfig(m=8, m0=16, ef_construction=40)
    host = ia.LeannIndex.build_bf16(bits, cfg, batch=1, select=select)
    t = torch.from_numpy(bits.view(np.int16)).to("cuda:0")
    torch.cuda.synchronize()
    idx = ia.LeannIndex.build_bf16(config=cfg, batch=1, select=select, device_ptr=t.data_ptr(), n=n, d=d)
    assert idx.to_bytes() == host.to_bytes()
    del t  # the index keeps its own copy of the rows
    q = clustered_vectors(8, d, 18)
    got, want = idx.search_batch(q, 5, 32), host.search_batch(q, 5, 32)
    assert got[0].tolist() == want[0].tolist() and got[2].tolist() == want[2].tolist()
    assert got[1].view(np.uint32).tolist() == want[1].view(np.uint32).tolist()


# ---------------------------------------------------------------- 8. f32 through the new entry point
def test_f32_through_the_new_entry_point():
    n, d = 500, 24
    v = clustered_vectors(n, d, 7)
    cfg = ia.LeannConfig(m=8, m0=16, ef_construction=40)
    lv = np.ascontiguousarray(random_levels(n, 8, 3), dtype=np.uint64)
    l, c = _ffi.lib(), cfg._to_c()
    vp, lp = v.ctypes.data_as(C.c_void_p), lv.ctypes.data_as(C.c_void_p)
    for rule in (0, 1):
        o = _ffi.BuildOptionsC()
        l.isl_build_options_default(C.byref(o))
        o.select_rule = rule
        h_ex, h_rows = C.c_void_p(), C.c_void_p()
        assert l.isl_index_build_ex(C.byref(c), C.byref(o), vp, n, d, lp, 0, 0, C.byref(h_ex)) == 0
        assert l.isl_index_build_rows(C.byref(c), C.byref(o), vp, 0, n, d, lp, 0, 0, C.byref(h_rows)) == 0
        a, b = ia.LeannIndex(_handle=h_ex), ia.LeannIndex(_handle=h_rows)
        assert a.to_bytes() == b.to_bytes()
        ia_, da, ca = a.search_batch(v[:8], 3, 32)
        ib, db, cb = b.search_batch(v[:8], 3, 32)
        assert ia_.tolist() == ib.tolist() and da.view(np.uint32).tolist() == db.view(np.uint32).tolist()


# ---------------------------------------------------------------- 9. the finished index
def test_the_finished_index(orc, tmp_path):
    n, d = 300, 24
    bits = to_bf16_bits(clustered_vectors(n, d, 23))
    rows = widen(bits)
    cfg = ia.LeannConfig(m=8, m0=16, ef_construction=40)
    want, csr = reference_bytes(orc, rows, cfg, None)
    idx = ia.LeannIndex.build_bf16(bits, cfg, batch=1)
    assert len(idx) == n and idx.dimension() == d and idx.entry_point == 0
    same_answers(orc, idx, csr, rows, clustered_vectors(10, d, 24), 10, 48)  # no set_embeddings_bf16 needed
    blob = idx.to_bytes()
    assert blob == want and ia.LeannIndex.from_bytes(blob).to_bytes() == blob
    path = os.path.join(str(tmp_path), "sub", "bf16.idx")
    idx.save(path)
    back, meta = ia.LeannIndex.load(path)
    assert back.to_bytes() == blob and meta.num_vectors == n and meta.dimension == d
    with pytest.raises(ia.CoreError) as ex:
        idx.select_neighbors([3], [[1, 2]], 2)
    assert ex.value.kind == "Unsupported"


@pytest.mark.parametrize("select", ["reference", "diverse"])
def test_one_and_two_rows(orc, select):
    bits = to_bf16_bits(np.array([[1, 2, 3, 4, 5, 6, 7, 8], [8, 7, 6, 5, 4, 3, 2, 1]], np.float32))
    one = ia.LeannIndex.build_bf16(bits[:1], select=select)
    assert len(one) == 1 and one.entry_point == 0 and one.get_neighbors(0).tolist() == []
    assert one.search(widen(bits[0]), 3)[0][0] == 0
    two = ia.LeannIndex.build_bf16(bits, select=select)
    assert len(two) == 2 and two.get_neighbors(0).tolist() == [1] and two.get_neighbors(1).tolist() == [0]
    cfg = ia.LeannConfig()
    want = (reference_bytes(orc, widen(bits), cfg, None) if select == "reference"
            else definition_bytes(orc, widen(bits), cfg))[0]
    assert two.to_bytes() == want
    ids, dist, cnt = two.search_batch(widen(bits), 1, 8)
    assert ids[:, 0].tolist() == [0, 1]


# ---------------------------------------------------------------- 10. batched mode
@pytest.mark.parametrize("select", ["reference", "diverse"])
def test_batched_build_keeps_the_invariants(select):
    n, d = 3000, 16
    bits = to_bf16_bits(uniform_vectors(n, d, 21))  # all 3000 rounded rows stay distinct, and the oracle's
    cfg = ia.LeannConfig(m=8, m0=16, ef_construction=64)  # sequential build of them reaches recall@1 = 1.0
    idx = ia.LeannIndex.build_bf16(bits, cfg, batch=256, select=select)
    assert len(idx) == n and idx.dimension() == d and idx.entry_point == 0
    rows = [idx.get_neighbors(i).tolist() for i in range(n)]
    degs = np.array([len(r) for r in rows])
    assert degs.max() <= 16 and degs[1:].min() >= 1
    for i, r in enumerate(rows):
        assert len(set(r)) == len(r) and i not in r and all(x < n for x in r)
    ids, dist, cnt = idx.search_batch(widen(bits[::30]), 1, 64)
    recall = float((ids[:, 0] == np.arange(0, n, 30)).mean())
    print(f"{select}: mean degree {degs.mean():.2f}, self-query recall@1 at ef 64: {recall:.3f}")
    assert recall >= 0.9
