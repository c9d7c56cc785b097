"""An HnswGraph over bf16 rows on the device: build, insert, remove, hand-over and search.  A bf16 value is exactly
representable in f32 and every distance of the builder, the removal and the search goes through the strictly
ordered f32 chain, so the graph over bf16 bits is -- list for list, byte for byte and answer for answer -- the
graph over widen(bits).  Every expected value is the oracle's (its HnswGraph::insert and search over the widened
rows) or the Python definitions' (tests/_hnsw_build_ref.py, tests/_hnsw_remove_ref.py) over the widened rows; none
is the library's.  Ids are compared as lists, distances as u32 bit patterns, graphs list by list and as bytes.
row_storage() is what keeps "widen on entry" from passing: the table is the flat index's bf16 table."""
import numpy as np
import pytest

import islands_amd as ia
import _hnsw_build_ref as ref
import _hnsw_remove_ref as href
from _data import clustered_vectors, random_levels, uniform_vectors
from test_gpu_build_bf16 import to_bf16_bits, widen
from test_gpu_hnsw import METRICS, assert_same, bits as fbits
from test_gpu_hnsw_build import structure
from test_gpu_hnsw_remove import same_answers, same_graph
from test_hnsw_bytes import hnsw_to_bincode

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
_oracle_graphs = {}
_definitions = {}


@pytest.fixture(scope="module", autouse=True)
def shared_references():
    """the references are computed once and shared among the tests; they go when the module is done"""
    yield
    _oracle_graphs.clear()
    _definitions.clear()


def oracle_graph(orc, key, v, lv, m, m0, efc, metric):
    """the oracle's graph of v[0..n) inserted one by one (built once per key, never changed)"""
    if key not in _oracle_graphs:
        h = orc.Hnsw(m=m, m0=m0, ef_construction=efc, metric=int(metric))
        for i in range(v.shape[0]):
            st, idx = h.insert(v[i], int(lv[i]))
            assert st == 0 and idx == i
        _oracle_graphs[key] = h
    return _oracle_graphs[key]


def definition(orc, key, v, lv, m, m0, efc, metric, rule, alpha=1.0, keep=True):
    if key not in _definitions:
        _definitions[key] = ref.build(orc, v, lv, m, m0, efc, int(metric), rule, alpha, keep)
    return _definitions[key]


def layers_of(h, n):
    return [[(h.neighbors(i, L) or []) for i in range(n)] for L in range(h.max_level + 1)]


def oracle_bytes(h, v, lv, m, m0, efc, metric):
    return hnsw_to_bincode(v, layers_of(h, v.shape[0]), [int(x) for x in lv], h.entry_point, h.max_level, m=m,
                           m0=m0, ef_construction=efc, metric=int(metric))


def same_as_oracle(g, h, lv):
    n = len(lv)
    assert len(g) == n and g.entry_point == h.entry_point and g.max_level == h.max_level
    assert g.levels().tolist() == [int(x) for x in lv]
    for i in range(n):  # (first, for a readable failure; the bytes say the same)
        for L in range(int(lv[i]) + 1):
            assert g.neighbors(i, L) == list(h.neighbors(i, L) or []), (i, L)
        assert g.neighbors(i, int(lv[i]) + 1) is None


def check_reference(orc, key, bits, lv, m, m0, efc, metric, queries=None, k=10, ef=50, f32_twin=True):
    """build_bf16(bits) == the oracle's inserts of widen(bits), byte for byte, == build(widen(bits)); then the
    bf16 graph answers f32 queries and bf16-valued queries as the oracle does"""
    v = widen(bits)
    n, d = v.shape
    h = oracle_graph(orc, key, v, lv, m, m0, efc, metric)
    kw = dict(m=m, m0=m0, ef_construction=efc, metric=metric, ml=1.0 / np.log(m), levels=lv)
    g = ia.HnswGraph.build_bf16(bits, **kw)
    same_as_oracle(g, h, lv)
    want = oracle_bytes(h, v, lv, m, m0, efc, metric)
    assert g.to_bytes() == want
    if f32_twin:
        assert ia.HnswGraph.build(v, **kw).to_bytes() == want
    assert g.row_storage()["dtype"] == BF16
    q = uniform_vectors(24, d, 99) if queries is None else queries
    for qq in (q, widen(to_bf16_bits(q))):
        assert_same(h, g, qq, k, ef)
        assert_same(h, g, qq, min(3, n), 3)
    return h, g


# ---------------------------------------------------------------- 1. reference rule, one node per step
def base_rows():
    return to_bf16_bits(uniform_vectors(600, 24, 11)), random_levels(600, 16, 14)


@pytest.mark.parametrize("metric", METRICS)
def test_reference_rule_is_the_oracle_over_the_widened_rows(orc, metric):
    bits, lv = base_rows()
    h, g = check_reference(orc, ("base", int(metric)), bits, lv, 16, 32, 200, metric)
    assert h.max_level >= 1
    assert fbits(g.get_vector(17)).tolist() == fbits(widen(bits[17])).tolist()


# ---------------------------------------------------------------- 2. dimensions around the loads
@pytest.mark.parametrize("metric", [ia.DistanceMetric.Cosine, ia.DistanceMetric.Euclidean])
@pytest.mark.parametrize("n,d", [(300, 3), (300, 100), (400, 768)])
def test_dimensions(orc, metric, n, d):
    """d 3: one guarded load; d 100: a multiple of 4 but not of 8, the stride is padded; d 768: the ring of loads"""
    bits, lv = to_bf16_bits(uniform_vectors(n, d, 50 + d)), random_levels(n, 8, 8)
    h, _ = check_reference(orc, ("dim", d, int(metric)), bits, lv, 8, 16, 40, metric, f32_twin=d != 768)
    assert h.max_level >= 1


# ---------------------------------------------------------------- 3. ties
def test_ties(orc):
    base = to_bf16_bits(uniform_vectors(60, 8, 3))
    bits = np.concatenate([base, base, base[:30], base[:60]])  # 210 rows, equal distances everywhere
    h, g = check_reference(orc, "ties", bits, random_levels(bits.shape[0], 6, 24), 6, 12, 30,
                           ia.DistanceMetric.Euclidean, queries=widen(base[:20]), k=10, ef=40)
    g.search_batch(widen(base[:20]), 10, 40)
    assert g.last_stats()["exact_path"] > 0  # equal distances: the heap-exact kernel decides


# ---------------------------------------------------------------- 4. wide lists
@pytest.mark.parametrize("shape", [(64, 128, 256, 1), (32, 64, 400, 0)])
def test_wide_lists(orc, shape):
    """(64, 128, 256): rows of more than one 64-id slice.  (32, 64, 400): a list is at most m0 = 64 ids and one
    under re-selection holds 65 -- the second slice is one id; "longer than 64" can hold for m0 = 128 alone."""
    m, m0, efc, metric = shape
    bits, lv = to_bf16_bits(uniform_vectors(400, 12, 33)), random_levels(400, m, 5)
    h, g = check_reference(orc, ("wide", m), bits, lv, m, m0, efc, metric)
    longest = max(len(g.neighbors(i, 0)) for i in range(400))
    assert longest > 64 if m0 == 128 else longest == 64


# ---------------------------------------------------------------- 5. a rising top layer
def test_rising_top_layer(orc):
    lv = np.zeros(300, np.uint64)
    lv[5], lv[40], lv[100], lv[101], lv[200] = 3, 1, 5, 5, 2
    h, g = check_reference(orc, "rising", to_bf16_bits(uniform_vectors(300, 16, 9)), lv, 8, 16, 64, 0)
    assert g.entry_point == 100 and g.max_level == 5 and h.entry_point == 100
    assert g.neighbors(101, 5) == list(h.neighbors(101, 5)) and g.level(5) == 3


# ---------------------------------------------------------------- 6. one node, two nodes
@pytest.mark.parametrize("n", [1, 2])
def test_tiny(orc, n):
    check_reference(orc, ("tiny", n), to_bf16_bits(uniform_vectors(n, 8, 2)), np.asarray([1, 0][:n], np.uint64), 4, 8,
                    16, 1, queries=uniform_vectors(3, 8, 4), k=2, ef=4)


# ---------------------------------------------------------------- 7. the diverse rule
def diverse_rows(kind):
    v = uniform_vectors(500, 24, 7) if kind == "uniform" else clustered_vectors(500, 16, 7)
    return to_bf16_bits(v), random_levels(500, 8, 4)


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("alpha", [1.0, 1.2])
@pytest.mark.parametrize("rows", [("uniform", 0), ("clustered", 1)])
def test_diverse_rule_is_the_definition(orc, rows, alpha, keep):
    kind, metric = rows
    bits, lv = diverse_rows(kind)
    want = definition(orc, ("diverse", kind, alpha, keep), widen(bits), lv, 8, 16, 64, metric, "diverse", alpha, keep)
    g = ia.HnswGraph.build_bf16(bits, m=8, m0=16, ef_construction=64, metric=metric, levels=lv, select="diverse",
                                alpha=alpha, keep_pruned=keep)
    assert g.entry_point == want.entry and g.max_level == want.max_level and want.max_level >= 1
    for i in range(500):
        for L in range(int(lv[i]) + 1):
            assert g.neighbors(i, L) == list(want.conn[i][L]), (i, L)
    assert g.row_storage()["dtype"] == BF16


# ---------------------------------------------------------------- 8. insert
def split_build(bits, lv, n0, m, m0, efc, metric, **kw):
    g = ia.HnswGraph.build_bf16(bits[:n0], m=m, m0=m0, ef_construction=efc, metric=metric, ml=1.0 / np.log(m),
                                levels=lv[:n0], **kw)
    assert g.insert_bf16(bits[n0:], levels=lv[n0:], **kw) == n0
    return g


def test_split_build_reference_rule_with_a_new_top_layer(orc):
    """node 250 enters through insert_bf16 and rises above every layer the built graph had"""
    bits = to_bf16_bits(uniform_vectors(500, 24, 7))
    lv = random_levels(500, 8, 4)
    lv[250] = int(lv.max()) + 1
    h = oracle_graph(orc, "split-top", widen(bits), lv, 8, 16, 64, 1)
    assert int(lv[:200].max()) < int(lv[250]) and h.entry_point == 250
    g = split_build(bits, lv, 200, 8, 16, 64, 1)
    same_as_oracle(g, h, lv)
    want = oracle_bytes(h, widen(bits), lv, 8, 16, 64, 1)
    assert g.to_bytes() == want
    assert ia.HnswGraph.build_bf16(bits, m=8, m0=16, ef_construction=64, metric=1, ml=1.0 / np.log(8),
                                   levels=lv).to_bytes() == want
    assert_same(h, g, uniform_vectors(24, 24, 99), 10, 50)  # padded adjacency and lanes were set up again


def test_split_build_diverse_rule(orc):
    bits, lv = diverse_rows("uniform")
    want = definition(orc, ("diverse", "uniform", 1.0, True), widen(bits), lv, 8, 16, 64, 0, "diverse")
    g = split_build(bits, lv, 200, 8, 16, 64, 0, select="diverse")
    assert g.entry_point == want.entry and g.max_level == want.max_level
    for i in range(500):
        for L in range(int(lv[i]) + 1):
            assert g.neighbors(i, L) == list(want.conn[i][L]), (i, L)
    one_call = ia.HnswGraph.build_bf16(bits, m=8, m0=16, ef_construction=64, metric=0, ml=1.0 / np.log(8), levels=lv,
                                       select="diverse")
    assert g.to_bytes() == one_call.to_bytes()
    assert g.row_storage() == one_call.row_storage()


def test_rows_of_the_other_type_are_refused_and_an_empty_graph_takes_bf16(orc):
    bits, lv = diverse_rows("uniform")
    kw = dict(m=8, m0=16, ef_construction=64, metric=0, ml=1.0 / np.log(8))
    g16 = ia.HnswGraph.build_bf16(bits[:200], levels=lv[:200], **kw)
    g32 = ia.HnswGraph.build(widen(bits[:200]), levels=lv[:200], **kw)
    b16, b32 = g16.to_bytes(), g32.to_bytes()
    assert b16 == b32
    with pytest.raises(ia.CoreError) as e:
        g16.insert(widen(bits[200:]), levels=lv[200:])
    assert e.value.kind == "Unsupported" and "bf16" in str(e.value)
    with pytest.raises(ia.CoreError) as e:
        g32.insert_bf16(bits[200:], levels=lv[200:])
    assert e.value.kind == "Unsupported" and "float32" in str(e.value)
    assert g16.to_bytes() == b16 and g32.to_bytes() == b32 and len(g16) == len(g32) == 200
    assert g16.row_storage()["dtype"] == BF16 and g32.row_storage()["dtype"] == F32
    # an empty handle takes the type of the rows it is given
    empty = ia.HnswGraph.build_bf16(np.zeros((0, 0), np.uint16), **kw)
    assert empty.row_storage() == {"dtype": F32, "block_bytes": 0}
    assert empty.insert_bf16(bits, levels=lv) == 0
    assert empty.row_storage()["dtype"] == BF16
    h = oracle_graph(orc, "empty-takes", widen(bits), lv, 8, 16, 64, 0)
    assert empty.to_bytes() == oracle_bytes(h, widen(bits), lv, 8, 16, 64, 0)


# ---------------------------------------------------------------- 9. remove
REMOVE_CFG = dict(m=4, m0=8, ef_construction=40)  # small caps: layers 1-3 are populated, an upper list can pass m


def flat_block_bytes(bits):
    """row_storage()["block_bytes"] of a flat LeannIndex with these rows set as bf16"""
    n = bits.shape[0]
    g = ia.CsrGraph(node_offsets=np.zeros(n + 1, np.uint64), neighbors=np.zeros(0, np.uint64),
                    levels=np.zeros(n, np.uint64), entry_point=0, max_level=0, num_nodes=n,
                    degree_counts=np.zeros(n, np.uint64))
    idx = ia.LeannIndex.from_csr(g, ia.LeannConfig(), dimension=bits.shape[1]).upload(0)
    idx.set_embeddings_bf16(bits)
    st = idx.row_storage()
    assert st["dtype"] == BF16
    return st["block_bytes"]


@pytest.mark.parametrize("rule", ["reference", "diverse"])
def test_remove_is_the_definition_over_the_widened_rows(orc, rule):
    bits, lv = to_bf16_bits(uniform_vectors(600, 24, 11)), random_levels(600, 4, 14)
    v, metric, cfg = widen(bits), ia.DistanceMetric.Euclidean, REMOVE_CFG
    start = definition(orc, "remove-start", v, lv, cfg["m"], cfg["m0"], cfg["ef_construction"], metric, "diverse")
    layers = href.layers_of_graph(start, 600)
    g = ia.HnswGraph.build_bf16(bits, metric=metric, ml=1.0 / np.log(cfg["m"]), levels=lv, select="diverse", **cfg)
    top = int(lv.max())
    assert g.max_level == top == start.max_level >= 3 and g.entry_point == start.entry
    # the entry point, the whole top layer, and a hundred others
    ids = np.unique(np.concatenate([np.flatnonzero(lv == top),
                                    np.random.default_rng(9).choice(600, 100, replace=False)])).astype(np.uint64)
    assert g.entry_point in ids
    stats = []
    want = href.remove(orc, layers, [int(x) for x in lv], start.entry, start.max_level, v, ids, cfg["m"], cfg["m0"],
                       int(metric), rule, 1.0, True, stats)
    assert want.max_level == top - 1 and max(c for L, _, c in stats if L == 0) > cfg["m0"]  # distances were needed
    got = g.remove(ids, select=rule)
    assert got.dtype == np.uint64 and got.tolist() == want.remap.tolist()
    keep = want.remap != href.REMOVED
    rows, kept_bits = np.ascontiguousarray(v[keep]), np.ascontiguousarray(bits[keep])
    same_graph(g, want, rows, metric, cfg)  # lists, levels, entry point, and the bytes over the widened survivors
    for node in (0, 1, len(want) // 2, len(want) - 1):
        assert fbits(g.get_vector(node)).tolist() == fbits(rows[node]).tolist()
    st = g.row_storage()
    assert st["dtype"] == BF16 and st["block_bytes"] == flat_block_bytes(kept_bits)
    same_answers(orc, g, want, rows, metric, cfg, rule)
    if rule == "diverse":
        # the shrunk graph grows again, through insert_bf16, as the definition does
        more, more_lv = to_bf16_bits(uniform_vectors(12, 24, 77)), [0, 1, 0, 0, 5, 0, 2, 0, 0, 1, 0, 0]
        n1 = len(want)
        rows2 = np.concatenate([rows, widen(more)])
        seeded = href.seed_graph(ref.Graph(orc, rows2, cfg["m"], cfg["m0"], cfg["ef_construction"], int(metric),
                                           "diverse"), want, rows2)
        levels2 = want.levels + more_lv
        for i in range(n1, n1 + 12):
            seeded.insert_step([i], levels2)
        assert g.insert_bf16(more, levels=more_lv, select="diverse") == n1
        grown = href.Shrunk(href.layers_of_graph(seeded, n1 + 12), levels2, seeded.entry, seeded.max_level, None)
        assert seeded.max_level == 5 and seeded.entry == n1 + 4
        same_graph(g, grown, rows2, metric, cfg)
        same_answers(orc, g, grown, rows2, metric, cfg)
        assert g.row_storage()["dtype"] == BF16
        with pytest.raises(ia.CoreError) as e:
            g.insert(widen(more), levels=more_lv)
        assert e.value.kind == "Unsupported"


# ---------------------------------------------------------------- 10. hand-over: the search descent alone
@pytest.mark.parametrize("metric", METRICS)
def test_a_graph_handed_over_with_bf16_rows_searches_like_the_oracle(orc, metric):
    bits, lv = base_rows()
    v = widen(bits)
    h = oracle_graph(orc, ("base", int(metric)), v, lv, 16, 32, 200, metric)
    g = ia.HnswGraph.from_layers_bf16(bits, layers_of(h, 600), [int(x) for x in lv], h.entry_point, h.max_level,
                                      m=16, m0=32, ef_construction=200, metric=metric)
    assert h.max_level >= 1 and g.row_storage()["dtype"] == BF16
    q = uniform_vectors(40, 24, 99)
    assert_same(h, g, q, 10, 50)
    assert_same(h, g, widen(to_bf16_bits(q)), 10, 50)
    assert_same(h, g, v[:16], 5, 5)
    assert_same(h, g, q[:8], 20, 10)  # ef < k -> ef = k
    image = bytearray(oracle_bytes(h, v, lv, 16, 32, 200, metric))
    image[24:32] = np.float64(1.0 / np.log(16.0)).tobytes()  # (the layer constructor: the default config's ml)
    assert g.to_bytes() == bytes(image)
    for r in ia.Searcher(g).include_vectors().top_k(3).search(q[0]):  # the widened rows
        assert fbits(r.vector).tolist() == fbits(v[r.id]).tolist()


def test_handed_over_d768(orc):
    bits, lv = to_bf16_bits(uniform_vectors(400, 768, 50 + 768)), random_levels(400, 8, 8)
    h = oracle_graph(orc, ("dim", 768, 0), widen(bits), lv, 8, 16, 40, 0)
    g = ia.HnswGraph.from_layers_bf16(bits, layers_of(h, 400), [int(x) for x in lv], h.entry_point, h.max_level,
                                      m=8, m0=16, ef_construction=40, metric=0)
    q = uniform_vectors(24, 768, 6)
    for ef in (1, 3, 64):
        assert_same(h, g, q, 1 if ef < 10 else 10, ef)
        assert_same(h, g, widen(to_bf16_bits(q)), 1 if ef < 10 else 10, ef)


# ---------------------------------------------------------------- 11. storage
def test_row_storage_is_the_flat_index_s_bf16_table():
    bits, lv = diverse_rows("clustered")  # 500 x 16
    kw = dict(m=8, m0=16, ef_construction=64, metric=1, select="diverse")
    g = ia.HnswGraph.build_bf16(bits[:300], levels=lv[:300], **kw)
    st = g.row_storage()
    assert st["dtype"] == BF16 and st["block_bytes"] == flat_block_bytes(bits[:300])
    f32 = ia.HnswGraph.build(widen(bits[:300]), levels=lv[:300], **kw).row_storage()
    assert f32["dtype"] == F32 and f32["block_bytes"] >= 2 * 300 * 16 * 2 > st["block_bytes"]
    g.insert_bf16(bits[300:], levels=lv[300:], select="diverse")
    st = g.row_storage()
    assert st["dtype"] == BF16 and st["block_bytes"] == flat_block_bytes(bits)
    remap = g.remove(np.arange(0, 500, 3), select="diverse")
    keep = remap != href.REMOVED
    st = g.row_storage()
    assert st["dtype"] == BF16 and st["block_bytes"] == flat_block_bytes(bits[keep]) and len(g) == int(keep.sum())
    # a dimension whose stride is padded
    odd = to_bf16_bits(uniform_vectors(50, 100, 3))
    assert ia.HnswGraph.build_bf16(odd, m=4, m0=8, ef_construction=16).row_storage()["block_bytes"] == \
        flat_block_bytes(odd)


# ---------------------------------------------------------------- 12. rows resident on the device
def test_device_resident_rows(orc):
    torch = pytest.importorskip("torch")
    bits, lv = diverse_rows("clustered")
    kw = dict(m=8, m0=16, ef_construction=64, metric=ia.DistanceMetric.Euclidean, levels=lv, select="diverse")
    blob = ia.HnswGraph.build_bf16(bits, **kw).to_bytes()
    want = definition(orc, ("diverse", "clustered", 1.0, True), widen(bits), lv, 8, 16, 64, 1, "diverse")
    t = torch.from_numpy(bits.view(np.int16)).to("cuda:0")
    g = ia.HnswGraph.build_bf16(t, **kw)
    assert g.to_bytes() == blob
    t.zero_()  # the graph keeps its own copy
    del t
    torch.cuda.synchronize()
    assert g.row_storage()["dtype"] == BF16
    q = uniform_vectors(10, 16, 8)
    for (ids, dd), x in zip(g.search_batch(q, 5, 40), q):
        wi, wd = want.search(x, 5, 40)
        assert ids.tolist() == wi and fbits(dd).tolist() == fbits(np.array(wd, np.float32)).tolist()
    # the same tensor as bfloat16, and insert_bf16 from the device
    tb = torch.from_numpy(bits.view(np.int16)).to("cuda:0").view(torch.bfloat16)
    kw2 = dict(kw, levels=lv[:300])
    g2 = ia.HnswGraph.build_bf16(tb[:300], **kw2)
    assert g2.insert_bf16(tb[300:], levels=lv[300:], select="diverse") == 300
    assert g2.to_bytes() == blob
    with pytest.raises(TypeError):
        ia.HnswGraph.build_bf16(torch.zeros(4, 4, device="cuda:0"), m=4, m0=8, ef_construction=16)


# ---------------------------------------------------------------- 13. batched mode
@pytest.mark.parametrize("kind", ["uniform", "clustered"])
@pytest.mark.parametrize("rule", ["reference", "diverse"])
def test_batched_build(kind, rule):
    """the bounds are test_gpu_hnsw_build.test_batched_build's for the f32 build of this mode; the sequential
    definition over these widened rows leaves 0 nodes without an inbound edge"""
    n, d, m, m0, efc = 3000, 16, 8, 16, 64
    bits = to_bf16_bits(uniform_vectors(n, d, 21) if kind == "uniform" else clustered_vectors(n, d, 21))
    metric = 0 if kind == "uniform" else 1
    lv = random_levels(n, m, 3)
    g = ia.HnswGraph.build_bf16(bits, m=m, m0=m0, ef_construction=efc, metric=metric, levels=lv, select=rule,
                                batch=256)
    assert len(g) == n and g.levels().tolist() == [int(x) for x in lv]
    top = int(lv.max())
    assert g.max_level == top and g.entry_point == int(np.argmax(lv == top))
    assert g.row_storage()["dtype"] == BF16
    layer0 = structure(g, n, lv, m, m0)
    if rule == "diverse":
        lost = ref.no_inbound(layer0)
        probes = list(range(0, n, 30))
        got = g.search_batch(widen(bits[probes]), 1, 64)
        hits = sum(1 for i, (ids, _) in zip(probes, got) if ids.tolist()[:1] == [i])
        print(f"{kind}: nodes without an inbound layer-0 edge {lost} of {n}; self-query recall@1 {hits}/{len(probes)}")
        assert lost <= 0.01 * n
        assert hits >= 0.95 * len(probes)
