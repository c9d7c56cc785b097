"""isl_hnsw_insert on the device: rows inserted into an existing HnswGraph.  Insertion is sequential in id
order, so with one node per step build(A) followed by insert(B) must give the graph build(A || B) gives:
the bytes equal the bincode image of the oracle's graph over all rows (reference rule), every list equals
the Python definition over all rows (diverse rule).  Batched: structural invariants, and for the diverse
rule reachability and recall under the caps of test_batched_build.  Every comparison is exact."""
import numpy as np
import pytest

import islands_amd as ia
import _hnsw_build_ref as ref
from _data import clustered_vectors, random_levels, uniform_vectors
from test_gpu_hnsw import assert_same, bits
from test_gpu_hnsw_build import METRICS, structure
from test_hnsw_bytes import hnsw_to_bincode

pytestmark = pytest.mark.gpu

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


def layers_of(h, n):
    return [[(h.neighbors(i, L) or []) for i in range(n)] for L in range(h.max_level + 1)]


def oracle_bytes(h, v, lv, m, m0, efc, metric):
    n = v.shape[0]
    return hnsw_to_bincode(v, layers_of(h, n), [int(x) for x in lv], h.entry_point, h.max_level, m=m, m0=m0,
                           ef_construction=efc, metric=int(metric))


def split_build(v, lv, n0, m, m0, efc, metric, **kw):
    g = ia.HnswGraph.build(v[:n0], m=m, m0=m0, ef_construction=efc, metric=metric, ml=1.0 / np.log(m),
                           levels=lv[:n0], **kw)
    assert g.insert(v[n0:], levels=lv[n0:], **kw) == n0
    return g


def base_rows():
    return uniform_vectors(600, 24, 11), random_levels(600, 16, 14)


@pytest.mark.parametrize("n0", [1, 20, 333])
@pytest.mark.parametrize("metric", METRICS)
def test_split_build_is_the_oracle(orc, metric, n0):
    v, lv = base_rows()
    h = oracle_graph(orc, ("base", int(metric)), v, lv, 16, 32, 200, metric)
    g = split_build(v, lv, n0, 16, 32, 200, metric)
    assert len(g) == 600 and g.entry_point == h.entry_point and g.max_level == h.max_level
    assert g.levels().tolist() == [int(x) for x in lv]
    for i in range(600):
        for L in range(int(lv[i]) + 1):
            assert g.neighbors(i, L) == list(h.neighbors(i, L) or []), (i, L)
        assert g.neighbors(i, int(lv[i]) + 1) is None
    assert g.to_bytes() == oracle_bytes(h, v, lv, 16, 32, 200, metric)
    # the grown graph searches like the oracle's: padded adjacency and lanes were set up again
    assert_same(h, g, uniform_vectors(24, 24, 99), 10, 50)


def test_several_inserts_in_a_row(orc):
    v, lv = base_rows()
    metric = ia.DistanceMetric.Euclidean
    h = oracle_graph(orc, ("base", int(metric)), v, lv, 16, 32, 200, metric)
    g = ia.HnswGraph.build(v[:100], m=16, m0=32, ef_construction=200, metric=metric, levels=lv[:100])
    for i in range(100, 105):
        assert g.insert(v[i], levels=lv[i:i + 1]) == i and len(g) == i + 1
    assert g.insert(v[105:305], levels=lv[105:305]) == 105
    assert g.insert(v[305:], levels=lv[305:]) == 305
    one_call = ia.HnswGraph.build(v, m=16, m0=32, ef_construction=200, metric=metric, levels=lv)
    assert g.to_bytes() == one_call.to_bytes() == oracle_bytes(h, v, lv, 16, 32, 200, metric)


def test_new_top_layer(orc):
    v = uniform_vectors(300, 16, 9)
    lv = np.zeros(300, np.uint64)
    lv[5], lv[250], lv[251], lv[260] = 1, 4, 4, 2
    h = oracle_graph(orc, "top", v, lv, 8, 16, 64, 0)
    g = split_build(v, lv, 200, 8, 16, 64, 0)
    assert g.entry_point == 250 and g.max_level == 4
    # node 250 rose above a graph whose top was node 5's layer 1: its lists on layers 2..4 are [current] = [5],
    # a node that lacks those layers (no back link).  Node 251 searches layer 4 from 250, meets 5 through that
    # list and 250 itself: the oracle's list is both, nearest first.
    assert list(h.neighbors(251, 4)) == [5, 250] and g.neighbors(251, 4) == [5, 250]
    for node in (250, 251):
        for L in (2, 3, 4):
            assert g.neighbors(node, L) == list(h.neighbors(node, L) or []), (node, L)
    assert g.level(250) == 4 and g.level(260) == 2 and g.level(5) == 1
    assert g.to_bytes() == oracle_bytes(h, v, lv, 8, 16, 64, 0)


def test_wide_lists(orc):
    v, lv = uniform_vectors(400, 12, 33), random_levels(400, 64, 5)
    h = oracle_graph(orc, "wide", v, lv, 64, 128, 256, 1)
    g = split_build(v, lv, 200, 64, 128, 256, 1)
    assert max(len(g.neighbors(i, 0)) for i in range(200)) > 64  # imported rows of more than one slice
    assert g.to_bytes() == oracle_bytes(h, v, lv, 64, 128, 256, 1)


def test_d768(orc):
    v, lv = uniform_vectors(400, 768, 5), random_levels(400, 8, 8)
    h = oracle_graph(orc, "d768", v, lv, 8, 16, 40, 0)
    g = split_build(v, lv, 250, 8, 16, 40, 0)
    assert g.to_bytes() == oracle_bytes(h, v, lv, 8, 16, 40, 0)


def test_ties(orc):
    base = uniform_vectors(60, 8, 3)
    v = np.concatenate([base, base, base[:30], base[:60]]).astype(np.float32)
    lv = random_levels(v.shape[0], 6, 24)
    metric = ia.DistanceMetric.Euclidean
    h = oracle_graph(orc, "ties", v, lv, 6, 12, 30, metric)
    g = split_build(v, lv, 100, 6, 12, 30, metric)
    assert g.to_bytes() == oracle_bytes(h, v, lv, 6, 12, 30, metric)
    g.search_batch(base[:20], 10, 40)
    assert g.last_stats()["exact_path"] > 0  # equal distances: the heap-exact kernel decides


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("alpha", [1.0, 1.2])
@pytest.mark.parametrize("rows", [("uniform", 0), ("clustered", 1)])
def test_diverse_rule_is_the_definition(orc, rows, alpha, keep):
    kind, metric = rows
    v = uniform_vectors(500, 24, 7) if kind == "uniform" else clustered_vectors(500, 16, 7)
    lv = random_levels(500, 8, 4)
    key = (kind, alpha, keep)
    if key not in _definitions:
        _definitions[key] = ref.build(orc, v, lv, 8, 16, 64, metric, "diverse", alpha, keep)
    want = _definitions[key]
    g = split_build(v, lv, 300, 8, 16, 64, metric, select="diverse", alpha=alpha, keep_pruned=keep)
    assert g.entry_point == want.entry and g.max_level == want.max_level and want.max_level >= 1
    for i in range(500):
        for L in range(int(lv[i]) + 1):
            assert g.neighbors(i, L) == list(want.conn[i][L]), (i, L)


def prefix_and_whole(orc, n0=333):
    v, lv = base_rows()
    whole = oracle_graph(orc, ("base", 0), v, lv, 16, 32, 200, 0)
    part = oracle_graph(orc, ("base-prefix", n0), v[:n0], lv[:n0], 16, 32, 200, 0)
    return v, lv, part, whole


def test_onto_a_graph_from_bytes(orc):
    n0 = 333
    v, lv, part, whole = prefix_and_whole(orc, n0)
    g = ia.HnswGraph.from_bytes(oracle_bytes(part, v[:n0], lv[:n0], 16, 32, 200, 0))
    assert g.insert(v[n0:], levels=lv[n0:]) == n0
    assert g.to_bytes() == oracle_bytes(whole, v, lv, 16, 32, 200, 0)
    for node in (7, 599):
        assert bits(g.get_vector(node)).tolist() == bits(v[node]).tolist()


def test_onto_a_graph_from_layers(orc):
    n0 = 333
    v, lv, part, whole = prefix_and_whole(orc, n0)
    g = ia.HnswGraph(v[:n0], layers_of(part, n0), [int(x) for x in lv[:n0]], part.entry_point, part.max_level,
                     m=16, m0=32, ef_construction=200, metric=ia.DistanceMetric.Cosine)
    assert bits(g.get_vector(7)).tolist() == bits(v[7]).tolist()
    assert g.insert(v[n0:], levels=lv[n0:]) == n0
    assert g.to_bytes() == oracle_bytes(whole, v, lv, 16, 32, 200, 0)
    for node in (7, 599):  # the object's own copy of the smaller graph's rows is gone
        assert bits(g.get_vector(node)).tolist() == bits(v[node]).tolist()
    assert g.level(599) == int(lv[599])


def test_device_rows_and_seeded_levels():
    torch = pytest.importorskip("torch")
    v = clustered_vectors(800, 32, 3)
    lv = random_levels(800, 8, 6)
    n0 = 500
    kw = dict(m=8, m0=16, ef_construction=64, metric=ia.DistanceMetric.Euclidean, select="diverse")
    blob = ia.HnswGraph.build(v, levels=lv, **kw).to_bytes()
    g = ia.HnswGraph.build(v[:n0], levels=lv[:n0], **kw)
    t = torch.from_numpy(v[n0:]).to("cuda:0")
    assert g.insert(t, levels=lv[n0:], select="diverse") == n0
    assert g.to_bytes() == blob
    # the seed's stream is addressed by position: the insert continues it at len
    a = ia.HnswGraph.build(v, level_seed=5, **kw)
    b = ia.HnswGraph.build(v[:n0], level_seed=5, **kw)
    b.insert(v[n0:], level_seed=5, select="diverse")
    assert a.to_bytes() == b.to_bytes() and a.max_level >= 1


@pytest.mark.parametrize("n", [1, 150])
def test_insert_into_the_empty_graph(n):
    v, lv = uniform_vectors(n, 16, 4), random_levels(n, 8, 9)
    kw = dict(m=8, m0=16, ef_construction=64, metric=ia.DistanceMetric.DotProduct, ml=0.4, max_layers=9)
    g = ia.HnswGraph.build(np.zeros((0, 0), np.float32), **kw)
    assert g.is_empty() and g.insert(v, levels=lv) == 0
    assert len(g) == n and g.to_bytes() == ia.HnswGraph.build(v, levels=lv, **kw).to_bytes()
    assert bits(g.get_vector(n - 1)).tolist() == bits(v[n - 1]).tolist()


def test_failure_leaves_the_graph_as_it_was():
    v, lv = uniform_vectors(300, 16, 6), random_levels(300, 8, 2)
    g = ia.HnswGraph.build(v[:200], m=8, m0=16, ef_construction=64, levels=lv[:200])
    q = uniform_vectors(16, 16, 8)

    def state():
        return g.to_bytes(), [(ids.tolist(), bits(dd).tolist()) for ids, dd in g.search_batch(q, 10, 40)]

    before = state()
    with pytest.raises(ia.CoreError) as e:
        g.insert(uniform_vectors(100, 12, 6))
    assert e.value.kind == "DimensionMismatch" and (e.value.expected, e.value.actual) == (16, 12)
    assert state() == before and len(g) == 200
    bad = lv[200:].copy()
    bad[40] = 16
    with pytest.raises(ia.CoreError) as e:
        g.insert(v[200:], levels=bad)
    assert e.value.kind == "InvalidArgument"
    assert state() == before and len(g) == 200
    assert g.insert(v[200:], levels=lv[200:]) == 200  # and it still grows
    assert g.to_bytes() == ia.HnswGraph.build(v, m=8, m0=16, ef_construction=64, levels=lv).to_bytes()


@pytest.mark.parametrize("kind", ["uniform", "clustered"])
@pytest.mark.parametrize("rule", ["reference", "diverse"])
def test_batched_insert(kind, rule):
    """The split batched build, under the caps of test_batched_build on the same rows.  Measured on an
    MI355X (diverse rule, uniform and clustered): 0 of 3000 nodes without an inbound layer-0 edge, self-query
    recall@1 100 / 100 -- the one-call build's figures."""
    n, n0, d, m, m0, efc = 3000, 2000, 16, 8, 16, 64
    v = uniform_vectors(n, d, 21) if kind == "uniform" else clustered_vectors(n, d, 21)
    metric = 0 if kind == "uniform" else 1
    lv = random_levels(n, m, 3)
    g = ia.HnswGraph.build(v[:n0], m=m, m0=m0, ef_construction=efc, metric=metric, levels=lv[:n0], select=rule,
                           batch=256)
    assert g.insert(v[n0:], levels=lv[n0:], select=rule, batch=256) == n0
    assert len(g) == n and g.levels().tolist() == [int(x) for x in lv]
    top = int(lv.max())
    assert g.max_level == top and g.entry_point == int(np.argmax(lv == top))
    layer0 = structure(g, n, lv, m, m0)
    if rule == "diverse":
        lost = ref.no_inbound(layer0)
        probes = list(range(0, n, 30))
        got = g.search_batch(v[probes], 1, 64)
        hits = sum(1 for i, (ids, _) in zip(probes, got) if ids.tolist()[:1] == [i])
        print(f"{kind}: split batched build, nodes without an inbound layer-0 edge {lost} of {n}; "
              f"self-query recall@1 {hits}/{len(probes)}")
        assert lost <= 0.01 * n
        assert hits >= 0.95 * len(probes)


def small_image(layer0_of_0=None, layer1_of_0=None):
    """12 x 4 rows, m 4 / m0 8, nodes 0..5 on layer 1: a ring on each layer, node 0's lists as given"""
    n = 12
    v = uniform_vectors(n, 4, 2)
    lv = [1] * 6 + [0] * 6
    layer0 = [[(i + 1) % n, (i + 2) % n] for i in range(n)]
    layer1 = [[(i + 1) % 6] if i < 6 else [] for i in range(n)]
    if layer0_of_0 is not None:
        layer0[0] = layer0_of_0
    if layer1_of_0 is not None:
        layer1[0] = layer1_of_0
    return v, [layer0, layer1], lv


REFUSED_IMAGES = [("upper list longer than m", dict(layer1_of_0=[1, 2, 3, 4, 5]), "longer than"),
                  ("layer-0 list longer than m0", dict(layer0_of_0=list(range(1, 10))), "longer than"),
                  ("an id twice in a layer-0 list", dict(layer0_of_0=[1, 1, 2]), "verbatim")]


@pytest.mark.parametrize("what,lists,words", REFUSED_IMAGES, ids=[c[0] for c in REFUSED_IMAGES])
def test_graphs_the_tables_cannot_hold_are_refused(what, lists, words):
    """from_bytes accepts these images; the builder's tables cannot take them over.  The over-long upper list is
    seen by the import kernel alone.  Each is refused with a message that says which, the handle as it was."""
    v, layers, lv = small_image(**lists)
    g = ia.HnswGraph.from_bytes(hnsw_to_bincode(v, layers, lv, 0, 1, m=4, m0=8, ef_construction=16, metric=1))
    q = uniform_vectors(4, 4, 8)
    before = g.to_bytes(), [(ids.tolist(), bits(dd).tolist()) for ids, dd in g.search_batch(q, 5, 12)]
    with pytest.raises(ia.CoreError) as e:
        g.insert(uniform_vectors(3, 4, 5), levels=[0, 2, 0])
    assert e.value.kind == "Unsupported" and words in str(e.value), str(e.value)
    after = g.to_bytes(), [(ids.tolist(), bits(dd).tolist()) for ids, dd in g.search_batch(q, 5, 12)]
    assert after == before and len(g) == 12


def test_a_graph_without_its_levels_is_refused():
    """The link kernel takes "has the layer" from the levels.  A handle with layers above 0 whose levels do not
    reach them (here: all 0) is refused; the same layers with their levels grow."""
    v, layers, lv = small_image()
    kw = dict(m=4, m0=8, ef_construction=16, metric=ia.DistanceMetric.Euclidean)
    g = ia.HnswGraph(v, layers, [0] * 12, 0, 1, **kw)
    blob = g.to_bytes()
    with pytest.raises(ia.CoreError) as e:
        g.insert(uniform_vectors(3, 4, 5), levels=[0, 2, 0])
    assert e.value.kind == "Unsupported" and "levels" in str(e.value)
    assert g.to_bytes() == blob and len(g) == 12
    g = ia.HnswGraph(v, layers, lv, 0, 1, **kw)
    assert g.insert(uniform_vectors(3, 4, 5), levels=[0, 2, 0]) == 12
    assert len(g) == 15 and g.entry_point == 13 and g.max_level == 2
