"""isl_hnsw_remove on the device: rows removed from an HnswGraph, in place, on every layer.  After each case the
handle equals tests/_hnsw_remove_ref.py's graph (the definition restated in Python over the lists the handle held
before, distances through the oracle): remap, len, entry point, max_level, levels, every list on every layer, and
to_bytes() against the bincode image of the definition's graph; a handful of queries answer as
_hnsw_build_ref.Graph.search over that graph, in ids and distance bits.  Every comparison is exact."""
import struct

import numpy as np
import pytest

import islands_amd as ia
import _hnsw_build_ref as ref
import _hnsw_remove_ref as href
from _data import random_levels, uniform_vectors
from test_gpu_hnsw import METRICS, bits
from test_gpu_hnsw_insert import small_image
from test_gpu_index_remove import index_from_lists
from test_hnsw_bytes import hnsw_to_bincode

pytestmark = pytest.mark.gpu

REMOVED = href.REMOVED
BASE = dict(m=4, m0=8, ef_construction=40)  # small caps: layers 1-3 are populated and an upper list can pass m

_built = {}


@pytest.fixture(scope="module", autouse=True)
def shared_builds():
    """the starting graphs are built once and shared among the tests; they go when the module is done"""
    yield
    _built.clear()


def base_rows():
    return uniform_vectors(600, 24, 11), random_levels(600, 4, 14)


def pick_ids(layers, n, count):
    """`count` ids; a single one is an id some list names (a node may have lost every inbound edge)"""
    if count == 1:
        return [int(layers[0][0][0])]
    return np.random.default_rng(count).choice(n, count, replace=False).astype(np.uint64)


def layers_of(g):
    n = len(g)
    return [[(g.neighbors(i, L) or []) for i in range(n)] for L in range(g.max_level + 1)]


def fresh(key, v, lv, metric=ia.DistanceMetric.Euclidean, rule="diverse", **cfg):
    """(graph, its layers): built on the device with one node per step the first time, read from its bytes
    afterwards"""
    cfg = dict(BASE, **cfg)
    if key not in _built:
        g = ia.HnswGraph.build(v, metric=metric, ml=1.0 / np.log(cfg["m"]), levels=lv, select=rule, batch=1, **cfg)
        _built[key] = g.to_bytes(), layers_of(g)
        return g, _built[key][1]
    blob, layers = _built[key]
    return ia.HnswGraph.from_bytes(blob), layers


def same_graph(g, want, rows, metric, cfg, ml=None):
    """`ml`: what the handle carries where it is not hnsw_to_bincode's 1 / ln(m) (the layer constructor: the
    default config's)"""
    assert len(g) == len(want) == rows.shape[0]
    assert g.entry_point == want.entry and g.max_level == want.max_level
    assert g.levels().tolist() == want.levels
    for i in range(len(want)):
        for L in range(want.levels[i] + 1):
            assert g.neighbors(i, L) == (want.layers[L][i] if L < len(want.layers) else []), (i, L)
        assert g.neighbors(i, want.levels[i] + 1) is None
    image = bytearray(hnsw_to_bincode(rows, want.layers if len(want) else [[]], want.levels, want.entry,
                                      want.max_level, metric=int(metric), **cfg))
    if ml is not None:
        image[24:32] = struct.pack("<d", ml)
    assert g.to_bytes() == bytes(image)


def same_answers(orc, g, want, rows, metric, cfg, rule="diverse", q=None, k=5, ef=30):
    seeded = href.seed_graph(ref.Graph(orc, rows, cfg["m"], cfg["m0"], cfg["ef_construction"], int(metric), rule), want,
                             rows)
    q = uniform_vectors(5, rows.shape[1], 99) if q is None else q
    for (ids, dd), x in zip(g.search_batch(q, k, ef), q):
        wi, wd = seeded.search(x, k, ef)
        assert ids.tolist() == wi and bits(dd).tolist() == bits(np.array(wd, np.float32)).tolist()
    return seeded


def remove_and_check(orc, g, layers, lv, v, ids, metric=ia.DistanceMetric.Euclidean, rule="diverse", alpha=1.0,
                     keep=True, stats=None, ml=None, **cfg):
    """remove `ids` from `g`, whose lists are `layers` over rows `v`: the handle is the definition's graph.
    Returns (the definition's graph, the survivors' rows)."""
    cfg = dict(BASE, **cfg)
    want = href.remove(orc, layers, [int(x) for x in lv], g.entry_point, g.max_level, v, ids, cfg["m"], cfg["m0"],
                       int(metric), rule, alpha, keep, stats)
    got = g.remove(ids, select=rule, alpha=alpha, keep_pruned=keep)
    assert got.dtype == np.uint64 and got.tolist() == want.remap.tolist()
    rows = np.ascontiguousarray(v[want.remap != REMOVED])
    same_graph(g, want, rows, metric, cfg, ml)
    same_answers(orc, g, want, rows, metric, cfg, rule)
    return want, rows


# ---------------------------------------------------------------- the definition, list by list and byte for byte
@pytest.mark.parametrize("count", [1, 20, 333])
@pytest.mark.parametrize("rule", ["reference", "diverse"])
@pytest.mark.parametrize("metric", METRICS)
def test_remove_is_the_definition(orc, metric, rule, count):
    v, lv = base_rows()
    g, layers = fresh(("base", int(metric)), v, lv, metric)
    assert g.max_level >= 3
    stats = []
    remove_and_check(orc, g, layers, lv, v, pick_ids(layers, 600, count), metric, rule, stats=stats)
    assert stats  # some list named a removed id
    if count == 333:  # lists outgrew M_L on layer 0 and above it: distances, the sort and the rule ran there
        assert max(c for L, _, c in stats if L == 0) > BASE["m0"]
        assert max(c for L, _, c in stats if L >= 1) > BASE["m"]


@pytest.mark.parametrize("alpha,keep", [(1.2, True), (1.0, False)])
def test_diverse_rule_parameters(orc, alpha, keep):
    v, lv = base_rows()
    g, layers = fresh(("base", 1), v, lv)
    remove_and_check(orc, g, layers, lv, v, pick_ids(layers, 600, 333), rule="diverse", alpha=alpha, keep=keep)


# ---------------------------------------------------------------- the entry point and the layers above it
def entry_case(orc, ids_of):
    v, lv = base_rows()
    g, layers = fresh(("base", 1), v, lv)
    top = int(lv.max())
    assert g.max_level == top and int(lv[g.entry_point]) == top
    want, _ = remove_and_check(orc, g, layers, lv, v, ids_of(g, lv, top))
    return g, want, lv, top


def test_the_entry_point_goes_and_a_peer_takes_over(orc):
    g, want, lv, top = entry_case(orc, lambda g, lv, top: [g.entry_point])
    assert (lv == top).sum() >= 2  # a peer shares the level
    assert want.max_level == top == g.max_level and int(want.levels[want.entry]) == top


def test_the_only_top_level_nodes_go_and_max_level_drops(orc):
    g, want, lv, top = entry_case(orc, lambda g, lv, top: np.flatnonzero(lv == top))
    assert g.max_level == top - 1 == want.max_level and len(want.layers) == top
    assert g.neighbors(g.entry_point, top) is None and g.entry_point == want.levels.index(top - 1)


def test_every_upper_node_goes_and_one_layer_is_left(orc):
    g, want, lv, top = entry_case(orc, lambda g, lv, top: np.flatnonzero(lv >= 1))
    assert g.max_level == 0 and g.entry_point == 0 and len(want.layers) == 1 and len(g) == int((lv == 0).sum())
    # ... and it grows again into layers
    assert g.insert(uniform_vectors(3, 24, 8), levels=[0, 2, 1], select="diverse") == len(want)
    assert g.max_level == 2 and g.entry_point == len(want) + 1


# ---------------------------------------------------------------- lists that name nodes lacking the layer
@pytest.mark.parametrize("gone", [[5], [250], [5, 250, 251]])
def test_lists_naming_a_node_that_lacks_the_layer(orc, gone):
    """the test_new_top_layer shape: node 250 rose above a graph whose top was node 5's layer 1, so its lists on
    layers 2..4 start with 5, a node without those layers.  Removed, 5 emits nothing there; kept, it stays named."""
    v = uniform_vectors(300, 16, 9)
    lv = np.zeros(300, np.uint64)
    lv[5], lv[250], lv[251], lv[260] = 1, 4, 4, 2
    cfg = dict(m=8, m0=16, ef_construction=64)
    g, layers = fresh("top", v, lv, ia.DistanceMetric.Cosine, "reference", **cfg)
    assert g.entry_point == 250 and layers[4][250] == [5, 251] and layers[4][251] == [5, 250] and 5 in layers[2][250]
    want, _ = remove_and_check(orc, g, layers, lv, v, gone, ia.DistanceMetric.Cosine, "reference", **cfg)
    if gone == [5]:
        assert want.layers[4][249] == [250] and want.layers[4][250] == [249] and want.levels[249] == 4
    if gone == [250]:
        assert want.entry == 250 and want.layers[4][250] == [5]  # 251 under its new id; 5 stays named
    if len(gone) == 3:
        assert want.max_level == 2 and want.entry == 257 and len(want.layers) == 3


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize("rule", ["reference", "diverse"])
def test_wide_lists(orc, rule):
    v, lv = uniform_vectors(400, 12, 33), random_levels(400, 64, 5)
    cfg = dict(m=64, m0=128, ef_construction=256)
    g, layers = fresh("wide", v, lv, ia.DistanceMetric.Euclidean, **cfg)
    assert max(len(r) for r in layers[0]) > 64  # rows of more than one 64-id slice
    stats = []
    remove_and_check(orc, g, layers, lv, v, pick_ids(layers, 400, 150), rule=rule, stats=stats, **cfg)
    assert max(c for L, _, c in stats if L == 0) > 128


def test_d768(orc):
    v, lv = uniform_vectors(400, 768, 5), random_levels(400, 8, 8)
    cfg = dict(m=8, m0=16, ef_construction=40)
    g, layers = fresh("d768", v, lv, ia.DistanceMetric.Cosine, **cfg)
    stats = []
    remove_and_check(orc, g, layers, lv, v, pick_ids(layers, 400, 200), ia.DistanceMetric.Cosine, stats=stats, **cfg)
    assert max(c for L, _, c in stats if L == 0) > 16


@pytest.mark.parametrize("count", [1, 20, 120])
@pytest.mark.parametrize("rule", ["reference", "diverse"])
def test_a_single_layer_graph_shrinks_as_the_flat_index_does(orc, rule, count):
    """every level 0 from the start: max_level 0 and a device level array of zeros.  The graph is the definition's,
    and a LeannIndex over the same layer-0 lists and m0 loses the same ids into the same remap and lists."""
    v, lv = uniform_vectors(200, 24, 21), np.zeros(200, np.uint64)
    g, layers = fresh("single", v, lv)
    assert g.max_level == 0 and len(layers) == 1
    flat = index_from_lists(layers[0], v, ia.LeannConfig(metric=ia.DistanceMetric.Euclidean, **BASE), entry=g.entry_point)
    ids = pick_ids(layers, 200, count)
    want, _ = remove_and_check(orc, g, layers, lv, v, ids, rule=rule)  # (the handle's remap is want.remap)
    assert flat.remove(ids, select=rule).tolist() == want.remap.tolist()
    assert len(flat) == len(g) == 200 - count
    for i in range(len(g)):
        assert flat.get_neighbors(i).tolist() == g.neighbors(i, 0), i


def test_repeated_ids_and_their_order(orc):
    v, lv = base_rows()
    ids = pick_ids(None, 600, 50)
    g, layers = fresh(("base", 1), v, lv)
    want, _ = remove_and_check(orc, g, layers, lv, v, ids)
    blob = g.to_bytes()
    shuffled = np.concatenate([ids[::-1], ids[:7], ids[20:22]])  # repeated ids count once, in any order
    h, _ = fresh(("base", 1), v, lv)
    assert h.remove(shuffled, select="diverse").tolist() == want.remap.tolist()
    assert h.to_bytes() == blob and len(h) == 550


def test_every_node_removed_and_the_graph_starts_again():
    v, lv = base_rows()
    g, _ = fresh(("base", 1), v, lv)
    remap = g.remove(np.arange(600), select="diverse")
    assert remap.tolist() == [REMOVED] * 600 and len(g) == 0 and g.is_empty()
    assert g.entry_point is None and g.max_level == 0 and g.search(v[0], 5, 20) == []
    kw = dict(BASE, metric=ia.DistanceMetric.Euclidean, ml=1.0 / np.log(4))
    assert g.to_bytes() == ia.HnswGraph.build(np.zeros((0, 0), np.float32), **kw).to_bytes()
    w, lw = uniform_vectors(150, 16, 4), random_levels(150, 4, 9)  # another dimension: the handle has none
    assert g.insert(w, levels=lw, select="diverse") == 0
    assert len(g) == 150 and g.to_bytes() == ia.HnswGraph.build(w, levels=lw, select="diverse", **kw).to_bytes()
    assert g.remove([]).tolist() == list(range(150))


def test_remove_insert_remove_is_the_same_chain_on_the_definitions(orc):
    """device: remove, insert (one node per step), remove, a search after each; the definitions: _hnsw_remove_ref,
    then _hnsw_build_ref.Graph.insert_step on the seeded graph, then _hnsw_remove_ref again"""
    v, lv = base_rows()
    metric, cfg = ia.DistanceMetric.Euclidean, BASE
    g, layers = fresh(("base", 1), v, lv)
    want, rows = remove_and_check(orc, g, layers, lv, v, pick_ids(layers, 600, 120))
    more, more_lv = uniform_vectors(12, 24, 77), [0, 1, 0, 0, 5, 0, 2, 0, 0, 1, 0, 0]  # (5: a new top layer)
    rows2 = np.concatenate([rows, more])
    seeded = href.seed_graph(ref.Graph(orc, rows2, cfg["m"], cfg["m0"], cfg["ef_construction"], int(metric), "diverse"),
                             want, rows2)
    levels2 = want.levels + more_lv
    for i in range(480, 492):
        seeded.insert_step([i], levels2)
    assert g.insert(more, levels=more_lv, select="diverse") == 480
    grown = href.Shrunk(href.layers_of_graph(seeded, 492), levels2, seeded.entry, seeded.max_level, None)
    assert seeded.max_level == 5 and seeded.entry == 484
    same_graph(g, grown, rows2, metric, cfg)
    same_answers(orc, g, grown, rows2, metric, cfg)
    ids = np.concatenate([[484, 481], np.random.default_rng(5).choice(480, 100, replace=False)])
    want3, rows3 = remove_and_check(orc, g, grown.layers, levels2, rows2, ids)
    assert want3.max_level < 5 and len(g) == 390


# ---------------------------------------------------------------- other handle sources
def test_a_graph_from_the_layer_constructor_shrinks(orc):
    v, lv = base_rows()
    src, layers = fresh(("base", 1), v, lv)
    g = ia.HnswGraph(v, layers, [int(x) for x in lv], src.entry_point, src.max_level, metric=ia.DistanceMetric.Euclidean,
                     **BASE)
    assert bits(g.get_vector(7)).tolist() == bits(v[7]).tolist()
    want, rows = remove_and_check(orc, g, layers, lv, v, pick_ids(layers, 600, 60), ml=1.0 / np.log(16.0))
    for node in (0, 7, 539):  # the object's own copy of the larger graph's rows is gone
        assert bits(g.get_vector(node)).tolist() == bits(rows[node]).tolist()
    assert g.level(539) == want.levels[539]


def test_a_graph_from_bytes_shrinks(orc):
    v, lv = base_rows()
    _, layers = fresh(("base", 1), v, lv)
    g, _ = fresh(("base", 1), v, lv)  # the second handle of a key comes from the bytes
    want, rows = remove_and_check(orc, g, layers, lv, v, pick_ids(layers, 600, 60))
    assert bits(g.get_vector(100)).tolist() == bits(rows[100]).tolist()


# ---------------------------------------------------------------- failures leave the handle unchanged
def state(g, q, k=5, ef=12):
    return g.to_bytes(), [(ids.tolist(), bits(dd).tolist()) for ids, dd in g.search_batch(q, k, ef)], len(g)


def test_an_unknown_id_leaves_the_graph_as_it_was():
    v, lv = base_rows()
    g, _ = fresh(("base", 1), v, lv)
    q = uniform_vectors(4, 24, 8)
    before = state(g, q)
    with pytest.raises(ia.CoreError) as e:
        g.remove([3, 600, 5], select="diverse")
    assert e.value.kind == "NodeNotFound" and e.value.node == 600
    assert state(g, q) == before
    assert len(g.remove([3, 5], select="diverse")) == 600 and len(g) == 598  # and it still shrinks


@pytest.mark.parametrize("lists,words", [(dict(layer1_of_0=[1, 2, 3, 4, 5]), "longer than"),
                                         (dict(layer0_of_0=list(range(1, 10))), "longer than"),
                                         (dict(layer0_of_0=[1, 1, 2]), "verbatim")],
                         ids=["upper list longer than m", "layer-0 list longer than m0", "an id twice in a layer-0 list"])
def test_graphs_the_tables_cannot_hold_are_refused(lists, words):
    v, layers, lv = small_image(**lists)
    g = ia.HnswGraph.from_bytes(hnsw_to_bincode(v, layers, lv, 0, 1, m=4, m0=8, ef_construction=16, metric=1))
    q = uniform_vectors(4, 4, 8)
    before = state(g, q)
    with pytest.raises(ia.CoreError) as e:
        g.remove([7])
    assert e.value.kind == "Unsupported" and words in str(e.value) and "isl_hnsw_remove" in str(e.value), str(e.value)
    assert state(g, q) == before


def test_a_graph_without_its_levels_is_refused():
    v, layers, lv = small_image()
    kw = dict(m=4, m0=8, ef_construction=16, metric=ia.DistanceMetric.Euclidean)
    g = ia.HnswGraph(v, layers, [0] * 12, 0, 1, **kw)
    q = uniform_vectors(4, 4, 8)
    before = state(g, q)
    with pytest.raises(ia.CoreError) as e:
        g.remove([7])
    assert e.value.kind == "Unsupported" and "levels" in str(e.value) and "isl_hnsw_remove" in str(e.value)
    assert state(g, q) == before
    g = ia.HnswGraph(v, layers, lv, 0, 1, **kw)  # the same layers with their levels shrink
    assert g.remove([7]).tolist() == [0, 1, 2, 3, 4, 5, 6, REMOVED, 7, 8, 9, 10]
    assert len(g) == 11 and g.neighbors(6, 0) == [7, 8] and g.neighbors(5, 0) == [6, 7, 8]  # 7's own [8, 9] stand in


def test_the_core_index_still_refuses_the_flat_removal():
    import ctypes as C
    v, lv = base_rows()
    g, _ = fresh(("base", 1), v, lv)
    lib = ia._ffi.lib()
    core = C.c_void_p.from_address(g._h.value)  # isl_hnsw's first member: the layer-0 isl_index
    ids = np.array([3], np.uint64)
    st = lib.isl_index_remove(core, None, ids.ctypes.data_as(C.c_void_p), 1, None, None)
    assert lib.isl_status_name(st).decode() == "Unsupported" and len(g) == 600


# ---------------------------------------------------------------- searchers made before the removal
def test_searchers_made_before_the_removal_see_the_shrunk_graph(orc):
    v, lv = base_rows()
    g, layers = fresh(("base", 1), v, lv)
    one = ia.Searcher(g).top_k(5).ef(30)
    many = ia.MultiIndexSearcher(ia.SearchConfig(top_k=5, ef=30))
    many.add_index("a", g)
    q = uniform_vectors(3, 24, 99)
    assert len(one.search(q[0])) == 5 and many.total_vectors() == 600
    want, rows = remove_and_check(orc, g, layers, lv, v, pick_ids(layers, 600, 200))
    seeded = href.seed_graph(ref.Graph(orc, rows, BASE["m"], BASE["m0"], BASE["ef_construction"], 1, "diverse"), want, rows)
    assert many.total_vectors() == 400
    for x in q:
        wi, _ = seeded.search(x, 5, 30)
        assert [r.id for r in one.search(x)] == wi
        assert [(name, r.id) for name, r in many.search(x)] == [("a", i) for i in wi]
    for r in ia.Searcher(g).include_vectors().top_k(3).search(q[0]):
        assert (r.vector == rows[r.id]).all()
