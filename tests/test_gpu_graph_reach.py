"""Graph reachability and covering entry seeds on the GPU against tests/_reach_ref.py, the definitions of
include/islands_amd.h restated over adjacency lists.  Every output is independent of execution order, so every
comparison is exact.  Shapes are the smallest at which each piece can go wrong: a frontier of one node over 70 levels,
a list wider than 128 ids, 30 000 claims on 150 nodes in one level, sizes that are no multiple of a wave or a
workgroup, a frontier of more waves than one grid holds, graphs the library itself changed under the handle."""
import ctypes as C

import numpy as np
import pytest

import islands_amd as ia
from _data import random_csr, uniform_vectors

import _entry_seeds_ref as sref
import _reach_ref as rr

pytestmark = pytest.mark.gpu

COS = ia.DistanceMetric.Cosine


# ------------------------------------------------------------------ helpers
def index_from_lists(lists, entry=0, dimension=4):
    """A graph-only LeannIndex on the device whose rows are `lists` as given (repeats and ids >= len included)."""
    n = len(lists)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(l) for l in lists])
    nb = np.fromiter((v for l in lists for v in l), dtype=np.uint64, count=int(off[-1]))
    g = ia.CsrGraph(node_offsets=off, neighbors=nb, levels=np.zeros(n, np.uint64), entry_point=entry, max_level=0,
                    num_nodes=n, degree_counts=np.diff(off).astype(np.uint64))
    return ia.LeannIndex.from_csr(g, ia.LeannConfig(), dimension=dimension).upload(0)


def lists_of(idx):
    """list(u) of every node, read back through get_neighbors"""
    return [rr.distinct(idx.get_neighbors(u)) for u in range(len(idx))]


def report_of(res):
    return {k: res[k] for k in rr.REPORT_FIELDS}


def check(idx_or_graph, lists, sources, member=None, default=False, **kw):
    """report, depth and in_degree of one call against the definition; `default`: the call names no sources"""
    depth, indeg, rep = rr.reach(lists, sources, member)
    res = idx_or_graph.reachability(sources=None if default else sources, depth=True, in_degree=True, **kw)
    assert report_of(res) == rep, (report_of(res), rep)
    assert res["depth"].dtype == np.uint32 and res["depth"].tolist() == depth.tolist()
    assert res["in_degree"].tolist() == indeg.tolist()
    return res


def contended_lists(tail=False):
    """Node 0 lists 1..200 (a row wider than 128), nodes 1..200 all list the same 150 nodes 201..350, 49 isolated
    nodes pad to 400; `tail`: 350 -> 351 -> 352, a third and fourth level behind the contended one."""
    lists = [list(range(1, 201))] + [list(range(201, 351)) for _ in range(200)] + [[] for _ in range(199)]
    if tail:
        lists[350], lists[351] = [351], [352]
    assert len(lists) == 400
    return lists


# ------------------------------------------------------------------ hand graphs
def test_one_node_without_edges():
    check(index_from_lists([[]]), [[]], [0])


def test_ring_of_70_entered_at_node_5():
    lists = [[(i + 1) % 70] for i in range(70)]
    idx = index_from_lists(lists, entry=5)
    res = check(idx, lists, [5], default=True)
    assert res["levels"] == 70 and res["reached"] == 70 and res["depth"][4] == 69


def test_dangling_edge_is_counted_and_not_followed():
    lists = [[1], [2, 9], [3], [4], [], [0]]  # 9 names no node of 6
    res = check(index_from_lists(lists), lists, [0])
    assert res["dangling_edges"] == 1 and res["edges"] == 4 and res["reached"] == 5
    far = [[1], [0x7FFFFFE0, 2], []]  # the largest id the device copy represents
    assert check(index_from_lists(far), far, [0])["dangling_edges"] == 1


def test_self_loop_is_an_ordinary_edge():
    lists = [[0, 1], [1], [2, 0]]
    res = check(index_from_lists(lists), lists, [0])
    assert res["in_degree"].tolist() == [2, 2, 1] and res["edges"] == 3 and res["no_inbound"] == 0


def test_two_rings_joined_downstream_of_the_source():
    lists = [[1], [2], [3, 4], [0], [5], [6], [4]]
    idx = index_from_lists(lists, entry=5)
    res = check(idx, lists, [5], default=True)
    assert res["reached"] == 3 and (res["depth"][:4] == ia.DEPTH_UNREACHED).all()
    assert check(idx, lists, [0])["reached"] == 7


def test_repeated_ids_within_a_row_are_one_edge():
    raw = [[1, 1, 2, 1], [0, 0], [2, 2, 2]]
    idx = index_from_lists(raw)
    lists = lists_of(idx)
    assert lists == [[1, 2], [0], [2]]
    res = check(idx, lists, [0])
    assert res["in_degree"].tolist() == [1, 1, 2] and res["edges"] == 4


# ------------------------------------------------------------------ contended claims, wide rows
def test_contended_claims_on_150_nodes():
    lists = contended_lists()
    res = check(index_from_lists(lists), lists, [0])
    assert (res["depth"][201:351] == 2).all() and res["reached"] == 351 and res["levels"] == 3
    assert res["edges"] == 200 + 30000 and res["max_in_degree"] == 200


def test_contended_claims_enter_the_next_frontier_once():
    lists = contended_lists(tail=True)
    res = check(index_from_lists(lists), lists, [0])
    # a node that won its claim twice would sit in the queue twice: reached, edges and the levels behind it say so
    assert res["reached"] == 353 and res["edges"] == 200 + 30000 + 2 and res["levels"] == 5
    assert res["depth"][351] == 3 and res["depth"][352] == 4


# ------------------------------------------------------------------ random digraphs
_random = {}


def random_case(n):
    """(lists, sources, (depth, in_degree, report)) of random_csr(n, 6, seed, dup=True): computed once, shared"""
    if n not in _random:
        off, nb = random_csr(n, 6, 1000 + n, dup=True)
        lists = rr.lists_from_csr(off, nb)
        r = np.random.default_rng(n)
        # some nodes lose their lists, so that part of the graph stays unreached and some nodes have no inbound edge
        for u in r.choice(n, size=n // 3, replace=False):
            lists[int(u)] = []
        sources = [next(u for u in range(n) if lists[u])]  # the first node that kept its list
        _random[n] = (lists, sources, rr.reach(lists, sources))
    return _random[n]


@pytest.mark.parametrize("n", [65, 97, 1000, 50000])
def test_random_digraph_host_arrays(n):
    lists, sources, (depth, indeg, rep) = random_case(n)
    idx = index_from_lists(lists, entry=sources[0])
    res = idx.reachability(sources=sources, depth=True, in_degree=True)
    assert report_of(res) == rep
    assert res["depth"].tolist() == depth.tolist() and res["in_degree"].tolist() == indeg.tolist()
    assert 1 < rep["reached"] < n and rep["no_inbound"] > 0  # the case is not a trivial one
    # either array alone, neither, and no report
    only_d = idx.reachability(sources=sources, depth=True)
    only_i = idx.reachability(sources=sources, in_degree=True)
    none = idx.reachability(sources=sources)
    assert only_d["depth"].tolist() == depth.tolist() and "in_degree" not in only_d
    assert only_i["in_degree"].tolist() == indeg.tolist() and "depth" not in only_i
    assert report_of(only_d) == report_of(only_i) == report_of(none) == rep
    lib = ia._ffi.lib()
    src = np.asarray(sources, np.uint64)
    d2, i2 = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    assert lib.isl_index_reachability(idx._h, src.ctypes.data, src.size, d2.ctypes.data, i2.ctypes.data, 0, None) == 0
    assert d2.tolist() == depth.tolist() and i2.tolist() == indeg.tolist()
    assert lib.isl_index_reachability(idx._h, src.ctypes.data, src.size, d2.ctypes.data, None, 0, None) == 0
    assert lib.isl_index_reachability(idx._h, src.ctypes.data, src.size, None, None, 0, None) == 0


@pytest.mark.parametrize("n", [65, 97, 1000, 50000])
def test_random_digraph_device_arrays(n):
    import torch
    lists, sources, (depth, indeg, rep) = random_case(n)
    idx = index_from_lists(lists, entry=sources[0])
    dd = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    di = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    res = idx.reachability(sources=sources, d_depth_ptr=dd.data_ptr(), d_in_degree_ptr=di.data_ptr())
    assert report_of(res) == rep and "depth" not in res
    assert dd.cpu().numpy().view(np.uint32).tolist() == depth.tolist()
    assert di.cpu().numpy().view(np.uint32).tolist() == indeg.tolist()
    di.fill_(7)
    torch.cuda.synchronize()
    res = idx.reachability(sources=sources, d_depth_ptr=dd.data_ptr())  # in_degree NULL: the buffer is not touched
    assert report_of(res) == rep and (di.cpu().numpy() == 7).all()
    res = idx.reachability(sources=sources, d_in_degree_ptr=di.data_ptr())
    assert di.cpu().numpy().view(np.uint32).tolist() == indeg.tolist()


# ------------------------------------------------------------------ sources
def test_explicit_sources_with_repeats():
    lists, _, _ = random_case(1000)
    idx = index_from_lists(lists)
    res = check(idx, lists, [7, 900, 7, 7, 13, 900])
    assert res["sources"] == 3
    with pytest.raises(ia.CoreError) as e:
        idx.reachability(sources=[7, 1000])
    assert e.value.kind == "NodeNotFound" and e.value.node == 1000


def test_default_sources_follow_the_seed_table():
    x, _ = sref.fixture()
    lists, _, _ = random_case(1000)
    idx = index_from_lists(lists, entry=3, dimension=x.shape[1])
    idx.set_embeddings(x[:1000])
    check(idx, lists, [3], default=True)
    ids = [40, 41, 999, 40]
    idx.set_entry_seeds(ids)
    res = check(idx, lists, ids, default=True)
    assert report_of(res) == report_of(idx.reachability(sources=ids)) and res["sources"] == 3
    idx.set_entry_seeds([])
    check(idx, lists, [3], default=True)


# ------------------------------------------------------------------ every kind of index
@pytest.mark.parametrize("rows", ["none", "f32", "bf16", "fp8", "recompute"])
def test_rows_make_no_difference(orc, rows):
    lists, sources, (depth, indeg, rep) = random_case(97)
    v = uniform_vectors(97, 16, 5)
    if rows == "recompute":
        from test_gpu_encoder import _recompute_case
        _, enc, tok, lens, emb = _recompute_case(orc, n=97)
        idx = index_from_lists(lists, entry=sources[0], dimension=emb.shape[1])
        idx.set_recompute_provider(enc, tok, lens)
    else:
        idx = index_from_lists(lists, entry=sources[0], dimension=16)
        if rows == "f32":
            idx.set_embeddings(v)
        elif rows == "bf16":
            idx.set_embeddings_bf16(sref.bf16_bits(v))
        elif rows == "fp8":
            idx.set_embeddings_fp8(*ia.quantize_fp8_e4m3(v))
    check(idx, lists, sources, default=True)


# ------------------------------------------------------------------ a graph the library changed
@pytest.mark.parametrize("rule", ["reference", "diverse"])
def test_build_insert_remove_are_followed(rule):
    v = uniform_vectors(640, 16, 17)
    cfg = ia.LeannConfig(m=8, m0=16, ef_construction=40)
    idx = ia.LeannIndex.build(v[:600], cfg, batch=32, select=rule)
    check(idx, lists_of(idx), [idx.entry_point], default=True)
    idx.insert(v[600:], batch=8, select=rule)
    assert len(idx) == 640
    lists = lists_of(idx)
    check(idx, lists, [idx.entry_point], default=True)
    check(idx, lists, [639, 0])
    idx.remove(list(range(5, 600, 15)), select=rule)
    assert len(idx) == 600
    lists = lists_of(idx)
    res = check(idx, lists, [idx.entry_point], default=True)
    assert res["nodes"] == 600 and res["dangling_edges"] == 0


# ------------------------------------------------------------------ HnswGraph
def hnsw_layer(g, layer, levels):
    member = levels >= layer
    lists = [(g.neighbors(i, layer) or []) if member[i] else [] for i in range(len(g))]
    return lists, member


@pytest.mark.parametrize("case", ["reference", "diverse", "bf16"])
def test_every_layer_of_an_hnsw_graph(case):
    from _data import random_levels
    n, d, m, m0, efc = 3000, 16, 8, 16, 64
    v = uniform_vectors(n, d, 21)
    lv = random_levels(n, m, 3)
    kw = dict(m=m, m0=m0, ef_construction=efc, levels=lv, batch=256, select="reference" if case == "reference" else "diverse")
    g = ia.HnswGraph.build_bf16(sref.bf16_bits(v), **kw) if case == "bf16" else ia.HnswGraph.build(v, **kw)
    levels = g.levels().astype(np.int64)
    assert g.max_level >= 2
    for layer in range(g.max_level + 1):
        lists, member = hnsw_layer(g, layer, levels)
        res = check(g, lists, [g.entry_point], member, default=True, layer=layer)
        assert res["nodes"] == int(member.sum())
        assert (res["depth"][~member] == ia.DEPTH_ABSENT).all() and (res["in_degree"][~member] == 0).all()
    # explicit sources on an upper layer, and one that is not on it
    on1 = np.nonzero(levels >= 1)[0]
    lists, member = hnsw_layer(g, 1, levels)
    check(g, lists, [int(on1[-1]), int(on1[0]), int(on1[-1])], member, layer=1)
    below = int(np.nonzero(levels == 0)[0][0])
    with pytest.raises(ia.CoreError) as e:
        g.reachability(layer=1, sources=[int(on1[0]), below])
    assert e.value.kind == "NodeNotFound" and e.value.node == below
    with pytest.raises(ia.CoreError) as e:
        g.reachability(layer=g.max_level + 1)
    assert e.value.kind == "InvalidArgument"


def test_a_list_that_names_a_node_below_the_layer():
    """the reference rule leaves such ids in upper lists: dangling on that layer, not followed, no in-degree"""
    lv = np.zeros(300, np.uint64)
    lv[5], lv[40], lv[100], lv[101], lv[200] = 3, 1, 5, 5, 2
    g = ia.HnswGraph.build(uniform_vectors(300, 16, 9), m=8, m0=16, ef_construction=64, ml=1.0 / np.log(8), levels=lv)
    assert g.neighbors(101, 5) == [100, 5]
    levels = g.levels().astype(np.int64)
    for layer in range(g.max_level + 1):
        lists, member = hnsw_layer(g, layer, levels)
        res = check(g, lists, [100], member, default=True, layer=layer)
    lists, member = hnsw_layer(g, 5, levels)
    res = check(g, lists, [101], member, layer=5)
    assert res["dangling_edges"] >= 1 and res["nodes"] == 2 and res["depth"][5] == ia.DEPTH_ABSENT


def test_an_empty_hnsw_graph():
    g = ia.HnswGraph.build(np.zeros((0, 4), np.float32))
    with pytest.raises(ia.CoreError) as e:
        g.reachability(layer=1)
    assert e.value.kind == "InvalidArgument"  # layer > max_level is answered first
    with pytest.raises(ia.CoreError) as e:
        g.reachability()
    assert e.value.kind == "EmptyCollection"


# ------------------------------------------------------------------ cover
def fixture_index(orc, bf16=False):
    from test_gpu_entry_seeds import fixture_index as make
    return make(orc, COS, bf16=bf16)


_fixture_lists = {}


def fixture_lists(idx, tag):
    if tag not in _fixture_lists:
        _fixture_lists[tag] = lists_of(idx)
    return _fixture_lists[tag]


def test_cover_on_the_clustered_fixture(orc):
    from test_gpu_entry_seeds import assert_seeded_search
    idx, csr, x, q = fixture_index(orc)
    lists = fixture_lists(idx, "f32")
    _, _, before = rr.reach(lists, [0])
    assert report_of(idx.reachability()) == before and before["reached"] < 2000
    ids0, _, cnt0 = idx.search_batch(q, 5, 32)
    recall0 = sref.recall_at(orc, 0, q, x, ids0, cnt0, 5)
    want, added, unreached = rr.cover(lists, [0], 65536)
    got = idx.cover_entry_seeds()
    assert got["ids"].dtype == np.uint64 and got["ids"].tolist() == want and got["unreached"] == unreached == 0
    assert added == len(want) - 1 > 0 and idx.entry_seeds().tolist() == want
    after = idx.reachability()
    assert after["reached"] == 2000 and after["sources"] == len(want)
    ids1, _, cnt1, _ = assert_seeded_search(orc, idx, csr, x, q, 5, 32, COS)
    recall1 = sref.recall_at(orc, 0, q, x, ids1, cnt1, 5)
    print(f"recall@5: {recall0:.3f} from node 0 ({before['reached']} of 2000 rows reachable), {recall1:.3f} with the "
          f"{len(want)} seeds of the cover")
    assert recall1 > recall0
    again = idx.cover_entry_seeds()  # nothing left to add: the table stays
    assert again["ids"].tolist() == want and again["unreached"] == 0


def test_cover_capped_at_ten_seeds(orc):
    idx, csr, x, q = fixture_index(orc)
    lists = fixture_lists(idx, "f32")
    full, _, _ = rr.cover(lists, [0], 65536)
    want, _, unreached = rr.cover(lists, [0], 10)
    got = idx.cover_entry_seeds(10)
    assert got["ids"].tolist() == want == full[:10] and got["unreached"] == unreached > 0
    assert idx.entry_seeds().tolist() == want
    assert idx.reachability()["reached"] == 2000 - unreached


def test_cover_keeps_an_existing_table_as_its_prefix(orc):
    idx, csr, x, q = fixture_index(orc)
    lists = fixture_lists(idx, "f32")
    first = idx.select_entry_seeds(8).tolist()
    want, added, unreached = rr.cover(lists, first, 65536)
    got = idx.cover_entry_seeds()
    assert got["ids"].tolist() == want and want[:8] == first and added > 0 and got["unreached"] == 0
    assert idx.reachability()["reached"] == 2000


def test_cover_on_a_ring_adds_nothing_and_installs_nothing(orc):
    from test_gpu_entry_seeds import chain_csr, make_index
    x = uniform_vectors(70, 8, 3)
    idx = make_index(chain_csr(orc, 70, entry=5), x)
    got = idx.cover_entry_seeds()
    assert got["ids"].size == 0 and got["unreached"] == 0 and idx.entry_seeds().size == 0
    idx.set_entry_seeds([9, 9])
    got = idx.cover_entry_seeds()
    assert got["ids"].tolist() == [9, 9] and idx.entry_seeds().tolist() == [9, 9]


def test_cover_bf16_rows(orc):
    from test_gpu_entry_seeds import assert_seeded_search
    idx, csr, x, q = fixture_index(orc, bf16=True)
    lists = fixture_lists(idx, "bf16")
    want, _, _ = rr.cover(lists, [0], 65536)
    got = idx.cover_entry_seeds()
    assert got["ids"].tolist() == want and got["unreached"] == 0 and idx.reachability()["reached"] == 2000
    assert_seeded_search(orc, idx, csr, x, q, 5, 32, COS)


def _unchanged_after(idx, call, kind, queries=None):
    table, n = idx.entry_seeds().tolist(), len(idx)
    before = idx.search_batch(queries, 3, 16) if queries is not None else None
    for c in (call, lambda: idx.select_entry_seeds(4)):  # the same status as select_entry_seeds
        with pytest.raises(ia.CoreError) as e:
            c()
        assert e.value.kind == kind, (e.value.kind, kind)
    assert idx.entry_seeds().tolist() == table and len(idx) == n
    if before is not None:
        after = idx.search_batch(queries, 3, 16)
        for a, b in zip(before, after):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_cover_refusals_leave_the_index_unchanged(orc):
    lists, sources, _ = random_case(97)
    v = uniform_vectors(97, 16, 5)
    q = uniform_vectors(4, 16, 6)
    # fp8 rows
    idx = index_from_lists(lists, entry=sources[0], dimension=16)
    idx.set_embeddings_fp8(*ia.quantize_fp8_e4m3(v))
    _unchanged_after(idx, lambda: idx.cover_entry_seeds(), "Unsupported", q)
    # the recompute provider
    from test_gpu_encoder import _recompute_case
    _, enc, tok, lens, emb = _recompute_case(orc, n=97)
    rec = index_from_lists(lists, entry=sources[0], dimension=emb.shape[1])
    rec.set_recompute_provider(enc, tok, lens)
    _unchanged_after(rec, lambda: rec.cover_entry_seeds(), "Unsupported")
    assert len(rec.search(emb[5], 1)) == 1
    # a graph without rows
    bare = index_from_lists(lists, entry=sources[0], dimension=16)
    _unchanged_after(bare, lambda: bare.cover_entry_seeds(), "Unsupported")
    # above the cap: nothing is looked at
    f32 = index_from_lists(lists, entry=sources[0], dimension=16)
    f32.set_embeddings(v)
    f32.set_entry_seeds([1, 2])
    table, n = f32.entry_seeds().tolist(), len(f32)
    before = f32.search_batch(q, 3, 16)
    with pytest.raises(ia.CoreError) as e:
        f32.cover_entry_seeds(65537)
    assert e.value.kind == "Unsupported" and f32.entry_seeds().tolist() == table and len(f32) == n
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(before, f32.search_batch(q, 3, 16)))
    # an empty index
    empty = ia.LeannIndex.with_defaults()
    _unchanged_after(empty, lambda: empty.cover_entry_seeds(), "EmptyCollection")
    # the core of an HnswGraph
    g = ia.HnswGraph.build(uniform_vectors(60, 8, 3), m=4, m0=8, ef_construction=16)
    blob = g.to_bytes()
    core = C.c_void_p.from_address(g._h.value)  # isl_hnsw's first member: the layer-0 isl_index
    lib = ia._ffi.lib()
    n_out, un = C.c_uint64(7), C.c_uint64(7)
    st = lib.isl_index_cover_entry_seeds(core, 8, None, C.byref(n_out), C.byref(un))
    assert lib.isl_status_name(st).decode() == "Unsupported" and "HnswGraph" in lib.isl_last_error_message().decode()
    assert st == lib.isl_index_select_entry_seeds(core, 8, None, C.byref(n_out))
    assert g.to_bytes() == blob and len(g) == 60
