"""isl_index_insert on the device: rows inserted into a built LeannIndex, in place.  LeannIndex::build is a loop
over ids that reads only the lists so far and entry_point / max_level, so with one node per step build(A)
followed by insert(B) must give the index build(A || B) gives: the bytes equal those of the oracle's index over
all rows (reference rule) or of tests/_diverse_ref.py's (diverse rule), through LeannIndex.from_csr(...).to_bytes()
as in test_gpu_build*.py.  Then what the handle carries besides the graph: the heap-exact kernel's pool, the
prepared lanes, the entry seeds, the PQ codes.  Batched: structural invariants, and for the diverse rule the
reachability and self-recall caps of test_gpu_hnsw_insert.py.  Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import islands_amd as ia
import _diverse_ref as dref
import _entry_seeds_ref as sref
from _data import clustered_vectors, random_levels, uniform_vectors
from test_gpu_build import reference_bytes
from test_gpu_build_bf16 import csr_bytes, same_answers, to_bf16_bits, widen
from test_gpu_entry_seeds import assert_seeded_search

pytestmark = pytest.mark.gpu

METRICS = [ia.DistanceMetric.Cosine, ia.DistanceMetric.Euclidean, ia.DistanceMetric.DotProduct,
           ia.DistanceMetric.Manhattan]

_references = {}


@pytest.fixture(scope="module", autouse=True)
def shared_references():
    """the references are computed once and shared among the tests; they go when the module is done"""
    yield
    _references.clear()


def oracle_index(orc, key, v, cfg, levels):
    """(bytes, csr) of the oracle's build of all rows under the reference rule (once per key, never changed)"""
    if key not in _references:
        _references[key] = reference_bytes(orc, v, cfg, levels)
    return _references[key]


def definition_index(orc, key, v, cfg, levels=None, alpha=1.0, keep_pruned=True):
    """... of tests/_diverse_ref.py's build under the diverse rule"""
    if key not in _references:
        csr = dref.build(orc, v, cfg.m0, cfg.ef_construction, int(cfg.metric), alpha, keep_pruned, levels)
        _references[key] = csr_bytes(csr, cfg, v.shape[1]), csr
    return _references[key]


def split_build(v, cfg, n0, levels=None, **kw):
    lv = (None, None) if levels is None else (levels[:n0], levels[n0:])
    idx = ia.LeannIndex.build(v[:n0], cfg, levels=lv[0], batch=1, **kw)
    kw.setdefault("select", "reference")
    assert idx.insert(v[n0:], levels=lv[1], **kw) == n0
    return idx


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def state(idx, q, k=5, ef=30):
    """bytes and answers of a handle; a search that fails is recorded by the kind of its error"""
    try:
        ids, dist, cnt = idx.search_batch(q, k, ef)
        answers = (ids.tolist(), bits(dist).tolist(), cnt.tolist())
    except ia.CoreError as e:
        answers = e.kind
    return idx.to_bytes(), len(idx), answers


def base_rows():
    return clustered_vectors(600, 24, 7), random_levels(600, 8, 3)


def base_cfg(metric=ia.DistanceMetric.Cosine):
    return ia.LeannConfig(m=8, m0=16, ef_construction=40, metric=metric)


# ---------------------------------------------------------------- the split build is the oracle's build
@pytest.mark.parametrize("n0", [1, 20, 333])
@pytest.mark.parametrize("metric", METRICS)
def test_split_build_is_the_oracle(orc, metric, n0):
    v, lv = base_rows()
    cfg = base_cfg(metric)
    want, csr = oracle_index(orc, ("base", int(metric)), v, cfg, lv)
    idx = split_build(v, cfg, n0, lv)
    assert len(idx) == 600 and idx.entry_point == csr.entry_point and idx.dimension() == 24
    assert idx.to_bytes() == want
    # the grown index searches like the oracle's: padded adjacency, pool and lanes belong to the grown graph
    same_answers(orc, idx, csr, v, clustered_vectors(24, 24, 99), 10, 50, metric)


def test_several_inserts_in_a_row(orc):
    v, lv = base_rows()
    cfg = base_cfg(ia.DistanceMetric.Euclidean)
    want, _ = oracle_index(orc, ("base", 1), v, cfg, lv)
    idx = ia.LeannIndex.build(v[:100], cfg, levels=lv[:100], batch=1)
    for i in range(100, 105):
        assert idx.insert(v[i], levels=lv[i:i + 1]) == i and len(idx) == i + 1
    assert idx.insert(v[105:305], levels=lv[105:305]) == 105
    assert idx.insert(v[305:], levels=lv[305:]) == 305
    one_call = ia.LeannIndex.build(v, cfg, levels=lv, batch=1)
    assert idx.to_bytes() == one_call.to_bytes() == want


# ---------------------------------------------------------------- levels
def test_a_new_node_above_max_level_becomes_the_entry_point(orc):
    v = uniform_vectors(300, 16, 9)
    lv = np.zeros(300, np.uint64)
    lv[5], lv[250], lv[251], lv[260] = 1, 4, 4, 2
    cfg = base_cfg()
    want, csr = oracle_index(orc, "top", v, cfg, lv)
    idx = ia.LeannIndex.build(v[:200], cfg, levels=lv[:200], batch=1)
    assert idx.entry_point == 5
    assert idx.insert(v[200:], levels=lv[200:]) == 200
    # node 250 rose above max_level 1 and nodes 251.. searched from it: the lists are the oracle's
    assert idx.entry_point == 250 == csr.entry_point and idx.to_bytes() == want
    same_answers(orc, idx, csr, v, uniform_vectors(8, 16, 10), 5, 30)


@pytest.mark.parametrize("built_with", [False, True])
def test_levels_on_one_side_only(built_with):
    v, lv = base_rows()
    v, lv, n0 = v[:300], lv[:300].copy(), 180
    lv[7], lv[200] = 9, 12
    cfg = base_cfg()
    zeros = np.zeros(300, np.uint64)
    if built_with:  # built with levels, grown without
        idx = ia.LeannIndex.build(v[:n0], cfg, levels=lv[:n0], batch=1)
        assert idx.insert(v[n0:]) == n0
        whole = np.concatenate([lv[:n0], zeros[n0:]])
        assert idx.entry_point == 7
    else:  # built without levels, grown with
        idx = ia.LeannIndex.build(v[:n0], cfg, batch=1)
        assert idx.insert(v[n0:], levels=lv[n0:]) == n0
        whole = np.concatenate([zeros[:n0], lv[n0:]])
        assert idx.entry_point == 200
    assert idx.to_bytes() == ia.LeannIndex.build(v, cfg, levels=whole, batch=1).to_bytes()


# ---------------------------------------------------------------- the reference rule's variants
@pytest.mark.parametrize("hub_percentile,high_degree", [(0.02, True), (0.25, True), (0.02, False)])
def test_hub_rule_variants(orc, hub_percentile, high_degree):
    v = uniform_vectors(700, 16, 11)
    cfg = ia.LeannConfig(m=6, m0=12, ef_construction=48, hub_percentile=hub_percentile,
                         high_degree_pruning=high_degree)
    want, csr = oracle_index(orc, ("hub", hub_percentile, high_degree), v, cfg, None)
    idx = split_build(v, cfg, 350)
    assert idx.to_bytes() == want
    same_answers(orc, idx, csr, v, uniform_vectors(12, 16, 12), 5, 30)


def test_duplicated_rows(orc):
    """equal rows tie everywhere: the heap-exact kernel decides construction searches"""
    base = uniform_vectors(150, 32, 5)
    v = np.concatenate([base, base[:60]]).astype(np.float32)
    cfg = ia.LeannConfig.paper_default()
    want, _ = oracle_index(orc, "ties", v, cfg, None)
    assert split_build(v, cfg, 100).to_bytes() == want


def test_wide_rows(orc):
    v, lv = uniform_vectors(400, 12, 159), random_levels(400, 64, 5)
    cfg = ia.LeannConfig.accurate()
    cfg.m, cfg.m0, cfg.ef_construction = 64, 128, 256
    want, _ = oracle_index(orc, "wide", v, cfg, lv)
    idx = ia.LeannIndex.build(v[:200], cfg, levels=lv[:200], batch=1)
    assert max(len(idx.get_neighbors(i)) for i in range(200)) > 64  # imported rows of more than one slice
    assert idx.insert(v[200:], levels=lv[200:]) == 200
    assert idx.to_bytes() == want


def test_d768(orc):
    v, lv = clustered_vectors(400, 768, 5), random_levels(400, 8, 8)
    cfg = base_cfg()
    want, _ = oracle_index(orc, "d768", v, cfg, lv)
    assert split_build(v, cfg, 250, lv).to_bytes() == want


# ---------------------------------------------------------------- diverse rule
@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("alpha", [1.0, 1.2])
@pytest.mark.parametrize("rows", [("uniform", 0), ("clustered", 1)])
def test_diverse_rule_is_the_definition(orc, rows, alpha, keep):
    kind, metric = rows
    v = uniform_vectors(500, 24, 7) if kind == "uniform" else clustered_vectors(500, 24, 7)
    lv = random_levels(500, 8, 4)
    cfg = base_cfg(ia.DistanceMetric(metric))
    want, csr = definition_index(orc, ("diverse", kind, alpha, keep), v, cfg, lv, alpha, keep)
    idx = split_build(v, cfg, 300, lv, select="diverse", alpha=alpha, keep_pruned=keep)
    assert idx.entry_point == csr.entry_point and idx.to_bytes() == want


# ---------------------------------------------------------------- bf16 rows
@pytest.mark.parametrize("d", [3, 100, 768])
@pytest.mark.parametrize("select", ["reference", "diverse"])
def test_bf16(orc, select, d):
    n, n0 = 200, 120
    rows_bits = to_bf16_bits(uniform_vectors(n, d, 50 + d) if d == 3 else clustered_vectors(n, d, 50 + d))
    rows = widen(rows_bits)
    cfg = base_cfg()
    if select == "reference":
        want, csr = oracle_index(orc, ("bf16", d), rows, cfg, None)
    else:
        want, csr = definition_index(orc, ("bf16-diverse", d), rows, cfg)
    idx = ia.LeannIndex.build_bf16(rows_bits[:n0], cfg, batch=1, select=select)
    assert idx.insert_bf16(rows_bits[n0:], select=select) == n0
    assert idx.to_bytes() == want == ia.LeannIndex.build_bf16(rows_bits, cfg, batch=1, select=select).to_bytes()
    # the grown index keeps bf16 rows (isl_select_neighbors takes float32 rows alone) and answers over them
    with pytest.raises(ia.CoreError) as ex:
        idx.select_neighbors([3], [[1, 2]], 2)
    assert ex.value.kind == "Unsupported"
    same_answers(orc, idx, csr, rows, uniform_vectors(10, d, 12), 5, 30)
    same_answers(orc, idx, csr, rows, widen(to_bf16_bits(uniform_vectors(10, d, 13))), 5, 30)


def test_the_stored_type_is_the_only_one_taken():
    n, d = 150, 24
    v = clustered_vectors(n, d, 3)
    rows_bits = to_bf16_bits(v)
    cfg = base_cfg()
    q = clustered_vectors(6, d, 4)
    for idx, wrong in ((ia.LeannIndex.build_bf16(rows_bits[:100], cfg), lambda i: i.insert(v[100:])),
                       (ia.LeannIndex.build(v[:100], cfg), lambda i: i.insert_bf16(rows_bits[100:]))):
        before = state(idx, q)
        with pytest.raises(ia.CoreError) as ex:
            wrong(idx)
        assert ex.value.kind == "Unsupported" and "rows" in str(ex.value)
        assert state(idx, q) == before


# ---------------------------------------------------------------- what the handle carries besides the graph
def test_heap_exact_kernel_before_and_after_growth(orc):
    """ef 600 is above 512: the heap-exact kernel answers from its pool, whose visited bitmap and candidate heap
    are sized by the node count.  A pool of the 64-node graph under the 600-node one would be written past its
    end; the insert frees it and the next search makes it again."""
    v = uniform_vectors(600, 16, 41)
    cfg = base_cfg(ia.DistanceMetric.Euclidean)
    want, csr = oracle_index(orc, "exact", v, cfg, None)
    _, small = oracle_index(orc, "exact-64", v[:64], cfg, None)
    q = uniform_vectors(8, 16, 42)
    idx = ia.LeannIndex.build(v[:64], cfg, batch=1)
    same_answers(orc, idx, small, v[:64], q, 10, 600, 1)
    assert idx.last_stats()["exact_path"] > 0
    assert idx.insert(v[64:]) == 64
    assert idx.to_bytes() == want
    same_answers(orc, idx, csr, v, q, 10, 600, 1)
    assert idx.last_stats()["exact_path"] > 0
    same_answers(orc, idx, csr, v, q, 10, 50, 1)


def test_prepare_then_insert_then_search(orc):
    v, lv = base_rows()
    cfg = base_cfg()
    want, csr = oracle_index(orc, ("base", 0), v, cfg, lv)
    idx = ia.LeannIndex.build(v[:333], cfg, levels=lv[:333], batch=1)
    idx.prepare(32, 64, 10, lanes=2)
    q = clustered_vectors(24, 24, 99)
    idx.search_batch(q, 10, 50)
    assert idx.insert(v[333:], levels=lv[333:]) == 333
    same_answers(orc, idx, csr, v, q, 10, 50)  # on the lanes prepared before the insert
    same_answers(orc, idx, csr, v, q[:5], 10, 600)
    assert idx.to_bytes() == want


def test_entry_seeds_survive(orc):
    v, lv = base_rows()
    metric = ia.DistanceMetric.Euclidean
    cfg = base_cfg(metric)
    _, csr = oracle_index(orc, ("base", 1), v, cfg, lv)
    idx = ia.LeannIndex.build(v[:400], cfg, levels=lv[:400], batch=1)
    seeds = idx.select_entry_seeds(8).tolist()
    assert len(seeds) == 8 and seeds == sref.select(orc, 1, v[:400], idx.entry_point, 8)
    assert idx.insert(v[400:], levels=lv[400:]) == 400
    assert idx.entry_seeds().tolist() == seeds  # kept as they are, not re-selected
    # a plain search is the reference search over the grown graph entered at the nearest seed
    assert_seeded_search(orc, idx, csr, v, clustered_vectors(16, 24, 98), 10, 50, metric)


def test_pq_codes_are_detached(orc):
    from test_gpu_two_level import attach_pq
    from test_two_level_cpu import make_pq
    v = clustered_vectors(250, 16, 61, per_cluster=10)
    cfg = base_cfg(ia.DistanceMetric.Euclidean)
    _, csr = oracle_index(orc, "pq", v, cfg, None)
    cb, codes = make_pq(v[:200], 4, 8, 10)
    idx = ia.LeannIndex.build(v[:200], cfg, batch=1)
    bare = ia.LeannIndex.build(v[:200], cfg, batch=1)
    q = v[:3]
    with pytest.raises(ia.CoreError) as never:
        bare.search_two_level_batch(q, 3, 8, 0.5)
    pq = attach_pq(idx, cb, codes)
    assert idx.search_two_level_batch(q, 3, 8, 0.5)[2].tolist() == [3, 3, 3]
    assert idx.insert(v[200:]) == 200
    with pytest.raises(ia.CoreError) as after:  # the codes no longer cover every node: gone with the insert
        idx.search_two_level_batch(q, 3, 8, 0.5)
    assert after.value.kind == never.value.kind == "PQError" and str(after.value) == str(never.value)
    same_answers(orc, idx, csr, v, q, 3, 8, 1)
    del pq


# ---------------------------------------------------------------- onto indexes not built here
def prefix_and_whole(orc, n0=333):
    v, lv = base_rows()
    cfg = base_cfg()
    whole, _ = oracle_index(orc, ("base", 0), v, cfg, lv)
    part, csr = oracle_index(orc, ("base-prefix", n0), v[:n0], cfg, lv[:n0])
    return v, lv, cfg, part, csr, whole


def test_onto_an_index_from_csr(orc):
    n0 = 333
    v, lv, cfg, _, csr, whole = prefix_and_whole(orc, n0)
    g = ia.CsrGraph(node_offsets=csr.node_offsets, neighbors=csr.neighbors, levels=csr.levels,
                    entry_point=csr.entry_point, max_level=csr.max_level, num_nodes=csr.num_nodes,
                    degree_counts=csr.degree_counts)
    idx = ia.LeannIndex.from_csr(g, cfg, dimension=24).upload(0).set_embeddings(v[:n0])
    assert idx.insert(v[n0:], levels=lv[n0:]) == n0
    assert idx.to_bytes() == whole


def test_onto_an_index_from_bytes(orc):
    n0 = 333
    v, lv, cfg, part, _, whole = prefix_and_whole(orc, n0)
    idx = ia.LeannIndex.from_bytes(part).upload(0).set_embeddings(v[:n0])
    assert idx.insert(v[n0:], levels=lv[n0:]) == n0
    assert idx.to_bytes() == whole


def test_onto_a_loaded_index(orc, tmp_path):
    n0 = 333
    v, lv, cfg, part, _, whole = prefix_and_whole(orc, n0)
    path = os.path.join(str(tmp_path), "prefix.idx")
    ia.LeannIndex.from_bytes(part).save(path)
    idx, _ = ia.LeannIndex.load(path)
    idx.upload(0).set_embeddings(v[:n0])
    assert idx.insert(v[n0:], levels=lv[n0:]) == n0
    assert idx.to_bytes() == whole


def test_device_rows():
    torch = pytest.importorskip("torch")
    v, lv = base_rows()
    cfg = base_cfg()
    n0 = 333
    for select in ("reference", "diverse"):
        blob = ia.LeannIndex.build(v, cfg, levels=lv, batch=1, select=select).to_bytes()
        idx = ia.LeannIndex.build(v[:n0], cfg, levels=lv[:n0], batch=1, select=select)
        t = torch.from_numpy(v[n0:]).to("cuda:0")
        torch.cuda.synchronize()
        assert idx.insert(t, levels=lv[n0:], select=select) == n0
        del t  # the index keeps its own copy of the rows
        assert idx.to_bytes() == blob
    rows_bits = to_bf16_bits(v)
    blob = ia.LeannIndex.build_bf16(rows_bits, cfg, batch=1).to_bytes()
    idx = ia.LeannIndex.build_bf16(rows_bits[:n0], cfg, batch=1)
    t = torch.from_numpy(rows_bits[n0:].view(np.int16)).to("cuda:0")
    torch.cuda.synchronize()
    assert idx.insert_bf16(t) == n0 and idx.to_bytes() == blob


@pytest.mark.parametrize("n", [1, 150])
def test_insert_into_the_empty_index(n):
    v, lv = uniform_vectors(n, 16, 4), random_levels(n, 8, 9)
    cfg = base_cfg(ia.DistanceMetric.DotProduct)
    idx = ia.LeannIndex(cfg)
    assert idx.is_empty() and idx.insert(v, levels=lv) == 0
    assert len(idx) == n and idx.to_bytes() == ia.LeannIndex.build(v, cfg, levels=lv, batch=1).to_bytes()
    assert idx.search(v[n - 1], 1)[0][0] == n - 1
    bf = ia.LeannIndex(cfg)
    assert bf.insert_bf16(to_bf16_bits(v), levels=lv) == 0
    assert bf.to_bytes() == ia.LeannIndex.build_bf16(to_bf16_bits(v), cfg, levels=lv, batch=1).to_bytes()


# ---------------------------------------------------------------- failures
def test_failure_leaves_the_index_as_it_was():
    v, lv = uniform_vectors(300, 16, 6), random_levels(300, 8, 2)
    cfg = base_cfg()
    idx = ia.LeannIndex.build(v[:200], cfg, levels=lv[:200], batch=1)
    q = uniform_vectors(16, 16, 8)
    before = state(idx, q, 10, 40)
    with pytest.raises(ia.CoreError) as e:
        idx.insert(uniform_vectors(100, 12, 6))
    assert e.value.kind == "DimensionMismatch" and (e.value.expected, e.value.actual) == (16, 12)
    assert state(idx, q, 10, 40) == before
    for kw, kind in ((dict(select=7), "InvalidArgument"), (dict(select="diverse", alpha=0.5), "InvalidConfig")):
        with pytest.raises(ia.CoreError) as e:
            idx.insert(v[200:], levels=lv[200:], **kw)
        assert e.value.kind == kind
        assert state(idx, q, 10, 40) == before
    with pytest.raises(ia.CoreError) as e:  # refused after every argument check: the stored type
        idx.insert_bf16(to_bf16_bits(v[200:]), levels=lv[200:])
    assert e.value.kind == "Unsupported" and state(idx, q, 10, 40) == before
    assert idx.insert(v[200:], levels=lv[200:]) == 200  # and it still grows
    assert idx.to_bytes() == ia.LeannIndex.build(v, cfg, levels=lv, batch=1).to_bytes()


REFUSED_IMAGES = [("a list longer than m0", list(range(1, 10)), "longer than"),
                  ("an id twice in a list", [1, 1, 2], "verbatim"),
                  ("an id that is not below len", [1, 12], "not below")]


@pytest.mark.parametrize("what,list_of_0,words", REFUSED_IMAGES, ids=[c[0] for c in REFUSED_IMAGES])
def test_images_the_table_cannot_hold_are_refused(what, list_of_0, words):
    """from_csr and upload accept these lists; the builder's table cannot take them over.  Each is refused by a
    message that says which, after the import kernel has looked, and the handle is as it was."""
    n = 12
    v = uniform_vectors(n, 4, 2)
    lists = [[(i + 1) % n, (i + 2) % n] for i in range(n)]
    lists[0] = list_of_0
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in lists])
    g = ia.CsrGraph(node_offsets=off, neighbors=np.array([x for r in lists for x in r], np.uint64),
                    levels=np.zeros(n, np.uint64), entry_point=0, num_nodes=n,
                    degree_counts=np.diff(off.astype(np.int64)).astype(np.uint64))
    cfg = ia.LeannConfig(m=4, m0=8, ef_construction=16, metric=ia.DistanceMetric.Euclidean)
    idx = ia.LeannIndex.from_csr(g, cfg, dimension=4).upload(0).set_embeddings(v)
    q = uniform_vectors(4, 4, 8)
    before = state(idx, q, 5, 12)
    with pytest.raises(ia.CoreError) as e:
        idx.insert(uniform_vectors(3, 4, 5))
    assert e.value.kind == "Unsupported" and words in str(e.value), str(e.value)
    assert state(idx, q, 5, 12) == before and len(idx) == n


def test_the_core_of_an_hnsw_graph_is_refused():
    v = uniform_vectors(60, 8, 3)
    g = ia.HnswGraph.build(v, m=4, m0=8, ef_construction=16)
    blob = g.to_bytes()
    core = C.c_void_p.from_address(g._h.value)  # isl_hnsw's first member: the layer-0 isl_index
    first = C.c_uint64(77)
    st = ia._ffi.lib().isl_index_insert(core, None, v.ctypes.data_as(C.c_void_p), 0, 4, 8, None, 0, C.byref(first))
    assert ia._ffi.lib().isl_status_name(st).decode() == "Unsupported"
    assert "isl_hnsw_insert" in ia._ffi.lib().isl_last_error_message().decode()
    assert first.value == 77 and g.to_bytes() == blob and len(g) == 60


def test_a_recompute_index_is_refused(orc):
    from test_gpu_encoder import _recompute_case
    _, enc, tok, lens, emb = _recompute_case(orc, n=64)
    n, d = emb.shape
    ring = ia.CsrGraph(node_offsets=np.arange(n + 1, dtype=np.uint64),
                       neighbors=(np.arange(n, dtype=np.uint64) + 1) % n, levels=np.zeros(n, np.uint64),
                       entry_point=0, num_nodes=n, degree_counts=np.ones(n, np.uint64))
    idx = ia.LeannIndex.from_csr(ring, base_cfg(), dimension=d).upload(0)
    idx.set_recompute_provider(enc, tok, lens)
    blob = idx.to_bytes()
    with pytest.raises(ia.CoreError) as e:
        idx.insert(emb[:4])
    assert e.value.kind == "Unsupported" and "recompute" in str(e.value)
    assert idx.to_bytes() == blob and len(idx) == n
    assert len(idx.search(emb[5], 1)) == 1  # and it still answers


# ---------------------------------------------------------------- batched mode
def no_inbound(rows):
    seen = set()
    for r in rows:
        seen.update(r)
    return len(rows) - len(seen)


@pytest.mark.parametrize("kind", ["uniform", "clustered"])
@pytest.mark.parametrize("rule", ["reference", "diverse"])
def test_batched_insert(kind, rule):
    """The split batched build under the invariants of test_batched_build_keeps_the_invariants and, for the
    diverse rule, the caps of test_gpu_hnsw_insert.py::test_batched_insert; the one-call batched build of the
    same rows is held to the same caps first."""
    n, n0, d = 3000, 2000, 16
    v = uniform_vectors(n, d, 21) if kind == "uniform" else clustered_vectors(n, d, 21)
    cfg = ia.LeannConfig(m=8, m0=16, ef_construction=64, metric=ia.DistanceMetric(0 if kind == "uniform" else 1))
    probes = list(range(0, n, 30))

    def check(idx, what):
        assert len(idx) == n and idx.dimension() == d and idx.entry_point == 0
        rows = [idx.get_neighbors(i).tolist() for i in range(n)]
        degs = np.array([len(r) for r in rows])
        assert degs.max() <= 16 and degs[1:].min() >= 1
        for i, r in enumerate(rows):
            assert len(set(r)) == len(r) and i not in r and all(x < n for x in r)
        if rule == "diverse":
            lost = no_inbound(rows)
            ids, _, cnt = idx.search_batch(v[probes], 1, 64)
            hits = int(sum(1 for j, i in enumerate(probes) if cnt[j] and ids[j, 0] == i))
            print(f"{kind}: {what}, nodes without an inbound edge {lost} of {n}; self-query recall@1 "
                  f"{hits}/{len(probes)}")
            assert lost <= 0.01 * n
            assert hits >= 0.95 * len(probes)

    check(ia.LeannIndex.build(v, cfg, batch=256, select=rule), "one-call batched build")
    idx = ia.LeannIndex.build(v[:n0], cfg, batch=256, select=rule)
    assert idx.insert(v[n0:], batch=256, select=rule) == n0
    check(idx, "split batched build")
