"""isl_index_remove on the device: rows removed from a built LeannIndex, in place.  After each case the bytes of
the handle equal those of tests/_remove_ref.py's graph (the definition restated in Python over the graph the
handle held before, distances through the oracle), through LeannIndex.from_csr(...).to_bytes() as in
test_gpu_build*.py, the remap equals the definition's, and a few queries answer as the oracle's search of that
graph over the survivors' rows.  Then what the handle carries besides the graph: the prepared lanes, the
heap-exact kernel's pool, the entry seeds, the PQ codes.  Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import islands_amd as ia
import _remove_ref as rref
from _data import clustered_vectors, random_levels, uniform_vectors
from test_gpu_build_bf16 import csr_bytes, same_answers, to_bf16_bits, widen
from test_gpu_entry_seeds import assert_seeded_search
from test_gpu_index_insert import state

pytestmark = pytest.mark.gpu

METRICS = [ia.DistanceMetric.Cosine, ia.DistanceMetric.Euclidean, ia.DistanceMetric.DotProduct,
           ia.DistanceMetric.Manhattan]
REMOVED = rref.REMOVED

_built = {}


@pytest.fixture(scope="module", autouse=True)
def shared_builds():
    """the starting graphs are built once and shared among the tests; they go when the module is done"""
    yield
    _built.clear()


def base_cfg(metric=ia.DistanceMetric.Cosine, **kw):
    cfg = dict(m=4, m0=8, ef_construction=40, metric=metric)
    cfg.update(kw)
    return ia.LeannConfig(**cfg)


def base_rows():
    return clustered_vectors(600, 16, 7), random_levels(600, 8, 3)


def csr_of(orc, idx, levels=None):
    """the graph a handle holds, as an oracle Csr (lists in their stored order)"""
    n = len(idx)
    rows = [idx.get_neighbors(i).tolist() for i in range(n)]
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    g = orc.Csr(off, np.array([x for r in rows for x in r], np.uint64), idx.entry_point)
    if levels is not None:
        g.levels = np.asarray(levels, np.uint64).copy()
    g.max_level = int(ia._ffi.lib().isl_index_max_level(idx._h))
    return g


def fresh(orc, key, v, cfg, levels=None, rule="reference", bf16=False, **kw):
    """(index, its graph): built on the device the first time, from its bytes + upload + rows afterwards"""
    if key not in _built:
        if bf16:
            idx = ia.LeannIndex.build_bf16(v, cfg, levels=levels, batch=1, select=rule, **kw)
        else:
            idx = ia.LeannIndex.build(v, cfg, levels=levels, batch=1, select=rule, **kw)
        _built[key] = idx.to_bytes(), csr_of(orc, idx, levels)
        return idx, _built[key][1]
    blob, csr = _built[key]
    idx = ia.LeannIndex.from_bytes(blob).upload(0)
    idx.set_embeddings_bf16(v) if bf16 else idx.set_embeddings(v)
    return idx, csr


def pick_ids(n, count, seed):
    return np.random.default_rng(seed).choice(n, count, replace=False).astype(np.uint64)


def remove_and_check(orc, idx, csr, v, ids, cfg, rule="reference", alpha=1.0, keep=True, q=None, stats=None):
    """remove `ids` from `idx`, whose graph is `csr` over rows `v` (f32 images): remap, bytes and answers are the
    definition's.  Returns (the definition's graph, the survivors' rows, the remap)."""
    metric = ia.DistanceMetric(int(cfg.metric))
    want, remap = rref.remove(orc, csr, v, ids, cfg.m0, int(metric), rule, alpha, keep, stats)
    got = idx.remove(ids, select=rule, alpha=alpha, keep_pruned=keep)
    assert got.dtype == np.uint64 and got.tolist() == remap.tolist()
    rows = np.ascontiguousarray(v[remap != REMOVED])
    assert len(idx) == want.num_nodes == rows.shape[0] and idx.entry_point == want.entry_point
    assert idx.dimension() == v.shape[1]
    assert idx.to_bytes() == csr_bytes(want, cfg, v.shape[1])
    if q is None:
        q = uniform_vectors(6, v.shape[1], 99)
    same_answers(orc, idx, want, rows, q, 5, 30, metric)
    return want, rows, remap


# ---------------------------------------------------------------- the definition, byte for byte
@pytest.mark.parametrize("count", [1, 20, 333])
@pytest.mark.parametrize("rule", ["reference", "diverse"])
@pytest.mark.parametrize("metric", METRICS)
def test_remove_is_the_definition(orc, metric, rule, count):
    v, lv = base_rows()
    cfg = base_cfg(metric)
    idx, csr = fresh(orc, ("base", int(metric), rule), v, cfg, lv, rule)
    stats = []
    # (one id: one that some list names -- a node may have lost every inbound edge during the build)
    ids = pick_ids(600, count, count) if count > 1 else [int(csr.neighbors[0])]
    remove_and_check(orc, idx, csr, v, ids, cfg, rule, stats=stats)
    assert stats  # some list named a removed id
    if count == 333:
        assert max(c for _, c in stats) > cfg.m0  # lists outgrew m0: distances, the sort and the rule ran


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("alpha", [1.0, 1.2])
@pytest.mark.parametrize("kind", ["uniform", "clustered"])
def test_diverse_rule_variants(orc, kind, alpha, keep):
    v = uniform_vectors(600, 16, 7) if kind == "uniform" else clustered_vectors(600, 16, 7)
    cfg = base_cfg(ia.DistanceMetric.Euclidean if kind == "clustered" else ia.DistanceMetric.Cosine)
    idx, csr = fresh(orc, ("variants", kind, alpha, keep), v, cfg, None, "diverse", alpha=alpha, keep_pruned=keep)
    stats = []
    remove_and_check(orc, idx, csr, v, pick_ids(600, 250, 5), cfg, "diverse", alpha, keep, stats=stats)
    assert max(c for _, c in stats) > cfg.m0


@pytest.mark.parametrize("rule", ["reference", "diverse"])
@pytest.mark.parametrize("metric", [ia.DistanceMetric.Cosine, ia.DistanceMetric.Manhattan])
def test_quantised_and_duplicated_rows(orc, metric, rule):
    """four values per element and every row three times: equal distances everywhere, finite values only"""
    u = uniform_vectors(100, 6, 31)
    base = (np.sign(u) * np.where(np.abs(u) > 0.5, 1.0, 0.5)).astype(np.float32)
    assert np.all(base != 0)
    v = np.concatenate([base, base, base[::-1]]).astype(np.float32)
    cfg = base_cfg(metric)
    idx, csr = fresh(orc, ("ties", int(metric), rule), v, cfg, None, rule)
    stats = []
    remove_and_check(orc, idx, csr, v, pick_ids(300, 140, 8), cfg, rule, q=v[:6] * 0.75, stats=stats)
    assert max(c for _, c in stats) > cfg.m0


@pytest.mark.parametrize("rule", ["reference", "diverse"])
def test_wide_rows(orc, rule):
    """m0 = 96: lists and candidate lists past 64 ids, more than one slice everywhere"""
    v = uniform_vectors(400, 12, 159)
    cfg = base_cfg(ia.DistanceMetric.Euclidean, m=48, m0=96, ef_construction=128)
    idx, csr = fresh(orc, ("wide", rule), v, cfg, None, rule)
    assert max(len(r) for r in rref.lists_of(csr)) > 64
    stats = []
    remove_and_check(orc, idx, csr, v, pick_ids(400, 150, 3), cfg, rule, stats=stats)
    assert max(c for _, c in stats) > 96


@pytest.mark.parametrize("rule", ["reference", "diverse"])
def test_d768(orc, rule):
    v = clustered_vectors(300, 768, 5)
    cfg = base_cfg()
    idx, csr = fresh(orc, ("d768", rule), v, cfg, None, rule)
    remove_and_check(orc, idx, csr, v, pick_ids(300, 160, 4), cfg, rule)


@pytest.mark.parametrize("d", [3, 100, 768])
@pytest.mark.parametrize("rule", ["reference", "diverse"])
def test_bf16(orc, rule, d):
    n = 200
    rows_bits = to_bf16_bits(uniform_vectors(n, d, 50 + d) if d == 3 else clustered_vectors(n, d, 50 + d))
    v = widen(rows_bits)
    cfg = base_cfg()
    idx, csr = fresh(orc, ("bf16", d, rule), rows_bits, cfg, None, rule, bf16=True)
    want, rows, remap = remove_and_check(orc, idx, csr, v, pick_ids(n, 110, d), cfg, rule)
    # the rows afterwards are the survivors' bits: queries that are bf16 values answer over them bit for bit, the
    # index still takes bf16 rows alone, and a float32-only call still refuses it
    same_answers(orc, idx, want, rows, widen(to_bf16_bits(uniform_vectors(8, d, 13))), 5, 30)
    with pytest.raises(ia.CoreError) as ex:
        idx.select_neighbors([1], [[0, 2]], 2)
    assert ex.value.kind == "Unsupported"
    with pytest.raises(ia.CoreError) as ex:
        idx.insert(v[:3])
    assert ex.value.kind == "Unsupported"
    assert idx.insert_bf16(rows_bits[:3]) == 90
    # ... and equal the rows of an index given the survivors' bits directly
    twin = ia.LeannIndex.from_bytes(csr_bytes(want, cfg, d)).upload(0).set_embeddings_bf16(rows_bits[remap != REMOVED])
    assert twin.insert_bf16(rows_bits[:3]) == 90 and twin.to_bytes() == idx.to_bytes()


# ---------------------------------------------------------------- graphs made for one property
def index_from_lists(lists, v, cfg, entry=0, levels=None, max_level=0):
    n = len(lists)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in lists])
    g = ia.CsrGraph(node_offsets=off, neighbors=np.array([x for r in lists for x in r], np.uint64),
                    levels=np.zeros(n, np.uint64) if levels is None else np.asarray(levels, np.uint64),
                    entry_point=entry, max_level=max_level, num_nodes=n,
                    degree_counts=np.diff(off.astype(np.int64)).astype(np.uint64))
    return ia.LeannIndex.from_csr(g, cfg, dimension=v.shape[1]).upload(0).set_embeddings(v)


@pytest.mark.parametrize("rule", ["reference", "diverse"])
def test_candidate_cap(orc, rule):
    """Node 0's 32 neighbours each list 32 ids nobody else lists; all 32 go.  C(0) passes 512 distinct ids and is
    cut there: the ids of the last 16 neighbours never become candidates, however near they are."""
    n, m0 = 1200, 32
    v = uniform_vectors(n, 8, 77)
    v[33 + 16 * 32:33 + 32 * 32] = v[0] + 1e-3 * v[33 + 16 * 32:33 + 32 * 32]  # past the cut, and nearest to node 0
    lists = [[] for _ in range(n)]
    lists[0] = list(range(1, 33))
    for i in range(1, 33):
        lists[i] = list(range(33 + (i - 1) * 32, 33 + i * 32))
    for j in range(33, n):
        lists[j] = [0]
    cfg = base_cfg(ia.DistanceMetric.Euclidean, m=16, m0=m0)
    idx = index_from_lists(lists, v, cfg)
    stats = []
    want, _, remap = remove_and_check(orc, idx, csr_of(orc, idx), v, np.arange(1, 33, dtype=np.uint64), cfg, rule,
                                      stats=stats)
    assert stats == [(0, 512)]
    got = idx.get_neighbors(0).tolist()
    assert len(got) == m0 and all(remap[33] <= x < remap[33 + 16 * 32] for x in got)


def reachable(rows, entry):
    seen, todo = {entry}, [entry]
    while todo:
        for y in rows[todo.pop()]:
            if y not in seen:
                seen.add(y)
                todo.append(y)
    return seen


@pytest.mark.parametrize("rule", ["reference", "diverse"])
def test_bridge(orc, rule):
    """Two groups joined only through node 10.  Dropping its edges leaves the second group unreachable; the repair
    hands its neighbours to each other."""
    a, x, b = list(range(10)), 10, list(range(11, 21))
    lists = [[] for _ in range(21)]
    for grp in (a, b):
        for i, p in enumerate(grp):
            lists[p] = [grp[(i + 1) % 10], grp[(i - 1) % 10]]
    lists[9].append(x)
    lists[11].append(x)
    lists[x] = [9, 11]
    dropped = [[y - (y > x) for y in r if y != x] for p, r in enumerate(lists) if p != x]
    assert reachable(dropped, 0) == set(range(10))  # merely dropping the edges loses the second group
    v = uniform_vectors(21, 4, 6)
    cfg = base_cfg(ia.DistanceMetric.Euclidean)
    idx = index_from_lists(lists, v, cfg)
    remove_and_check(orc, idx, csr_of(orc, idx), v, [x], cfg, rule)
    rows = [idx.get_neighbors(i).tolist() for i in range(len(idx))]
    assert reachable(rows, idx.entry_point) == set(range(20))
    assert 10 in rows[9] and 9 in rows[10]  # old 9 <-> old 11


# ---------------------------------------------------------------- structure
def test_remove_the_entry_point(orc):
    v, _ = base_rows()
    v = v[:300]
    lv = np.zeros(300, np.uint64)
    lv[40], lv[17], lv[120], lv[250], lv[3] = 6, 4, 4, 4, 2
    cfg = base_cfg()
    idx, csr = fresh(orc, "entry", v, cfg, lv)
    assert idx.entry_point == 40 and csr.max_level == 6
    want, rows, remap = remove_and_check(orc, idx, csr, v, [40, 17, 5], cfg)
    # 17 went with it: of the survivors at level 4 the lowest new id takes over
    assert idx.entry_point == int(remap[120]) == 117 and want.max_level == 4
    # a surviving entry point is kept, remapped, with its level
    lv2 = want.levels
    want2, _, remap2 = remove_and_check(orc, idx, want, rows, [0, 1, int(remap[250])], cfg)
    assert idx.entry_point == 115 and want2.max_level == 4 and want2.levels.tolist() == np.delete(lv2, [0, 1, 247]).tolist()


def test_all_but_one_then_all_then_insert(orc):
    v, lv = base_rows()
    v, lv = v[:120], lv[:120]
    cfg = base_cfg(ia.DistanceMetric.DotProduct)
    idx, csr = fresh(orc, "all", v, cfg, lv, "diverse")
    ids = np.delete(np.arange(120, dtype=np.uint64), 77)
    want, rows, remap = remove_and_check(orc, idx, csr, v, ids, cfg, "diverse")
    assert len(idx) == 1 and remap[77] == 0 and idx.get_neighbors(0).tolist() == [] and idx.entry_point == 0
    assert idx.search(v[77], 3)[0][0] == 0
    # the last one: what a build of no rows gives under the handle's config
    assert idx.remove([0]).tolist() == [REMOVED]
    assert len(idx) == 0 and idx.is_empty() and idx.entry_point is None and idx.dimension() is None
    assert idx.to_bytes() == ia.LeannIndex(cfg).to_bytes() == ia.LeannIndex.build(v[:0].reshape(0, 16), cfg).to_bytes()
    with pytest.raises(ia.CoreError) as e:
        idx.remove([0])
    assert e.value.kind == "NodeNotFound"
    # and the emptied handle takes rows as an empty index does
    assert idx.insert(v[:60], levels=lv[:60]) == 0
    assert idx.to_bytes() == ia.LeannIndex.build(v[:60], cfg, levels=lv[:60], batch=1).to_bytes()
    assert idx.search(v[59], 1)[0][0] == 59
    # every node in one call
    idx2, _ = fresh(orc, "all", v, cfg, lv, "diverse")
    assert idx2.remove(np.arange(120)).tolist() == [REMOVED] * 120 and idx2.to_bytes() == ia.LeannIndex(cfg).to_bytes()


def test_a_survivor_whose_candidates_are_all_gone(orc):
    n = 12
    lists = [[(i - 3 + 1) % 9 + 3, (i - 3 - 1) % 9 + 3] for i in range(n)]  # nodes 3 .. 11: a ring of their own
    lists[0], lists[1], lists[2] = [1, 2], [0, 2], [0, 1]
    v = uniform_vectors(n, 4, 2)
    cfg = base_cfg(ia.DistanceMetric.Euclidean)
    idx = index_from_lists(lists, v, cfg)
    stats = []
    want, _, _ = remove_and_check(orc, idx, csr_of(orc, idx), v, [1, 2], cfg, stats=stats)
    assert stats == [(0, 0)] and idx.get_neighbors(0).tolist() == [] and want.entry_point == 0
    ids, _, cnt = idx.search_batch(v[5:6], 2, 8)
    assert cnt.tolist() == [1] and ids[0, 0] == 0  # the entry point leads nowhere: it is the only answer


def test_repeated_ids_and_no_remap(orc):
    v, lv = base_rows()
    cfg = base_cfg()
    ids = pick_ids(600, 50, 9)
    idx, csr = fresh(orc, ("base", 0, "reference"), v, cfg, lv)
    want, _, remap = remove_and_check(orc, idx, csr, v, np.concatenate([ids, ids[::-1], ids[:7]]), cfg)
    assert want.num_nodes == 550
    # out_remap and out_len may be NULL
    idx2, _ = fresh(orc, ("base", 0, "reference"), v, cfg, lv)
    st = ia._ffi.lib().isl_index_remove(idx2._h, None, ids.ctypes.data_as(C.c_void_p), ids.size, None, None)
    assert st == 0 and idx2.to_bytes() == idx.to_bytes()


# ---------------------------------------------------------------- composition
@pytest.mark.parametrize("rule", ["reference", "diverse"])
def test_remove_then_insert_continues_the_builders_loop(orc, rule):
    """insert with one node per step reads only the lists, the entry point and the rows: after a removal it must
    build what it builds on the definition's graph given as a CSR with the survivors' rows"""
    v, lv = base_rows()
    cfg = base_cfg(ia.DistanceMetric.Euclidean)
    idx, csr = fresh(orc, ("base", 1, rule), v, cfg, lv, rule)
    want, rows, _ = remove_and_check(orc, idx, csr, v, pick_ids(600, 200, 12), cfg, rule)
    more, more_lv = clustered_vectors(40, 16, 70), random_levels(40, 8, 71)
    assert idx.insert(more, levels=more_lv, select=rule) == 400
    g = ia.CsrGraph(node_offsets=want.node_offsets, neighbors=want.neighbors, levels=want.levels,
                    entry_point=want.entry_point, max_level=want.max_level, num_nodes=want.num_nodes,
                    degree_counts=want.degree_counts)
    twin = ia.LeannIndex.from_csr(g, cfg, dimension=16).upload(0).set_embeddings(rows)
    assert twin.insert(more, levels=more_lv, select=rule) == 400
    assert idx.to_bytes() == twin.to_bytes() and len(idx) == 440


def test_remove_twice_in_a_row(orc):
    v, lv = base_rows()
    cfg = base_cfg(ia.DistanceMetric.Manhattan)
    idx, csr = fresh(orc, ("base", 3, "diverse"), v, cfg, lv, "diverse")
    want, rows, _ = remove_and_check(orc, idx, csr, v, pick_ids(600, 150, 21), cfg, "diverse")
    want, rows, _ = remove_and_check(orc, idx, want, rows, pick_ids(450, 150, 22), cfg, "reference")
    remove_and_check(orc, idx, want, rows, pick_ids(300, 100, 23), cfg, "diverse")
    assert len(idx) == 200


def test_a_loaded_index(orc, tmp_path):
    v, lv = base_rows()
    cfg = base_cfg()
    built, csr = fresh(orc, ("base", 0, "reference"), v, cfg, lv)
    path = os.path.join(str(tmp_path), "base.idx")
    built.save(path)
    idx, _ = ia.LeannIndex.load(path)
    idx.upload(0).set_embeddings(v)
    remove_and_check(orc, idx, csr, v, pick_ids(600, 120, 31), cfg)
    again = ia.LeannIndex.from_bytes(built.to_bytes()).upload(0).set_embeddings(v)
    remove_and_check(orc, again, csr, v, pick_ids(600, 120, 31), cfg)


# ---------------------------------------------------------------- what the handle carries besides the graph
def test_prepare_search_remove_search(orc):
    v, lv = base_rows()
    cfg = base_cfg()
    idx, csr = fresh(orc, ("base", 0, "reference"), v, cfg, lv)
    idx.prepare(32, 64, 10, lanes=2)
    q = clustered_vectors(24, 16, 99)
    same_answers(orc, idx, csr, v, q, 10, 50)
    want, rows, _ = remove_and_check(orc, idx, csr, v, pick_ids(600, 300, 41), cfg, q=q)
    same_answers(orc, idx, want, rows, q, 10, 50)  # on the lanes prepared before the removal


def test_heap_exact_kernel_before_and_after(orc):
    """ef 600 is above 512: the heap-exact kernel answers from its pool, sized by the node count.  The removal
    frees it and the next search makes it again."""
    v, lv = base_rows()
    cfg = base_cfg(ia.DistanceMetric.Euclidean)
    idx, csr = fresh(orc, ("base", 1, "reference"), v, cfg, lv)
    q = uniform_vectors(8, 16, 42)
    same_answers(orc, idx, csr, v, q, 10, 600, 1)
    assert idx.last_stats()["exact_path"] > 0
    want, rows, _ = remove_and_check(orc, idx, csr, v, pick_ids(600, 500, 43), cfg)
    same_answers(orc, idx, want, rows, q, 10, 600, 1)
    assert idx.last_stats()["exact_path"] > 0
    same_answers(orc, idx, want, rows, q, 10, 50, 1)


def test_entry_seeds_are_reduced_and_remapped(orc):
    v, lv = base_rows()
    metric = ia.DistanceMetric.Euclidean
    cfg = base_cfg(metric)
    idx, csr = fresh(orc, ("base", 1, "reference"), v, cfg, lv)
    seeds = idx.select_entry_seeds(8).tolist()
    assert len(seeds) == 8
    ids = [i for i in pick_ids(600, 100, 51).tolist() if i not in seeds] + seeds[1:4]
    want, _ = rref.remove(orc, csr, v, ids, cfg.m0, 1)
    remap = idx.remove(ids)
    rows = v[remap != REMOVED]
    left = [int(remap[s]) for s in seeds if remap[s] != REMOVED]
    assert len(left) == 5 and idx.entry_seeds().tolist() == left
    assert idx.to_bytes() == csr_bytes(want, cfg, 16)
    # a plain search is the reference search over the shrunk graph entered at the nearest surviving seed
    assert_seeded_search(orc, idx, want, np.ascontiguousarray(rows), clustered_vectors(16, 16, 98), 10, 50, metric)
    # no seed left: no table, the search starts at the entry point
    idx.remove(left)
    assert idx.entry_seeds().tolist() == []
    want2, _ = rref.remove(orc, want, rows, left, cfg.m0, 1)
    same_answers(orc, idx, want2, np.ascontiguousarray(np.delete(rows, left, axis=0)), uniform_vectors(6, 16, 3), 5, 30, 1)


def test_pq_codes_are_detached(orc):
    from test_gpu_two_level import attach_pq
    from test_two_level_cpu import make_pq
    v = clustered_vectors(250, 16, 61, per_cluster=10)
    cfg = base_cfg(ia.DistanceMetric.Euclidean)
    idx, csr = fresh(orc, "pq", v, cfg)
    bare, _ = fresh(orc, "pq", v, cfg)
    cb, codes = make_pq(v, 4, 8, 10)
    q = v[:3]
    with pytest.raises(ia.CoreError) as never:
        bare.search_two_level_batch(q, 3, 8, 0.5)
    pq = attach_pq(idx, cb, codes)
    assert idx.search_two_level_batch(q, 3, 8, 0.5)[2].tolist() == [3, 3, 3]
    want, rows, _ = remove_and_check(orc, idx, csr, v, pick_ids(250, 50, 6), cfg)
    with pytest.raises(ia.CoreError) as after:  # the codes no longer cover the nodes: gone with the removal
        idx.search_two_level_batch(q, 3, 8, 0.5)
    assert after.value.kind == never.value.kind == "PQError" and str(after.value) == str(never.value)
    del pq


def test_device_resident_rows(orc):
    torch = pytest.importorskip("torch")
    v, lv = base_rows()
    cfg = base_cfg()
    _, csr = fresh(orc, ("base", 0, "reference"), v, cfg, lv)
    t = torch.from_numpy(v).to("cuda:0")
    torch.cuda.synchronize()
    idx = ia.LeannIndex.from_bytes(_built[("base", 0, "reference")][0]).upload(0)
    idx.set_embeddings(None, device_ptr=t.data_ptr(), n=600, d=16)
    del t  # the index keeps its own copy of the rows
    remove_and_check(orc, idx, csr, v, pick_ids(600, 90, 61), cfg)


# ---------------------------------------------------------------- failures
def test_failure_leaves_the_index_as_it_was(orc):
    v, lv = base_rows()
    cfg = base_cfg()
    idx, csr = fresh(orc, ("base", 0, "reference"), v, cfg, lv)
    idx.select_entry_seeds(4)
    q = uniform_vectors(16, 16, 8)
    before = state(idx, q, 10, 40), idx.entry_seeds().tolist()
    remap = np.full(600, 77, np.uint64)
    out_len = C.c_uint64(77)
    ids = np.array([5, 17, 300, 600, 8], np.uint64)  # NodeNotFound after other valid ids
    st = ia._ffi.lib().isl_index_remove(idx._h, None, ids.ctypes.data_as(C.c_void_p), ids.size,
                                        remap.ctypes.data_as(C.c_void_p), C.byref(out_len))
    assert ia._ffi.lib().isl_status_name(st).decode() == "NodeNotFound" and ia._ffi.lib().isl_last_error_node() == 600
    assert remap.tolist() == [77] * 600 and out_len.value == 77
    assert (state(idx, q, 10, 40), idx.entry_seeds().tolist()) == before
    for kw, kind in ((dict(select=7), "InvalidArgument"), (dict(select="diverse", alpha=0.5), "InvalidConfig")):
        with pytest.raises(ia.CoreError) as e:
            idx.remove([5, 17], **kw)
        assert e.value.kind == kind
        assert (state(idx, q, 10, 40), idx.entry_seeds().tolist()) == before
    idx.set_entry_seeds([])
    remove_and_check(orc, idx, csr, v, [5, 17, 300, 8], cfg)  # and it still shrinks


REFUSED_IMAGES = [("a list longer than m0", list(range(1, 10)), "longer than"),
                  ("an id twice in a list", [1, 1, 2], "verbatim"),
                  ("an id that is not below len", [1, 12], "not below")]


@pytest.mark.parametrize("what,list_of_0,words", REFUSED_IMAGES, ids=[c[0] for c in REFUSED_IMAGES])
def test_images_the_table_cannot_hold_are_refused(what, list_of_0, words):
    """from_csr and upload accept these lists; the builder's table cannot take them over.  Each is refused as
    insert refuses it, by a message that says which, and the handle is as it was."""
    n = 12
    v = uniform_vectors(n, 4, 2)
    lists = [[(i + 1) % n, (i + 2) % n] for i in range(n)]
    lists[0] = list_of_0
    cfg = ia.LeannConfig(m=4, m0=8, ef_construction=16, metric=ia.DistanceMetric.Euclidean)
    idx = index_from_lists(lists, v, cfg)
    q = uniform_vectors(4, 4, 8)
    before = state(idx, q, 5, 12)
    with pytest.raises(ia.CoreError) as e:
        idx.remove([3])
    assert e.value.kind == "Unsupported" and words in str(e.value) and "isl_index_remove" in str(e.value)
    assert state(idx, q, 5, 12) == before and len(idx) == n


def test_m0_above_128_is_refused():
    n = 12
    v = uniform_vectors(n, 4, 2)
    cfg = ia.LeannConfig(m=64, m0=129, ef_construction=200)
    idx = index_from_lists([[(i + 1) % n] for i in range(n)], v, cfg)
    blob = idx.to_bytes()
    with pytest.raises(ia.CoreError) as e:
        idx.remove([3])
    assert e.value.kind == "Unsupported" and "m0 <= 128" in str(e.value)
    with pytest.raises(ia.CoreError) as e:  # an unknown id wins over it
        idx.remove([3, 12])
    assert e.value.kind == "NodeNotFound" and idx.to_bytes() == blob


def test_the_core_of_an_hnsw_graph_is_refused():
    v = uniform_vectors(60, 8, 3)
    g = ia.HnswGraph.build(v, m=4, m0=8, ef_construction=16)
    blob = g.to_bytes()
    core = C.c_void_p.from_address(g._h.value)  # isl_hnsw's first member: the layer-0 isl_index
    ids = np.array([3, 4], np.uint64)
    out_len = C.c_uint64(77)
    st = ia._ffi.lib().isl_index_remove(core, None, ids.ctypes.data_as(C.c_void_p), 2, None, C.byref(out_len))
    assert ia._ffi.lib().isl_status_name(st).decode() == "Unsupported"
    assert "HnswGraph" in ia._ffi.lib().isl_last_error_message().decode()
    assert out_len.value == 77 and g.to_bytes() == blob and len(g) == 60


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
        idx.remove([4])
    assert e.value.kind == "Unsupported" and "recompute" in str(e.value)
    assert idx.to_bytes() == blob and len(idx) == n
    assert len(idx.search(emb[5], 1)) == 1  # and it still answers
