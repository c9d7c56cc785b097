"""Entry seeds on the GPU against tests/_entry_seeds_ref.py (the definition of include/islands_amd.h restated
on oracle.batch_distance) and oracle.leann_search: the selection element for element, the pick id for id, a
seeded search as the reference search entered at the pick -- ids, distance bits, counts and the H / E / V /
push totals.  Shapes are the smallest that reach every path: rows and seeds that are no multiple of the
64-row wave, the 32 x 32 pick tile or the 32-element chunk, more seed tiles than one range, d not a
multiple of 4."""
import os

import numpy as np
import pytest

import islands_amd as ia
from _data import uniform_vectors

import _entry_seeds_ref as ref

pytestmark = pytest.mark.gpu

METRICS = [ia.DistanceMetric.Cosine, ia.DistanceMetric.Euclidean, ia.DistanceMetric.DotProduct,
           ia.DistanceMetric.Manhattan]
COUNTERS = ("expansions", "edges", "evals", "pushes")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make_index(csr, rows, metric=ia.DistanceMetric.Cosine, bf16=False, **cfg):
    g = ia.CsrGraph(node_offsets=csr.node_offsets, neighbors=csr.neighbors, levels=csr.levels,
                    entry_point=csr.entry_point, max_level=csr.max_level, num_nodes=csr.num_nodes,
                    degree_counts=csr.degree_counts)
    idx = ia.LeannIndex.from_csr(g, ia.LeannConfig(metric=metric, **cfg), dimension=rows.shape[1]).upload(0)
    if bf16:
        idx.set_embeddings_bf16(ref.bf16_bits(rows))
    else:
        idx.set_embeddings(rows)
    return idx


def chain_csr(orc, n, entry=0):
    """A ring: enough of a graph for the calls that never traverse it."""
    return orc.Csr(np.arange(n + 1, dtype=np.uint64), (np.arange(n, dtype=np.uint64) + 1) % n, entry_point=entry)


def fixture_index(orc, metric, bf16=False, **cfg):
    x, q = ref.fixture()
    case = "bf16" if bf16 else metric.name
    rows = ref.bf16_image(ref.bf16_bits(x)) if bf16 else x
    csr = ref.knn_csr(orc, int(metric), rows, tag=case)
    return make_index(csr, rows, metric, bf16, **cfg), csr, rows, q


def assert_seeded_search(orc, idx, csr, rows, queries, k, ef, metric, got=None, **okw):
    """`got` (ids, dist, count, stats) or a search_batch now; against the oracle entered at every query's pick."""
    seeds = idx.entry_seeds().tolist()
    entries = ref.pick(orc, int(metric), queries, rows, seeds) if seeds else [csr.entry_point] * len(queries)
    if got is None:
        ids, dist, cnt = idx.search_batch(queries, k, ef)
        st = idx.last_stats()
    else:
        ids, dist, cnt, st = got
    tot = dict.fromkeys(COUNTERS, 0)
    for i, q in enumerate(queries):
        r = orc.leann_search(ref.with_entry(orc, csr, entries[i]), rows, q, k, ef, metric=int(metric), **okw)
        assert r.status == 0
        n = int(cnt[i])
        assert n == r.ids.size, (i, n, r.ids.size)
        assert np.asarray(ids[i, :n]).tolist() == r.ids.tolist(), (i, ids[i, :n], r.ids)
        assert bits(dist[i, :n]).tolist() == bits(r.dist).tolist(), (i, dist[i, :n], r.dist)
        for f in COUNTERS:
            tot[f] += r.counters[f]
    for f in COUNTERS:
        assert st[f] == tot[f], (f, st, tot)
    return ids, dist, cnt, st


# ------------------------------------------------------------------ selection
@pytest.mark.parametrize("metric", METRICS)
def test_selection_on_the_fixture(orc, metric):
    idx, csr, x, _ = fixture_index(orc, metric)
    want = ref.select(orc, int(metric), x, 0, 64)
    for count in (1, 2, 17, 64):
        got = idx.select_entry_seeds(count)
        assert got.dtype == np.uint64 and got.tolist() == want[:count], (metric, count)
        assert idx.entry_seeds().tolist() == want[:count]


def test_selection_bf16_rows(orc):
    idx, csr, x, _ = fixture_index(orc, ia.DistanceMetric.Cosine, bf16=True)
    assert idx.select_entry_seeds(64).tolist() == ref.select(orc, 0, x, 0, 64)


@pytest.mark.parametrize("metric", METRICS)
def test_selection_more_seeds_than_rows_and_entry(orc, metric):
    x = uniform_vectors(5, 7, 3)
    idx = make_index(chain_csr(orc, 5, entry=3), x, metric)
    got = idx.select_entry_seeds(9)
    assert got.tolist() == ref.select(orc, int(metric), x, 3, 9) and sorted(got.tolist()) == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("d", [1, 3, 17, 33])
@pytest.mark.parametrize("bf16", [False, True])
def test_selection_odd_dimensions(orc, d, bf16):
    x = np.random.default_rng(d).standard_normal((203, d)).astype(np.float32)
    if bf16:
        x = ref.bf16_image(ref.bf16_bits(x))
    for metric in METRICS:
        idx = make_index(chain_csr(orc, 203), x, metric, bf16)
        assert idx.select_entry_seeds(12).tolist() == ref.select(orc, int(metric), x, 0, 12), (metric, d, bf16)


@pytest.mark.parametrize("bf16", [False, True])
def test_selection_wide_rows(orc, bf16):
    x = np.random.default_rng(768).standard_normal((512, 768)).astype(np.float32)
    if bf16:
        x = ref.bf16_image(ref.bf16_bits(x))
    for metric in (ia.DistanceMetric.Cosine, ia.DistanceMetric.Euclidean):
        idx = make_index(chain_csr(orc, 512), x, metric, bf16)
        assert idx.select_entry_seeds(9).tolist() == ref.select(orc, int(metric), x, 0, 9), (metric, bf16)


@pytest.mark.parametrize("metric", METRICS)
def test_selection_duplicate_rows_tie_to_the_smaller_id(orc, metric):
    """Every row exists four times (ids i, i + 50, i + 100, i + 150 after the shuffle below): each maximum
    of mind is shared by equal rows and must go to the smallest id; a chosen row's twins, at distance
    D(x, x) from it, stay candidates (under DotProduct that is not 0)."""
    r = np.random.default_rng(5)
    base = r.standard_normal((50, 9)).astype(np.float32)
    x = np.ascontiguousarray(np.tile(base, (4, 1))[r.permutation(200)])
    idx = make_index(chain_csr(orc, 200), x, metric)
    assert idx.select_entry_seeds(70).tolist() == ref.select(orc, int(metric), x, 0, 70)


def test_selection_with_nan_rows_is_deterministic(orc):
    x = uniform_vectors(150, 8, 9).copy()
    x[[3, 77, 149]] = np.nan
    idx = make_index(chain_csr(orc, 150), x, ia.DistanceMetric.Euclidean)
    a = idx.select_entry_seeds(20).tolist()
    b = idx.select_entry_seeds(20).tolist()
    assert a == b and len(set(a)) == 20 and a[0] == 0 and max(a) < 150


# ----------------------------------------------------------------------- pick
def _pick_case(orc, metric, d, n_seeds, nq, bf16, seed):
    r = np.random.default_rng(seed)
    n = 300
    x = r.standard_normal((n, d)).astype(np.float32)
    x[11] = 0.0  # a zero row: Cosine distance 1.0 from everything
    if bf16:
        x = ref.bf16_image(ref.bf16_bits(x))
    seeds = r.integers(0, n, n_seeds).tolist()
    if n_seeds >= 15:
        seeds[3] = 11
        seeds[n_seeds - 1] = seeds[1]  # a repeated id: the smaller position wins
    q = r.standard_normal((nq, d)).astype(np.float32)
    q[0] = 0.0   # a zero query
    if nq > 2:
        q[2] = x[seeds[n_seeds // 2]]  # a query that is a seed row
    idx = make_index(chain_csr(orc, n), x, metric, bf16)
    idx.set_entry_seeds(seeds)
    assert idx.entry_seeds().tolist() == seeds
    got = idx.pick_entries(q)
    want = ref.pick(orc, int(metric), q, x, seeds)
    assert got.dtype == np.uint64 and got.tolist() == want.tolist(), (metric, d, n_seeds, nq, bf16)
    return idx, q, want


@pytest.mark.parametrize("n_seeds", [1, 15, 17, 65, 257])
@pytest.mark.parametrize("metric", METRICS)
def test_pick_seed_counts(orc, metric, n_seeds):
    for nq in (1, 17, 257):
        _pick_case(orc, metric, 17, n_seeds, nq, False, 100 + n_seeds)


@pytest.mark.parametrize("d", [1, 3, 17, 33, 768])
@pytest.mark.parametrize("bf16", [False, True])
def test_pick_dimensions(orc, d, bf16):
    for metric in METRICS:
        _pick_case(orc, metric, d, 65, 17, bf16, 200 + d)


def test_pick_zero_vectors_under_cosine(orc):
    """Every seed is at 1.0 from a zero query: position 0 wins; a zero seed row is at 1.0 from every query."""
    idx, q, want = _pick_case(orc, ia.DistanceMetric.Cosine, 17, 17, 17, False, 300)
    assert want[0] == idx.entry_seeds()[0]


def test_pick_device_buffers(orc):
    import torch
    idx, q, want = _pick_case(orc, ia.DistanceMetric.Euclidean, 33, 65, 257, False, 400)
    dq = torch.from_numpy(q).cuda()
    out = torch.zeros(q.shape[0], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    idx.pick_entries(d_queries_ptr=dq.data_ptr(), nq=q.shape[0], d=q.shape[1], d_out_ptr=out.data_ptr())
    assert out.cpu().numpy().astype(np.uint64).tolist() == want.tolist()


def test_argument_errors(orc):
    x = uniform_vectors(40, 8, 1)
    idx = make_index(chain_csr(orc, 40), x)
    with pytest.raises(ia.CoreError) as e:
        idx.set_entry_seeds([1, 40, 2])
    assert e.value.kind == "NodeNotFound" and e.value.node == 40
    with pytest.raises(ia.CoreError) as e:
        idx.pick_entries(x[:2])  # no table
    assert e.value.kind == "InvalidArgument"
    idx.set_entry_seeds([5, 6])
    with pytest.raises(ia.CoreError) as e:
        idx.pick_entries(np.zeros((2, 9), np.float32))
    assert e.value.kind == "DimensionMismatch" and (e.value.expected, e.value.actual) == (8, 9)
    with pytest.raises(ia.CoreError) as e:
        idx.select_entry_seeds(65537)
    assert e.value.kind == "Unsupported"
    assert idx.entry_seeds().tolist() == [5, 6]  # failed calls leave the table alone


# --------------------------------------------------------------------- search
@pytest.mark.parametrize("metric", METRICS)
def test_search_equals_reference_entered_at_the_pick(orc, metric):
    idx, csr, x, q = fixture_index(orc, metric)
    idx.select_entry_seeds(64)
    assert_seeded_search(orc, idx, csr, x, q, 5, 32, metric)


@pytest.mark.parametrize("strategy", [ia.PruningStrategy.Global, ia.PruningStrategy.Local])
def test_search_with_pruning(orc, strategy):
    m = ia.DistanceMetric.Cosine
    idx, csr, x, q = fixture_index(orc, m, prune_ratio=0.4, pruning_strategy=strategy)
    idx.select_entry_seeds(64)
    assert_seeded_search(orc, idx, csr, x, q, 5, 32, m, prune_ratio=0.4, strategy=int(strategy))


def test_search_bf16_rows(orc):
    m = ia.DistanceMetric.Cosine
    idx, csr, x, q = fixture_index(orc, m, bf16=True)
    idx.select_entry_seeds(64)
    assert_seeded_search(orc, idx, csr, x, q, 5, 32, m)


def test_search_wide_adjacency_rows(orc):
    """Rows of 65-128 neighbour ids: the fast kernel's wide-row instantiation."""
    n, d = 300, 12
    x = uniform_vectors(n, d, 21)
    r = np.random.default_rng(22)
    nb = np.concatenate([r.choice(n, size=100, replace=False) for _ in range(n)]).astype(np.uint64)
    csr = orc.Csr(np.arange(0, n * 100 + 1, 100, dtype=np.uint64), nb, entry_point=0)
    deg = np.diff(csr.node_offsets)
    assert deg.min() >= 65 and deg.max() <= 128, (deg.min(), deg.max())
    m = ia.DistanceMetric.Euclidean
    idx = make_index(csr, x, m)
    idx.select_entry_seeds(17)
    assert_seeded_search(orc, idx, csr, x, uniform_vectors(24, d, 23), 10, 48, m)


def test_search_on_the_heap_exact_kernel(orc):
    """ef = 600 is above the fast kernel's 512: every query goes to leann_search_exact."""
    m = ia.DistanceMetric.Cosine
    idx, csr, x, q = fixture_index(orc, m)
    idx.select_entry_seeds(64)
    _, _, _, st = assert_seeded_search(orc, idx, csr, x, q[:16], 5, 600, m)
    assert st["exact_path"] == 16


def test_search_async_and_device_entry_points(orc):
    import torch
    m = ia.DistanceMetric.Cosine
    idx, csr, x, q = fixture_index(orc, m)
    idx.select_entry_seeds(64)
    parts = [q[0:16], q[16:32], q[32:48], q[48:64]]
    toks = [idx.search_batch_async(p, 5, 32) for p in parts]  # four calls in flight
    outs = [idx._pending[t] for t in toks]
    stats = [idx.wait_stats(t) for t in toks]
    for p, (ids, dist, cnt), st in zip(parts, outs, stats):
        assert_seeded_search(orc, idx, csr, x, p, 5, 32, m, got=(ids, dist, cnt, st))
    dq = torch.from_numpy(np.array(q)).cuda()  # (the shared fixture is read-only)
    ids = torch.zeros((64, 5), dtype=torch.int64, device="cuda")
    dist = torch.zeros((64, 5), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(64, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    idx.search_batch_device(dq.data_ptr(), 64, x.shape[1], 5, 32, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
    got = (ids.cpu().numpy().astype(np.uint64), dist.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32),
           idx.last_stats())
    assert_seeded_search(orc, idx, csr, x, q, 5, 32, m, got=got)
    tok = idx.search_batch_device_async(dq.data_ptr(), 64, x.shape[1], 5, 32, ids.data_ptr(), dist.data_ptr(),
                                        cnt.data_ptr())
    st = idx.wait_stats(tok)
    got = (ids.cpu().numpy().astype(np.uint64), dist.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32), st)
    assert_seeded_search(orc, idx, csr, x, q, 5, 32, m, got=got)
    # the one-query entry point
    one = idx.search_with_params(q[5], 5, 32)
    r = orc.leann_search(ref.with_entry(orc, csr, ref.pick(orc, 0, q[5:6], x, idx.entry_seeds())[0]), x, q[5], 5, 32)
    assert [i for i, _ in one] == r.ids.tolist()


def test_recall_before_and_after_on_one_index(orc):
    m = ia.DistanceMetric.Cosine
    idx, csr, x, q = fixture_index(orc, m)
    ids, _, cnt = idx.search_batch(q, 5, 32)
    before = ref.recall_at(orc, 0, q, x, ids, cnt, 5)
    assert len(idx.select_entry_seeds(64)) == 64
    ids, _, cnt = idx.search_batch(q, 5, 32)
    after = ref.recall_at(orc, 0, q, x, ids, cnt, 5)
    print(f"recall@5: {before:.3f} from node 0, {after:.3f} with 64 entry seeds")
    assert before <= 0.1, before
    assert after >= 0.9, after


def test_entry_point_as_the_only_seed_and_clearing(orc):
    m = ia.DistanceMetric.Euclidean
    idx, csr, x, q = fixture_index(orc, m)
    plain = make_index(csr, x, m)  # never had seeds
    ids0, dist0, cnt0 = plain.search_batch(q, 5, 32)
    st0 = plain.last_stats()

    def same_as_plain():
        ids, dist, cnt = idx.search_batch(q, 5, 32)
        st = idx.last_stats()
        assert ids.tolist() == ids0.tolist() and cnt.tolist() == cnt0.tolist()
        assert bits(dist).tolist() == bits(dist0).tolist()
        for f in COUNTERS + ("exact_path", "replayed", "queries"):
            assert st[f] == st0[f], (f, st, st0)

    same_as_plain()
    idx.set_entry_seeds([csr.entry_point])
    same_as_plain()
    idx.select_entry_seeds(64)
    ids, _, _ = idx.search_batch(q, 5, 32)
    assert ids.tolist() != ids0.tolist()
    idx.set_entry_seeds([])
    assert idx.entry_seeds().size == 0
    same_as_plain()
    idx.select_entry_seeds(64)
    idx.select_entry_seeds(0)  # selecting none clears as well
    assert idx.entry_seeds().size == 0
    same_as_plain()


def test_prepare_after_seeding_leaves_nothing_to_allocate(orc):
    m = ia.DistanceMetric.Cosine
    idx, csr, x, q = fixture_index(orc, m)
    idx.select_entry_seeds(64)
    idx.prepare(64, 64, 5, lanes=4)
    for _ in range(2):
        idx.search_batch(q, 5, 32)
        assert idx.last_stats()["allocations"] == 0
    toks = [idx.search_batch_async(q[i * 16:(i + 1) * 16], 5, 64) for i in range(4)]
    assert all(idx.wait_stats(t)["allocations"] == 0 for t in toks)


def test_two_level_ignores_the_table_and_new_rows_drop_it(orc):
    m = ia.DistanceMetric.Euclidean
    idx, csr, x, q = fixture_index(orc, m)
    r = np.random.default_rng(3)
    books = np.ascontiguousarray(r.standard_normal((4, 16, 4)).astype(np.float32))
    pq = ia.ProductQuantizer(x.shape[1], books, metric=m)
    idx.set_pq_codes(pq, pq.encode(x))
    a = idx.search_two_level_batch(q, 5, 32, 0.5)
    sa = idx.last_stats()
    idx.select_entry_seeds(64)
    b = idx.search_two_level_batch(q, 5, 32, 0.5)
    sb = idx.last_stats()
    assert a[0].tolist() == b[0].tolist() and bits(a[1]).tolist() == bits(b[1]).tolist()
    assert a[2].tolist() == b[2].tolist()
    for f in COUNTERS:
        assert sa[f] == sb[f], (f, sa, sb)
    assert idx.entry_seeds().size == 64
    idx.set_embeddings(x)
    assert idx.entry_seeds().size == 0


def test_env_variable_selects_after_a_build(orc, monkeypatch):
    x = uniform_vectors(300, 12, 31)
    cfg = ia.LeannConfig(m=8, m0=16, ef_construction=40)
    monkeypatch.setenv("ISL_ENTRY_SEEDS", "16")
    idx = ia.LeannIndex.build(x, cfg, batch=32)
    monkeypatch.delenv("ISL_ENTRY_SEEDS")
    assert idx.entry_seeds().tolist() == ref.select(orc, 0, x, idx.entry_point, 16)
    assert ia.LeannIndex.build(x[:50], cfg, batch=32).entry_seeds().size == 0
    monkeypatch.setenv("ISL_ENTRY_SEEDS", "sixteen")
    with pytest.raises(ia.CoreError) as e:
        ia.LeannIndex.build(x[:50], cfg, batch=32)
    assert e.value.kind == "InvalidArgument"
