"""The row table on the GPU: what isl_set_embeddings, the swaps between providers and the growth of an
HnswGraph upload, read through searches that are compared with the oracle bit for bit -- ids, distance
bits, counts.  Shapes are the smallest at which the upload can go wrong: rows that pad under both stored
types (d = 5, 13), under neither (8), the shortest row (1); a host array and a device pointer as the source."""
import numpy as np
import pytest

import islands_amd as ia
from _data import clustered_vectors, knn_graph, random_levels

import _entry_seeds_ref as ref
from test_gpu_hnsw import assert_same

pytestmark = pytest.mark.gpu

N, DEGREE, K, EF, NQ = 300, 8, 5, 32, 16
_cases = {}


@pytest.fixture(scope="module", autouse=True)
def shared_cases():
    """rows, graph and queries per (d, seed) are made once and shared; they go when the module is done"""
    yield
    _cases.clear()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def case(orc, d, seed=1):
    """f32 rows, their bf16 bit patterns and the f32 images of those, a graph over the f32 rows, queries"""
    if (d, seed) not in _cases:
        x = clustered_vectors(N, d, seed)
        off, nb = knn_graph(x, DEGREE, seed=seed + 1)
        xb = ref.bf16_bits(x)
        _cases[(d, seed)] = (x, xb, ref.bf16_image(xb), orc.Csr(off, nb, entry_point=0), clustered_vectors(NQ, d, seed + 2))
    return _cases[(d, seed)]


def new_index(csr, d, metric):
    g = ia.CsrGraph(node_offsets=csr.node_offsets, neighbors=csr.neighbors, levels=csr.levels,
                    entry_point=csr.entry_point, max_level=csr.max_level, num_nodes=csr.num_nodes,
                    degree_counts=csr.degree_counts)
    return ia.LeannIndex.from_csr(g, ia.LeannConfig(metric=metric), dimension=d).upload(0)


def attach(idx, rows, bf16, on_device):
    """rows: float32 values, or uint16 bit patterns with bf16"""
    if not on_device:
        return idx.set_embeddings_bf16(rows) if bf16 else idx.set_embeddings(rows)
    import torch

    t = torch.from_numpy(rows.view(np.int16) if bf16 else rows).to("cuda:0")
    n, d = rows.shape
    (idx.set_embeddings_bf16 if bf16 else idx.set_embeddings)(None, device_ptr=t.data_ptr(), n=n, d=d)
    torch.cuda.synchronize()
    return idx


def assert_oracle(orc, idx, csr, values, queries, metric):
    ids, dist, cnt = idx.search_batch(queries, K, EF)
    for i, q in enumerate(queries):
        r = orc.leann_search(csr, values, q, K, EF, metric=int(metric))
        assert r.status == 0
        m = int(cnt[i])
        assert m == r.ids.size, (i, m, r.ids.size)
        assert ids[i, :m].tolist() == r.ids.tolist(), (i, ids[i, :m], r.ids)
        assert bits(dist[i, :m]).tolist() == bits(r.dist).tolist(), (i, dist[i, :m], r.dist)


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("metric", [ia.DistanceMetric.Cosine, ia.DistanceMetric.Euclidean], ids=["cosine", "euclidean"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("d", [1, 5, 8, 13])
def test_ragged_rows(orc, d, bf16, metric, on_device):
    x, xb, xw, csr, q = case(orc, d)
    idx = attach(new_index(csr, d, metric), xb if bf16 else x, bf16, on_device)
    assert_oracle(orc, idx, csr, xw if bf16 else x, q, metric)


@pytest.mark.parametrize("metric", [ia.DistanceMetric.Cosine, ia.DistanceMetric.Euclidean], ids=["cosine", "euclidean"])
def test_swaps_on_one_index(orc, metric):
    """f32 rows x, then bf16 rows of another matrix y, then f32 rows z: a stale block or a stale type shows in
    the search after the swap, stale seeds in entry_seeds()"""
    d = 13
    x, _, _, csr, q = case(orc, d, 1)
    _, yb, yw, _, _ = case(orc, d, 11)
    z = case(orc, d, 21)[0]
    idx = new_index(csr, d, metric)
    for rows, values, bf16 in ((x, x, False), (yb, yw, True), (z, z, False)):
        attach(idx, rows, bf16, False)
        assert idx.entry_seeds().size == 0
        assert_oracle(orc, idx, csr, values, q, metric)
        idx.set_entry_seeds([0, 7, 19])
        assert idx.entry_seeds().tolist() == [0, 7, 19]


def test_a_refused_swap_changes_nothing(orc):
    import torch

    d, metric = 5, ia.DistanceMetric.Cosine
    x, _, _, csr, q = case(orc, d)
    idx = attach(new_index(csr, d, metric), x, False, False)
    other = torch.from_numpy(case(orc, d, 11)[0]).to("cuda:0")
    for n, dd, kind in ((0, d, "EmptyCollection"), (N, 0, "InvalidArgument")):
        with pytest.raises(ia.CoreError) as e:
            idx.set_embeddings(None, device_ptr=other.data_ptr(), n=n, d=dd)
        assert e.value.kind == kind
        with pytest.raises(ia.CoreError):
            idx.set_embeddings_bf16(None, device_ptr=other.data_ptr(), n=n, d=dd)
    with pytest.raises(ia.CoreError):
        idx.set_embeddings(np.zeros((0, d), np.float32))
    with pytest.raises(ia.CoreError):
        idx.set_embeddings(np.zeros((N, 0), np.float32))
    assert_oracle(orc, idx, csr, x, q, metric)


def test_growth(orc):
    """HnswGraph.build over 100 rows, insert of 50 more: every row comes back bit for bit (old rows copied on the
    device, new ones uploaded behind them at a padded stride) and the graph searches like the oracle's"""
    d, m, m0, efc, metric = 13, 8, 16, 40, ia.DistanceMetric.Cosine
    v = clustered_vectors(150, d, 5)
    lv = random_levels(150, m, 6)
    g = ia.HnswGraph.build(v[:100], m=m, m0=m0, ef_construction=efc, metric=metric, levels=lv[:100])
    assert g.insert(v[100:], levels=lv[100:]) == 100 and len(g) == 150
    for i in range(150):
        assert bits(g.get_vector(i)).tolist() == bits(v[i]).tolist(), i
    h = orc.Hnsw(m=m, m0=m0, ef_construction=efc, metric=int(metric))
    for i in range(150):
        st, node = h.insert(v[i], int(lv[i]))
        assert st == 0 and node == i
    assert g.entry_point == h.entry_point and g.max_level == h.max_level
    for i in range(150):  # the oracle's layers are the resulting layers
        for L in range(int(lv[i]) + 1):
            assert g.neighbors(i, L) == list(h.neighbors(i, L) or []), (i, L)
    assert_same(h, g, clustered_vectors(NQ, d, 7), K, EF)
