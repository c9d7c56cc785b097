"""fp8 e4m3 rows on the device (ISL_DTYPE_FP8_E4M3, LeannIndex.set_embeddings_fp8): the provider's vectors are
the exact f32 images e4m3(code) * 2^scale_exp, the arithmetic is the reference's f32 chain, so every search
equals the oracle run on ia.fp8_e4m3_to_f32(codes, scale_exp) with a graph the oracle built on those images:
ids, distance bits and the H / E / V / push counters."""
import functools

import numpy as np
import pytest
import torch

import islands_amd as ia
from _data import clustered_vectors, random_csr, uniform_vectors

pytestmark = pytest.mark.gpu

METRICS = [ia.DistanceMetric.Cosine, ia.DistanceMetric.Euclidean, ia.DistanceMetric.DotProduct,
           ia.DistanceMetric.Manhattan]
FINITE_CODES = np.array([c for c in range(256) if c not in (0x7F, 0xFF)], dtype=np.uint8)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_search(orc, idx, csr, vectors, queries, k, ef, **okw):
    """idx.search_batch against the oracle over `vectors`: ids and distance bits per query; returns the call's
    counters and the oracle's, summed."""
    ids, dist, cnt = idx.search_batch(queries, k, ef)
    st = idx.last_stats()
    tot = {"expansions": 0, "edges": 0, "evals": 0, "pushes": 0}
    for i, q in enumerate(queries):
        r = orc.leann_search(csr, vectors, q, k, ef, **okw)
        assert r.status == 0
        n = int(cnt[i])
        assert n == r.ids.size, (i, n, r.ids.size)
        assert ids[i, :n].tolist() == r.ids.tolist(), (i, ids[i, :n], r.ids)
        assert bits(dist[i, :n]).tolist() == bits(r.dist).tolist(), (i, dist[i, :n], r.dist)
        for f in tot:
            tot[f] += r.counters[f]
    return st, tot


def assert_parity(orc, idx, csr, images, queries, k, ef, metric):
    st, tot = assert_same_search(orc, idx, csr, images, queries, k, ef, metric=int(metric))
    for f in tot:
        assert st[f] == tot[f], f
    return st


def fp8_index(csr, codes, scale_exp, metric, m, m0, efc):
    g = ia.CsrGraph(node_offsets=csr.node_offsets, neighbors=csr.neighbors, levels=csr.levels,
                    entry_point=csr.entry_point, max_level=csr.max_level, num_nodes=csr.num_nodes,
                    degree_counts=csr.degree_counts)
    idx = ia.LeannIndex.from_csr(g, ia.LeannConfig(m=m, m0=m0, ef_construction=efc, metric=metric), dimension=codes.shape[1])
    idx.upload(0)
    idx.set_embeddings_fp8(codes, scale_exp)
    return idx


@functools.lru_cache(maxsize=None)
def quantised_rows(n, d, seed):
    """codes and exponent of clustered rows, as quantize_fp8_e4m3 makes them"""
    codes, e = ia.quantize_fp8_e4m3(clustered_vectors(n, d, seed))
    codes.setflags(write=False)
    return codes, e


def case(orc, codes, scale_exp, metric, m=8, m0=16, efc=40):
    """(images, the oracle's graph on them, the index holding the codes)"""
    images = ia.fp8_e4m3_to_f32(codes, scale_exp)
    csr = orc.leann_build(images, m=m, m0=m0, ef_construction=efc, metric=int(metric))
    return images, csr, fp8_index(csr, codes, scale_exp, metric, m, m0, efc)


# A step is 64 elements, the load ring four steps.  d = 40: the guarded tail alone, rows padded to 48 bytes;
# 300: the ring exactly (4 full steps, no reload) and a guarded tail of 44 elements; 768: 12 full steps, the
# reload loop twice and the ring, no tail; 1640: the reload loop (25 full steps), the ring, a full step and a
# partial one of 40 elements in the guarded tail
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [40, 300, 768, 1640])
def test_quantised_rows_match_the_oracle_on_their_images(orc, metric, d):
    codes, e = quantised_rows(900, d, 31)
    images, csr, idx = case(orc, codes, e, metric)
    q = clustered_vectors(24, d, 32)  # arbitrary f32 queries
    st = assert_parity(orc, idx, csr, images, q, 10, 48, metric)
    assert st["exact_path"] == 0


@pytest.mark.parametrize("metric", [ia.DistanceMetric.Cosine, ia.DistanceMetric.Euclidean])
@pytest.mark.parametrize("scale_exp", [-7, 5])
def test_the_scale_exponent_is_part_of_the_image(orc, metric, scale_exp):
    codes, _ = quantised_rows(900, 768, 31)
    images, csr, idx = case(orc, codes, scale_exp, metric)
    q = clustered_vectors(24, 768, 32) * np.float32(2.0 ** (scale_exp + 9))  # (queries of the rows' magnitude)
    st = assert_parity(orc, idx, csr, images, q, 10, 48, metric)
    assert st["exact_path"] == 0


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("scale_exp", [0, -9])
def test_every_code_widens_to_its_exact_image(orc, metric, scale_exp):
    """Rows drawn uniformly from the 254 non-NaN bytes -- subnormals, both zeros, +-448 -- at d = 832 (13 full
    steps: the reload loop, the ring and one step of the tail): a convert that rounded or flushed any code under
    any of the two scales would move distance bits."""
    rng = np.random.default_rng(77)
    codes = FINITE_CODES[rng.integers(0, FINITE_CODES.size, size=(300, 832))]
    codes[0, :254] = FINITE_CODES  # every one of them at least once, whatever the draw
    assert np.unique(codes).size == 254
    images, csr, idx = case(orc, codes, scale_exp, metric)
    q = ia.fp8_e4m3_to_f32(FINITE_CODES[rng.integers(0, FINITE_CODES.size, size=(12, 832))], scale_exp)
    q = np.concatenate([q, (uniform_vectors(12, 832, 78) * np.float32(100.0 * 2.0 ** scale_exp))])
    assert_parity(orc, idx, csr, images, q, 10, 48, metric)


def test_wide_adjacency_rows(orc):
    """more than 64 ids in an adjacency row: the WIDE instantiation"""
    codes, e = quantised_rows(400, 96, 41)
    metric = ia.DistanceMetric.Cosine
    images, csr, idx = case(orc, codes, e, metric, m=40, m0=100, efc=128)
    assert int(np.diff(csr.node_offsets.astype(np.int64)).max()) > 64
    st = assert_parity(orc, idx, csr, images, clustered_vectors(24, 96, 42), 10, 64, metric)
    assert st["exact_path"] == 0


# one ef per result-set size of the fast kernel (fast_segments, search_geometry.hpp: ef <= 64, <= 128, <= 256,
# <= 512 give S = 1, 2, 4, 8) and one past 512, which the heap-exact kernel answers
@pytest.mark.parametrize("ef", [48, 100, 200, 400, 600])
def test_every_result_set_size_and_the_exact_kernel(orc, ef):
    codes, e = quantised_rows(900, 72, 51)
    metric = ia.DistanceMetric.Euclidean
    images, csr, idx = case(orc, codes, e, metric)
    st = assert_parity(orc, idx, csr, images, clustered_vectors(16, 72, 52), 10, ef, metric)
    assert (st["exact_path"] == 16) if ef > 512 else (st["exact_path"] == 0)


def test_ties_take_the_exact_kernel(orc):
    rng = np.random.default_rng(3)
    base = FINITE_CODES[rng.integers(0, FINITE_CODES.size, size=(80, 24))]
    codes = np.concatenate([base, base, base[:40]])
    metric = ia.DistanceMetric.Cosine
    images, csr, idx = case(orc, codes, -4, metric, m=6, m0=12, efc=30)
    st, _ = assert_same_search(orc, idx, csr, images, images[:16], 10, 30)
    assert st["exact_path"] + st["replayed"] > 0


def test_zero_rows_and_a_zero_query_under_cosine(orc):
    """norm == 0 -> distance 1.0 (distance.rs:82-85), for a row of +0 codes, one of -0 codes and a zero query"""
    codes = quantised_rows(200, 40, 61)[0].copy()
    codes[5] = 0x00
    codes[17] = 0x80
    metric = ia.DistanceMetric.Cosine
    images = ia.fp8_e4m3_to_f32(codes, -8)
    # a random graph entered at the zero row (a builder's graph need not keep an edge to a row that is far from
    # every other); ef = k = n below returns every node it reaches
    off, nb = random_csr(200, 16, 63)
    csr = orc.Csr(off, nb, entry_point=5)
    idx = fp8_index(csr, codes, -8, metric, 8, 16, 40)
    q = clustered_vectors(8, 40, 62)
    q[3] = 0.0
    ids, dist, cnt = idx.search_batch(q, 200, 200)
    assert_parity(orc, idx, csr, images, q, 200, 200, metric)
    assert (dist[3, :int(cnt[3])] == 1.0).all() and int(cnt[3]) > 0
    for row in (5, 17):
        hit = np.nonzero(ids[0, :int(cnt[0])] == row)[0]
        assert hit.size == 1 and dist[0, hit[0]] == 1.0


def test_host_codes_device_codes_and_the_async_call_agree(orc):
    codes, e = quantised_rows(900, 72, 51)
    metric = ia.DistanceMetric.DotProduct
    images, csr, idx = case(orc, codes, e, metric)
    q = clustered_vectors(32, 72, 53)
    ids, dist, cnt = idx.search_batch(q, 10, 64)
    t = torch.from_numpy(codes.copy()).to("cuda:0")
    torch.cuda.synchronize()
    dev = fp8_index(csr, codes, 0, metric, 8, 16, 40)  # (another scale first: the device call replaces the table)
    dev.set_embeddings_fp8(None, e, device_ptr=t.data_ptr(), n=codes.shape[0], d=codes.shape[1])
    del t  # the index keeps its own copy
    ids2, dist2, cnt2 = dev.search_batch(q, 10, 64)
    assert cnt2.tolist() == cnt.tolist() and ids2.tolist() == ids.tolist() and bits(dist2).tolist() == bits(dist).tolist()
    assert dev.row_storage() == idx.row_storage()
    ids3, dist3, cnt3 = dev.wait(dev.search_batch_async(q, 10, 64))
    assert cnt3.tolist() == cnt.tolist() and ids3[:, :10].tolist() == ids.tolist()
    assert bits(dist3[:, :10]).tolist() == bits(dist).tolist()
    assert_parity(orc, dev, csr, images, q, 10, 64, metric)


def test_provider_swaps_answer_each_providers_oracle(orc):
    n, d = 600, 72
    rows = clustered_vectors(n, d, 71)
    codes, e = ia.quantize_fp8_e4m3(rows)
    images = ia.fp8_e4m3_to_f32(codes, e)
    metric = ia.DistanceMetric.Cosine
    csr = orc.leann_build(rows, m=8, m0=16, ef_construction=40, metric=int(metric))
    idx = fp8_index(csr, codes, e, metric, 8, 16, 40)
    q = clustered_vectors(16, d, 72)
    assert_parity(orc, idx, csr, images, q, 10, 48, metric)
    idx.set_embeddings(rows)
    assert idx.row_storage()["dtype"] == 0 and idx.row_storage()["scale_exp"] == 0
    assert_parity(orc, idx, csr, rows, q, 10, 48, metric)
    idx.set_embeddings_fp8(codes, e)
    assert_parity(orc, idx, csr, images, q, 10, 48, metric)
    idx.set_embeddings(rows)
    assert_parity(orc, idx, csr, rows, q, 10, 48, metric)


@pytest.mark.parametrize("d,scale_exp", [(40, -9), (768, 0), (17, 32)])
def test_row_storage_reports_what_the_rows_cost(orc, d, scale_exp):
    n = 50
    codes = np.zeros((n, d), dtype=np.uint8)
    codes[:, 0] = 0x38  # 1.0
    images = ia.fp8_e4m3_to_f32(codes, 0)
    csr = orc.leann_build(images, m=4, m0=8, ef_construction=16)
    idx = fp8_index(csr, codes, scale_exp, ia.DistanceMetric.Cosine, 4, 8, 16)
    assert idx.row_storage() == {"dtype": 2, "scale_exp": scale_exp, "block_bytes": n * ((d + 15) // 16 * 16) + 1024}
    idx.set_embeddings(images)
    assert idx.row_storage() == {"dtype": 0, "scale_exp": 0, "block_bytes": (n * ((d + 3) // 4 * 4) + 256) * 4}


def test_what_an_fp8_index_refuses(orc):
    n, d = 300, 32
    rows = clustered_vectors(n, d, 81)
    codes, e = ia.quantize_fp8_e4m3(rows)
    metric = ia.DistanceMetric.Cosine
    csr = orc.leann_build(rows, m=8, m0=16, ef_construction=40, metric=int(metric))
    idx = fp8_index(csr, codes, e, metric, 8, 16, 40)
    idx.set_embeddings(rows)
    assert len(idx.select_entry_seeds(8)) == 8 and len(idx.entry_seeds()) == 8
    idx.set_embeddings_fp8(codes, e)
    assert len(idx.entry_seeds()) == 0  # the seeds were copies of the rows that went
    q = clustered_vectors(4, d, 82)
    refused = {
        "remove": lambda: idx.remove([1]),
        "insert": lambda: idx.insert(rows[:2]),
        "insert_bf16": lambda: idx.insert_bf16((rows[:2].view(np.uint32) >> 16).astype(np.uint16)),
        "select_entry_seeds": lambda: idx.select_entry_seeds(4),
        "set_entry_seeds": lambda: idx.set_entry_seeds([1, 2]),
        "two_level": lambda: idx.search_two_level_batch(q, 5, 32, 0.5),
    }
    for name, call in refused.items():
        with pytest.raises(ia.CoreError) as err:
            call()
        assert err.value.kind == "Unsupported" and "fp8" in str(err.value), (name, str(err.value))
    # nothing above touched the index
    assert len(idx) == n and idx.row_storage()["dtype"] == 2 and len(idx.entry_seeds()) == 0
    assert_parity(orc, idx, csr, ia.fp8_e4m3_to_f32(codes, e), q, 10, 48, metric)
    # the builders keep taking dtype 2 for an unknown type
    with pytest.raises(ia.CoreError) as err:
        idx._insert(codes[:2], 2, None, 1, "reference", 1.0, True)
    assert err.value.kind == "InvalidArgument" and "unknown row dtype" in str(err.value)
