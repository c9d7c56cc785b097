"""Row conversions on the device: isl_quantize_fp8_e4m3 / isl_round_bf16 against the Python definitions byte for
byte, and LeannIndex.convert_rows against a twin index whose rows were narrowed on the host and attached with
set_embeddings_bf16 / set_embeddings_fp8: row_storage, read_rows, and every search against the oracle run on the
target's images (ids, distance bits, the H / E / V / push counters; cosine covers the norms).  Then the chains,
the lifecycle a widening buys an fp8 index, the entry seeds, the no-ops and every refusal."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import islands_amd as ia
from islands_amd import _ffi
from _convert_ref import (EXPONENTS, auto_scale_exp, bf16_tie_patterns, boundary_set, is_nan_bits, random_patterns)
from _data import clustered_vectors
from test_gpu_fp8_rows import METRICS, assert_parity, bits

pytestmark = pytest.mark.gpu

COSINE = ia.DistanceMetric.Cosine
M, M0, EFC = 8, 16, 40


def bf16_images(b16):
    return (np.ascontiguousarray(b16, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def graph_of(csr):
    return ia.CsrGraph(node_offsets=csr.node_offsets, neighbors=csr.neighbors, levels=csr.levels,
                       entry_point=csr.entry_point, max_level=csr.max_level, num_nodes=csr.num_nodes,
                       degree_counts=csr.degree_counts)


def bare_index(csr, d, metric=COSINE):
    """from_csr + upload, no rows yet"""
    idx = ia.LeannIndex.from_csr(graph_of(csr), ia.LeannConfig(m=M, m0=M0, ef_construction=EFC, metric=metric), dimension=d)
    return idx.upload(0)


def f32_index(csr, rows, metric=COSINE):
    return bare_index(csr, rows.shape[1], metric).set_embeddings(rows)


@functools.lru_cache(maxsize=None)
def base_rows(n, d, seed):
    v = clustered_vectors(n, d, seed)
    v.setflags(write=False)
    return v


def same_answers(a, b):
    return a[2].tolist() == b[2].tolist() and a[0].tolist() == b[0].tolist() and bits(a[1]).tolist() == bits(b[1]).tolist()


# ---------------------------------------------------------------- the stand-alone entry points
def boundary_rows(e, d=40):
    x = boundary_set(e)
    pad = (-x.size) % d
    return np.concatenate([x, np.zeros(pad, np.float32)]).reshape(-1, d)


@pytest.mark.parametrize("e", EXPONENTS)
def test_quantiser_equals_the_definition_on_the_boundary_set(e):
    x = boundary_rows(e)
    want, _ = ia.quantize_fp8_e4m3(x, scale_exp=e)
    got, e_used = ia.quantize_fp8_e4m3_device(x, scale_exp=e)
    assert e_used == e and got.dtype == np.uint8 and got.shape == x.shape
    bad = np.nonzero(got != want)
    assert bad[0].size == 0, (e, x[bad][:5], got[bad][:5], want[bad][:5])
    # device buffers: aligned, and one float off alignment (the element-by-element path of a dense buffer)
    for shift in (0, 1):
        t = torch.zeros(x.size + 4, dtype=torch.float32, device="cuda:0")
        t[shift:shift + x.size] = torch.from_numpy(x.ravel().copy()).to("cuda:0")
        out = torch.full((x.size + 16,), 0xAA, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        e_used = ia.quantize_fp8_e4m3_device(scale_exp=e, device_ptr=t.data_ptr() + 4 * shift, out_ptr=out.data_ptr() + shift,
                                             n=x.shape[0], d=x.shape[1])
        o = out.cpu().numpy()
        assert e_used == e and (o[shift:shift + x.size].reshape(x.shape) == want).all()
        assert (o[:shift] == 0xAA).all() and (o[shift + x.size:] == 0xAA).all()  # nothing outside the n x d codes


@pytest.mark.parametrize("above", [False, True])
@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("d", [1, 15, 16, 17, 300, 768])
def test_automatic_exponent_at_the_edge_of_a_scale(d, n, above):
    """the top of the table lands exactly on 448 * 2^e, or on the float above it: e, or e + 1"""
    e = -3
    top = np.float32(448.0 * 2.0 ** e)
    x = base_rows(257, 768, 11)[:n, :d].copy()
    x *= np.float32(0.9) * top / np.abs(x).max()
    x[-1, -1] = -(np.nextafter(top, np.float32(np.inf)) if above else top)  # the last element of a ragged tail
    want, e_want = ia.quantize_fp8_e4m3(x)
    assert e_want == (e + 1 if above else e) == auto_scale_exp(float(np.abs(x).max()))
    got, e_got = ia.quantize_fp8_e4m3_device(x)
    assert e_got == e_want and (got == want).all()
    t = torch.from_numpy(x).to("cuda:0")
    out = torch.zeros(x.shape, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert ia.quantize_fp8_e4m3_device(device_ptr=t.data_ptr(), out_ptr=out.data_ptr(), n=n, d=d) == e_want
    assert (out.cpu().numpy() == want).all()


def test_automatic_exponent_of_zeros_infinities_and_a_nan():
    codes, e = ia.quantize_fp8_e4m3_device(np.zeros((5, 33), np.float32))
    assert e == -32 and not codes.any()
    x = base_rows(257, 768, 11)[:3, :40].copy()
    x[1, 7], x[2, 39] = np.inf, -np.inf
    codes, e = ia.quantize_fp8_e4m3_device(x)
    want, e_want = ia.quantize_fp8_e4m3(x)
    assert e == e_want == 32 and (codes == want).all() and codes[1, 7] == 0x7E and codes[2, 39] == 0xFE
    for scale_exp in (None, 0):
        x[0, 39] = np.nan
        with pytest.raises(ia.CoreError) as err:
            ia.quantize_fp8_e4m3_device(x, scale_exp=scale_exp)
        assert err.value.kind == "InvalidArgument" and "NaN" in str(err.value)
    # *out_scale_exp is not written on that way out
    lib = _ffi.lib()
    e_out = C.c_int32(77)
    out = np.zeros(x.shape, np.uint8)
    st = lib.isl_quantize_fp8_e4m3(x.ctypes.data, 3, 40, ia.FP8_SCALE_AUTO, out.ctypes.data, C.byref(e_out), 0, 0, None)
    assert lib.isl_status_name(st) == b"InvalidArgument" and e_out.value == 77


def test_round_bf16_equals_the_definition():
    big = np.array([0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x7F800000, 0xFF800000], np.uint32)  # to infinity, or not
    b = np.concatenate([random_patterns(), bf16_tie_patterns(), big])
    assert is_nan_bits(b).any()
    x = b.view(np.float32)
    want = ia.f32_to_bf16_bits(x)
    got = ia.round_bf16_device(x)
    bad = np.nonzero(got != want)[0]
    assert got.dtype == np.uint16 and bad.size == 0, ([hex(v) for v in b[bad[:5]]], got[bad[:5]], want[bad[:5]])
    assert got[-6:].tolist() == [0x7F80, 0xFF80, 0x7F80, 0x7F7F, 0x7F80, 0xFF80]
    # device buffers, rows of an odd length, one float off alignment
    n, d = 301, 77
    t = torch.from_numpy(x[:n * d + 1].copy()).to("cuda:0")
    out = torch.zeros(n * d, dtype=torch.int16, device="cuda:0")
    torch.cuda.synchronize()
    ia.round_bf16_device(device_ptr=t.data_ptr() + 4, out_ptr=out.data_ptr(), n=n, d=d)
    assert (out.cpu().numpy().view(np.uint16) == want[1:n * d + 1]).all()


# ---------------------------------------------------------------- a converted index against a twin
def narrowed(rows, target):
    """(host-narrowed array, scale_exp, images) of `rows` for a target: "bf16", "fp8" (automatic exponent) or
    "fp8x" (an explicit exponent one below the automatic one: the largest values saturate)"""
    if target == "bf16":
        b16 = ia.f32_to_bf16_bits(rows)
        return b16, 0, bf16_images(b16)
    codes, e = ia.quantize_fp8_e4m3(rows)
    if target == "fp8x":
        e -= 1
        codes, _ = ia.quantize_fp8_e4m3(rows, scale_exp=e)
        assert (codes & 0x7F).max() == 0x7E
    return codes, e, ia.fp8_e4m3_to_f32(codes, e)


def attach(idx, stored, e):
    return idx.set_embeddings_bf16(stored) if stored.dtype == np.uint16 else idx.set_embeddings_fp8(stored, e)


def convert(idx, target, e):
    return idx.convert_rows("bf16") if target == "bf16" else idx.convert_rows("fp8", scale_exp=e if target == "fp8x" else None)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("target", ["bf16", "fp8", "fp8x"])
@pytest.mark.parametrize("d", [40, 768])
def test_converted_index_equals_its_twin_and_the_oracle(orc, d, target, metric):
    rows = base_rows(900, d, 31)
    stored, e, images = narrowed(rows, target)
    csr = orc.leann_build(images, m=M, m0=M0, ef_construction=EFC, metric=int(metric))
    q = clustered_vectors(24, d, 32)
    idx = f32_index(csr, rows, metric)
    idx.search_batch(q, 10, 48)  # the lanes are made under the f32 rows and serve the converted ones
    convert(idx, target, e)
    twin = attach(bare_index(csr, d, metric), stored, e)
    assert idx.row_storage() == twin.row_storage() and idx.row_storage()["scale_exp"] == e
    got = idx.read_rows()  # d = 40: rows at a padded pitch on the device, dense here
    assert got.dtype == stored.dtype and got.shape == stored.shape and (got == stored).all()
    assert_parity(orc, idx, csr, images, q, 10, 48, metric)
    assert_parity(orc, twin, csr, images, q, 10, 48, metric)


# ---------------------------------------------------------------- chains
@functools.lru_cache(maxsize=None)
def chain_case(orc):
    rows = base_rows(900, 40, 31)
    csr = orc.leann_build(rows, m=M, m0=M0, ef_construction=EFC, metric=int(COSINE))
    return rows, csr


def test_chains_compose_through_the_images(orc):
    rows, csr = chain_case(orc)
    b16 = ia.f32_to_bf16_bits(rows)
    # f32 -> bf16 -> fp8 = quantize(images of the bf16 rows)
    idx = f32_index(csr, rows).convert_rows("bf16")
    assert (idx.read_rows() == b16).all()
    idx.convert_rows("fp8")
    codes, e = ia.quantize_fp8_e4m3(bf16_images(b16))
    assert idx.row_storage()["scale_exp"] == e and (idx.read_rows() == codes).all()
    # fp8 -> f32: the images, bit for bit
    images = ia.fp8_e4m3_to_f32(codes, e)
    idx.convert_rows("f32")
    assert idx.row_storage() == f32_index(csr, images).row_storage()
    assert bits(idx.read_rows()).tolist() == bits(images).tolist()
    # fp8 -> f32 -> fp8 under the same exponent: the same codes
    idx.convert_rows("fp8", scale_exp=e)
    assert (idx.read_rows() == codes).all() and idx.row_storage()["scale_exp"] == e
    # fp8 -> bf16 -> f32: the images again, which are exact in bf16
    idx.convert_rows("bf16")
    assert bits(bf16_images(idx.read_rows())).tolist() == bits(images).tolist()
    idx.convert_rows("f32")
    assert bits(idx.read_rows()).tolist() == bits(images).tolist()
    # a sub-range, its end, and what lies past it
    assert bits(idx.read_rows(17, 101)).tolist() == bits(images[17:118]).tolist()
    assert bits(idx.read_rows(899)).tolist() == bits(images[899:]).tolist() and idx.read_rows(900).shape == (0, 40)
    for first, count, node in ((0, 901, 900), (899, 2, 900), (905, 1, 905)):
        with pytest.raises(ia.CoreError) as err:
            idx.read_rows(first, count)
        assert err.value.kind == "NodeNotFound" and err.value.node == node
    # every code survives a round trip through f32 under every scale the tests use, the zeros' signs included
    finite = np.array([c for c in range(256) if c not in (0x7F, 0xFF)], np.uint8)
    all_codes = np.resize(finite, (900, 40))
    for e in (-32, 5, 32):
        idx = attach(bare_index(csr, 40), all_codes, e).convert_rows("f32")
        assert bits(idx.read_rows()).tolist() == bits(ia.fp8_e4m3_to_f32(all_codes, e)).tolist()
        assert (idx.convert_rows("fp8", scale_exp=e).read_rows() == all_codes).all()


def test_same_type_is_a_no_op(orc):
    rows, csr = chain_case(orc)
    idx = f32_index(csr, rows)
    assert bits(idx.convert_rows("f32").read_rows()).tolist() == bits(rows).tolist()
    assert bits(idx.convert_rows("f32", scale_exp=99).read_rows()).tolist() == bits(rows).tolist()  # read for fp8 only
    codes, e = ia.quantize_fp8_e4m3(rows)
    idx.convert_rows("fp8")
    before = idx.row_storage()
    for same in (None, e):
        assert (idx.convert_rows("fp8", scale_exp=same).read_rows() == codes).all() and idx.row_storage() == before
    idx.convert_rows("bf16")
    b16 = idx.read_rows()
    assert (idx.convert_rows("bf16").read_rows() == b16).all()


# ---------------------------------------------------------------- the lifecycle the widening buys
def test_an_fp8_index_widens_takes_rows_gives_rows_up_and_narrows_again(orc):
    rows, _ = chain_case(orc)
    n, d = rows.shape
    codes, e = ia.quantize_fp8_e4m3(rows[:n - 8])
    images = ia.fp8_e4m3_to_f32(codes, e)
    csr = orc.leann_build(images, m=M, m0=M0, ef_construction=EFC, metric=int(COSINE))
    idx = attach(bare_index(csr, d), codes, e)
    with pytest.raises(ia.CoreError):
        idx.insert(rows[n - 8:])  # frozen while the rows are fp8
    idx.convert_rows("f32")
    assert idx.insert(rows[n - 8:]) == n - 8 and len(idx) == n
    gone = [5, 300, n - 3]
    remap = idx.remove(gone)
    assert len(idx) == n - 3 and sorted(np.nonzero(remap == ia.REMOVED)[0].tolist()) == gone
    idx.convert_rows("fp8", scale_exp=e)
    assert idx.row_storage()["dtype"] == 2 and idx.row_storage()["scale_exp"] == e
    got = idx.read_rows()
    keep = np.array([i for i in range(n - 8) if i not in gone])
    assert got.shape == (n - 3, d) and (got[remap[keep].astype(np.int64)] == codes[keep]).all()  # untouched survivors
    new = np.array([i for i in range(n - 8, n) if i not in gone])
    assert (got[remap[new].astype(np.int64)] == ia.quantize_fp8_e4m3(rows[new], scale_exp=e)[0]).all()
    twin = ia.LeannIndex.from_bytes(idx.to_bytes()).upload(0).set_embeddings_fp8(got, e)
    q = clustered_vectors(24, d, 33)
    got_answers, got_stats = idx.search_batch(q, 10, 48), idx.last_stats()
    want_answers, want_stats = twin.search_batch(q, 10, 48), twin.last_stats()
    assert same_answers(got_answers, want_answers)
    assert got_stats["evals"] == want_stats["evals"] > 0 and got_stats["expansions"] == want_stats["expansions"]


# ---------------------------------------------------------------- entry seeds
def test_entry_seeds_follow_the_rows(orc):
    rows, csr = chain_case(orc)
    idx = f32_index(csr, rows)
    seeds = idx.select_entry_seeds(16)
    assert len(seeds) == 16
    idx.convert_rows("bf16")
    assert idx.entry_seeds().tolist() == seeds.tolist()
    twin = bare_index(csr, rows.shape[1]).set_embeddings_bf16(ia.f32_to_bf16_bits(rows)).set_entry_seeds(seeds)
    q = clustered_vectors(48, rows.shape[1], 34)
    assert idx.pick_entries(q).tolist() == twin.pick_entries(q).tolist()
    assert same_answers(idx.search_batch(q, 10, 48), twin.search_batch(q, 10, 48))
    idx.convert_rows("f32")
    assert idx.entry_seeds().tolist() == seeds.tolist()
    idx.convert_rows("fp8")
    assert idx.entry_seeds().size == 0  # an fp8 index carries none
    idx.convert_rows("f32")
    assert idx.entry_seeds().size == 0


# ---------------------------------------------------------------- refusals
def refused(call, kind, word):
    with pytest.raises(ia.CoreError) as err:
        call()
    assert err.value.kind == kind and word in str(err.value), str(err.value)


def test_refusals_leave_the_index_as_it_was(orc):
    rows, csr = chain_case(orc)
    d = rows.shape[1]
    q = clustered_vectors(16, d, 35)
    # fp8 -> fp8 under another exponent
    codes, e = ia.quantize_fp8_e4m3(rows)
    idx = attach(bare_index(csr, d), codes, e)
    want = idx.search_batch(q, 10, 48)
    refused(lambda: idx.convert_rows("fp8", scale_exp=e + 1), "Unsupported", "scale_exp")
    assert (idx.read_rows() == codes).all() and idx.row_storage()["scale_exp"] == e
    assert same_answers(idx.search_batch(q, 10, 48), want)
    # a NaN row with target fp8, automatic and explicit; the other targets take it
    bad = rows.copy()
    bad[899, 39] = np.nan
    idx = f32_index(csr, bad)
    idx.set_entry_seeds([3, 4])
    want = idx.search_batch(q, 10, 48)
    for scale_exp in (None, 0):
        refused(lambda: idx.convert_rows("fp8", scale_exp=scale_exp), "InvalidArgument", "NaN")
        assert idx.row_storage()["dtype"] == 0 and bits(idx.read_rows()).tolist() == bits(bad).tolist()
        assert idx.entry_seeds().tolist() == [3, 4] and same_answers(idx.search_batch(q, 10, 48), want)
    assert (idx.convert_rows("bf16").read_rows() == ia.f32_to_bf16_bits(bad)).all()
    # an index without rows
    idx = bare_index(csr, d)
    refused(lambda: idx.convert_rows("bf16"), "Unsupported", "resident")
    refused(lambda: idx.read_rows(), "Unsupported", "resident")
    # the core index of an HnswGraph: its rows keep their type (they can be read)
    lib = _ffi.lib()
    hnsw = ia.HnswGraph.build(rows[:300], m=M, m0=M0, ef_construction=EFC)
    core = C.c_void_p.from_address(hnsw._h.value)  # isl_hnsw's first member: the layer-0 isl_index
    want_h = hnsw.search(q[0], 5, 32)
    for dtype in (1, 2):
        assert lib.isl_status_name(lib.isl_index_convert_rows(core, dtype, ia.FP8_SCALE_AUTO)) == b"Unsupported"
        assert b"HnswGraph" in lib.isl_last_error_message()
    out = np.zeros((300, d), np.float32)
    assert lib.isl_index_read_rows(core, 0, 300, out.ctypes.data, 0) == 0 and bits(out).tolist() == bits(rows[:300]).tolist()
    assert hnsw.row_storage()["dtype"] == 0 and hnsw.search(q[0], 5, 32) == want_h


def test_refused_on_the_recompute_provider(orc):
    from test_gpu_encoder import _recompute_case

    cfg, enc, tok, lens, emb = _recompute_case(orc, n=400, seed=9)
    csr = orc.leann_build(emb, m=6, m0=12, ef_construction=30, levels=np.zeros(400, np.uint64))
    idx = bare_index(csr, emb.shape[1]).set_recompute_provider(enc, tok, lens)
    q = emb[::41] + np.float32(0.01)
    want = idx.search_batch(q, 5, 32)
    for target in ("f32", "bf16", "fp8"):
        refused(lambda: idx.convert_rows(target), "Unsupported", "recompute")
    refused(lambda: idx.read_rows(), "Unsupported", "recompute")
    assert same_answers(idx.search_batch(q, 5, 32), want)


def test_refused_while_a_search_is_in_flight(orc):
    rows, csr = chain_case(orc)
    d = rows.shape[1]
    idx = f32_index(csr, rows)
    idx.prepare(256, 64, 10, 2)
    qh = clustered_vectors(256, d, 36)
    want = idx.search_batch(qh, 10, 64)
    q = torch.from_numpy(qh).cuda()
    ids = torch.zeros((256, 10), dtype=torch.int64, device="cuda")
    dist = torch.zeros((256, 10), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(256, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    tok = idx.search_batch_device_async(q.data_ptr(), 256, d, 10, 64, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
    refused(lambda: idx.convert_rows("bf16"), "SearchError", "in flight")
    assert bits(idx.read_rows(0, 10)).tolist() == bits(rows[:10]).tolist()  # reading needs no idle lane
    idx.wait(tok)
    assert ids.cpu().numpy().astype(np.uint64).tolist() == want[0].tolist()
    assert idx.row_storage()["dtype"] == 0 and bits(idx.read_rows()).tolist() == bits(rows).tolist()
    idx.convert_rows("bf16")  # fine once nothing is in flight
    assert (idx.read_rows() == ia.f32_to_bf16_bits(rows)).all()
