"""fp8 e4m3 rows without a device: the enum and the two entry points, the scale_exp range, the layout rule of
islands_amd/csrc/row_table_plan.hpp for the one-byte type (tests/cpp/row_table_fp8_dump.cpp against a Python
restatement), the code table written from the format's definition, and the numpy quantiser.  torch is only
the cross-check."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import islands_amd as ia
from islands_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_CODES = np.arange(256, dtype=np.uint8)
NAN_CODES = [0x7F, 0xFF]
FINITE = np.array([c for c in range(256) if c not in NAN_CODES], dtype=np.uint8)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def torch_table():
    return torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float32).numpy()


def test_enum_abi_version_and_exports():
    hdr = open(os.path.join(ROOT, "include", "islands_amd.h")).read()
    assert re.search(r"ISL_DTYPE_F32 = 0, ISL_DTYPE_BF16 = 1, ISL_DTYPE_FP8_E4M3 = 2\b", hdr)
    assert re.search(r"#define ISL_ABI_VERSION 3\b", hdr)
    assert ia.DTYPE_FP8_E4M3 == 2
    lib = _ffi.lib()
    assert lib.isl_abi_version() == 3  # additions only
    for name in ("isl_set_embeddings_fp8", "isl_index_row_storage"):
        assert hasattr(lib, name) and name in _ffi.SIGNATURES


def small_index():
    g = ia.CsrGraph()
    g.add_node([1], 0)
    g.add_node([0], 0)
    return ia.LeannIndex.from_csr(g, dimension=16)


@pytest.mark.parametrize("scale_exp", [33, -33, 1000, -(2 ** 31)])
def test_scale_exp_outside_the_range_is_an_invalid_argument(scale_exp):
    """Answered before any device call: this runs without a GPU, on an index that was never uploaded."""
    idx = small_index()
    with pytest.raises(ia.CoreError) as e:
        idx.set_embeddings_fp8(np.zeros((2, 16), dtype=np.uint8), scale_exp=scale_exp)
    assert e.value.kind == "InvalidArgument" and "scale_exp" in str(e.value)


def test_checks_keep_the_order_of_set_embeddings():
    idx = small_index()
    lib = _ffi.lib()
    codes = np.zeros((2, 16), dtype=np.uint8)
    p = codes.ctypes.data
    assert lib.isl_status_name(lib.isl_set_embeddings_fp8(idx._h, None, 2, 16, 0, 0)) == b"InvalidArgument"
    assert lib.isl_status_name(lib.isl_set_embeddings_fp8(idx._h, p, 0, 16, 99, 0)) == b"EmptyCollection"
    assert lib.isl_status_name(lib.isl_set_embeddings_fp8(idx._h, p, 2, 0, 99, 0)) == b"InvalidArgument"
    assert b"scale_exp" in lib.isl_last_error_message()  # the type's own check stands where the dtype check does
    assert lib.isl_status_name(lib.isl_set_embeddings_fp8(idx._h, p, 2, 0, 0, 0)) == b"InvalidArgument"
    assert b"dimension" in lib.isl_last_error_message()
    # in range and well-formed: the next check is the upload, as for every other row type
    for call in (lambda: lib.isl_set_embeddings_fp8(idx._h, p, 2, 16, -32, 0),
                 lambda: lib.isl_set_embeddings_fp8(idx._h, p, 2, 16, 32, 0),
                 lambda: lib.isl_set_embeddings(idx._h, p, 2, 16, 2, 0)):
        assert lib.isl_status_name(call()) == b"Device"
    assert lib.isl_status_name(lib.isl_set_embeddings(idx._h, p, 2, 16, 3, 0)) == b"InvalidArgument"
    # nothing attached: the accessor says so
    assert idx.row_storage() == {"dtype": 0, "scale_exp": 0, "block_bytes": 0}
    with pytest.raises(TypeError):
        idx.set_embeddings_fp8(np.zeros((2, 16), dtype=np.float32))


def ceil_to(d, m):
    return (d + m - 1) // m * m


def test_layout_rule_of_one_byte_rows():
    src = os.path.join(ROOT, "tests", "cpp", "row_table_fp8_dump.cpp")
    exe = os.path.join(ROOT, "islands_amd", "lib", "row_table_fp8_dump")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", src, "-o", exe])
    got = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    want = []
    for d in (1, 15, 16, 17, 768, 4096):
        stride = ceil_to(d, 16)  # a row starts 16-byte aligned, an element is one byte
        assert stride % 16 == 0 and stride - d < 16
        want.append(f"layout 2 {d} -> 1 {stride} 1024")  # 1 KiB of slack = 1024 elements
        for n in (1, 1000, 10 ** 7):
            want.append(f"alloc 2 {d} {n} -> {n * stride + 1024}")
    want.append("scale_exp -32 32")
    assert got == want


def test_code_table_is_the_formats_definition():
    t = ia.fp8_e4m3_to_f32(ALL_CODES)
    ref = torch_table()
    assert t.dtype == np.float32 and t.shape == (256,)
    assert np.isnan(t[NAN_CODES]).all() and np.isnan(ref[NAN_CODES]).all() and not np.isnan(t[FINITE]).any()
    assert bits(t[FINITE]).tolist() == bits(ref[FINITE]).tolist()
    assert t[0x7E] == 448.0 and t[0xFE] == -448.0 and t[0x01] == 2.0 ** -9 and t[0x08] == 2.0 ** -6
    assert bits(t[[0x00, 0x80]]).tolist() == [0, 0x80000000]
    assert ia.fp8_e4m3_to_f32(ALL_CODES.reshape(16, 16)).shape == (16, 16)


@pytest.mark.parametrize("scale_exp", [-32, -7, 0, 5, 32])
def test_images_are_exact_and_normal(scale_exp):
    img = ia.fp8_e4m3_to_f32(FINITE, scale_exp)
    exact = torch_table()[FINITE].astype(np.float64) * 2.0 ** scale_exp
    assert (img.astype(np.float64) == exact).all()  # a power-of-two multiple: nothing rounds
    tiny = np.finfo(np.float32).tiny
    assert ((img == 0) | (np.abs(img) >= tiny)).all() and np.isfinite(img).all()
    assert np.abs(img[img != 0]).min() == np.float32(2.0 ** (scale_exp - 9))
    for bad in (33, -33):
        with pytest.raises(ValueError):
            ia.fp8_e4m3_to_f32(FINITE, bad)


def sample_rows(seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((64, 257)).astype(np.float32) * rng.choice([1e-3, 1.0, 40.0], size=(64, 1)).astype(np.float32)
    x[0, :8] = [0.0, -0.0, 1e-12, -1e-12, 3.0, -3.0, 17.5, 0.3]
    return x


def test_quantiser_rounds_to_nearest_ties_to_even():
    x = sample_rows()
    codes, e = ia.quantize_fp8_e4m3(x)
    assert codes.dtype == np.uint8 and codes.shape == x.shape
    assert not np.isin(codes, NAN_CODES).any()
    y = x.astype(np.float64) * 2.0 ** -e
    pos = torch_table()[:0x7F].astype(np.float64)  # codes 0x00 .. 0x7E: the 127 non-negative values, ascending
    assert pos[0] == 0 and (np.diff(pos) > 0).all()
    got = ia.fp8_e4m3_to_f32(codes).astype(np.float64)
    # nearest: no representable value is closer
    err = np.abs(got - y)
    best = np.abs(np.abs(y)[..., None] - pos).min(axis=-1)
    assert (err == best).all()
    assert (np.signbit(got) == np.signbit(x)).all()
    # exact midpoints of neighbouring values go to the even code, on both sides of zero
    mid = (pos[:-1] + pos[1:]) / 2
    lo_code = np.arange(pos.size - 1)  # the code of pos[i] is i
    want = np.where(lo_code % 2 == 0, lo_code, lo_code + 1).astype(np.uint8)
    for sign, bit in ((1.0, 0), (-1.0, 0x80)):
        rows = np.concatenate([[sign * 448.0], sign * mid]).astype(np.float32)[None, :]  # 448 pins scale_exp = 0
        assert (rows.astype(np.float64)[0, 1:] == sign * mid).all()  # the midpoints are float32 values
        c, e0 = ia.quantize_fp8_e4m3(rows)
        assert e0 == 0 and c[0, 0] == 0x7E | bit
        assert (c[0, 1:] == (want | bit)).all()


def test_quantiser_error_bound_saturation_and_torch():
    x = sample_rows(1)
    codes, e = ia.quantize_fp8_e4m3(x)
    y = x.astype(np.float64) * 2.0 ** -e
    got = ia.fp8_e4m3_to_f32(codes).astype(np.float64)
    normal = np.abs(y) >= 2.0 ** -6
    # three mantissa bits, round to nearest: half a unit in the last place of a value in [1, 2) is 2^-4
    assert (np.abs(got - y)[normal] <= 2.0 ** -4 * np.abs(y)[normal]).all()
    assert (np.abs(got - y)[~normal] <= 2.0 ** -10).all()  # subnormals: half of 2^-9
    # the clamped torch cast agrees code for code (a bare cast turns values past 448 into NaN: clamp first)
    t = torch.from_numpy((y).astype(np.float32)).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert (codes == t).all()
    # past the largest exponent the magnitudes saturate
    big = np.array([[448.0 * 2.0 ** 32, -3e30, 1e38, -np.inf, 1.0, 448.0 * 2.0 ** 32 * 1.01]], dtype=np.float32)
    c, e = ia.quantize_fp8_e4m3(big)
    assert e == 32 and c[0].tolist()[:4] == [0x7E, 0xFE, 0x7E, 0xFE] and c[0, 5] == 0x7E
    assert ia.fp8_e4m3_to_f32(c, e)[0, 0] == np.float32(448.0 * 2.0 ** 32)


@pytest.mark.parametrize("top", [1e-6, 0.04, 1.0, 448.0, 1e6])
def test_scale_exp_is_the_smallest_that_fits(top):
    rng = np.random.default_rng(7)
    x = (rng.random((5, 33), dtype=np.float32) * 2 - 1) * np.float32(top)
    x[2, 5] = -np.float32(top)
    codes, e = ia.quantize_fp8_e4m3(x)
    m = float(np.abs(x).max())
    assert -32 <= e <= 32
    assert m * 2.0 ** -e <= 448.0
    assert e == -32 or m * 2.0 ** -(e - 1) > 448.0
    assert np.abs(ia.fp8_e4m3_to_f32(codes, e)).max() <= 448.0 * 2.0 ** e
    if top == 448.0:
        assert e == 0 and codes[2, 5] == 0xFE


def test_quantiser_edges():
    c, e = ia.quantize_fp8_e4m3(np.zeros((3, 4), dtype=np.float32))
    assert e == -32 and not c.any()
    with pytest.raises(ValueError):
        ia.quantize_fp8_e4m3(np.array([[1.0, np.nan]], dtype=np.float32))
