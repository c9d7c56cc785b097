"""Row conversions without a device: the host definition in islands_amd/csrc/row_convert_plan.hpp (through
tests/cpp/row_convert_dump.cpp, g++ alone, and once more under AddressSanitizer + UBSan) against the Python
definitions ia.quantize_fp8_e4m3(x, scale_exp=e) and ia.f32_to_bf16_bits, torch's CPU cast as a cross-check of the
bf16 rounding, the four new symbols, and every argument check that is answered before a device call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import islands_amd as ia
from islands_amd import _ffi
from _convert_ref import (EXPONENTS, F32_DENORM_MIN, F32_MAX, auto_scale_exp, bf16_tie_patterns, boundary_set,
                          is_nan_bits, random_patterns)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "row_convert_dump.cpp")
NEW_SYMBOLS = ("isl_quantize_fp8_e4m3", "isl_round_bf16", "isl_index_convert_rows", "isl_index_read_rows")
AUTO = -2 ** 31


def build_dump(name, *flags):
    exe = os.path.join(ROOT, "islands_amd", "lib", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", *flags, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = build_dump("row_convert_dump")
    tmp = tmp_path_factory.mktemp("row_convert")

    def run(mode, bits, *args, exe=exe):
        src, dst = str(tmp / "in.bin"), str(tmp / "out.bin")
        np.ascontiguousarray(bits, dtype=np.uint32).tofile(src)
        pr = subprocess.run([exe, mode, *[str(a) for a in args], src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                            timeout=120)
        assert pr.returncode == 0, pr.stdout.decode(errors="replace")[-3000:]
        return np.fromfile(dst, dtype={"e4m3": np.uint8, "bf16": np.uint16, "scale": np.int32}[mode])

    return run


def f32_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def finite_random():
    b = random_patterns()
    return b[~is_nan_bits(b)]


def scale_tops():
    """(float32 tops, what the Python loop gives for each)"""
    tops = []
    for e in range(-33, 34):
        t = np.float32(448.0 * 2.0 ** e)
        assert float(t) == 448.0 * 2.0 ** e
        tops += [t, np.nextafter(t, np.float32(np.inf))]
    tops += [np.float32(0.0), F32_DENORM_MIN, F32_MAX, np.float32(np.inf)]
    tops = np.array(tops, dtype=np.float32)
    return tops, [auto_scale_exp(float(t)) for t in tops]


# ---------------------------------------------------------------- the definitions
@pytest.mark.parametrize("e", EXPONENTS)
def test_narrow_e4m3_is_the_python_definition(dump, e):
    for x in (boundary_set(e), finite_random().view(np.float32)):
        want, e_used = ia.quantize_fp8_e4m3(x, scale_exp=e)
        assert e_used == e
        got = dump("e4m3", f32_bits(x), e)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (e, x[bad[:5]], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("e", EXPONENTS)
def test_boundary_set_holds_what_it_says(e):
    x = boundary_set(e)
    codes, _ = ia.quantize_fp8_e4m3(x, scale_exp=e)
    assert set(codes.tolist()) == set(range(0x7F)) | set(range(0x80, 0xFF))  # every finite code of both signs
    for v, c in ((448.0, 0x7E), (464.0, 0x7E), (2.0 ** -10, 0x00), (2.0 ** -9, 0x01), (np.inf, 0x7E)):
        one = np.array([v * 2.0 ** e, -v * 2.0 ** e], dtype=np.float32)
        assert ia.quantize_fp8_e4m3(one, scale_exp=e)[0].tolist() == [c, c | 0x80]
    assert ia.quantize_fp8_e4m3(np.array([-0.0], np.float32), scale_exp=e)[0].tolist() == [0x80]


def test_the_explicit_exponent_is_the_default_given():
    x = np.random.default_rng(3).standard_normal((7, 33)).astype(np.float32) * np.float32(9.0)
    codes, e = ia.quantize_fp8_e4m3(x)
    again, e2 = ia.quantize_fp8_e4m3(x, scale_exp=e)
    assert e2 == e and (again == codes).all()
    for bad in (33, -33):
        with pytest.raises(ValueError):
            ia.quantize_fp8_e4m3(x, scale_exp=bad)
    with pytest.raises(ValueError):
        ia.quantize_fp8_e4m3(np.array([np.nan], np.float32), scale_exp=0)


def test_narrow_bf16_is_the_python_definition_and_torchs_cast(dump):
    b = np.concatenate([random_patterns(), bf16_tie_patterns()])
    want = ia.f32_to_bf16_bits(b.view(np.float32))
    assert want.dtype == np.uint16 and want.shape == b.shape
    got = dump("bf16", b)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, ([hex(v) for v in b[bad[:5]]], got[bad[:5]], want[bad[:5]])
    ok = ~is_nan_bits(b)
    t = torch.from_numpy(b[ok].view(np.float32).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert (want[ok] == t).all()
    # a NaN keeps its sign and comes out quiet, whatever its payload
    nan = want[~ok]
    assert nan.size and ((nan & 0x7FC0) == 0x7FC0).all() and ((nan >> 15) == (b[~ok] >> 31)).all()
    # the largest finite values round to infinity, a tie goes to the even neighbour
    assert ia.f32_to_bf16_bits(np.array([0x7F7FFFFF, 0xFF7F8000, 0x3F808000, 0x3F818000], np.uint32).view(np.float32)
                               ).tolist() == [0x7F80, 0xFF80, 0x3F80, 0x3F82]
    assert ia.f32_to_bf16_bits(np.ones((3, 5), np.float32)).shape == (3, 5)


def test_scale_exp_for_is_the_python_loop(dump):
    tops, want = scale_tops()
    assert dump("scale", f32_bits(tops)).tolist() == want
    assert want[-4:] == [-32, -32, 32, 32] and want[:4] == [-32, -32, -32, -31]
    # ... and the loop is what the quantiser runs
    for t, w in zip(tops[::7], want[::7]):
        assert ia.quantize_fp8_e4m3(np.array([t, -t / 2], np.float32))[1] == w


def test_plan_arithmetic():
    exe = build_dump("row_convert_dump")
    got = subprocess.run([exe, "plan"], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    want = [f"chunks {d} -> {(d + 15) // 16}" for d in (1, 15, 16, 17, 300, 768, 7680000000)]
    want += [f"grid {n} -> {min(max((n + 255) // 256, 1), 2048)}" for n in (0, 1, 256, 257, 524288, 524289, 480000000)]
    tops = f32_bits([448.0 * 2.0 ** e for e in (-32, 0, 32)])
    want.append("lane 16 top " + " ".join(f"{int(t):08x}" for t in tops))
    assert got == want


def test_dump_is_clean_under_address_and_ub_sanitizers(dump):
    """a host program with its own main, instrumented and run directly"""
    exe = build_dump("row_convert_dump_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                     "-fno-omit-frame-pointer")
    b = np.concatenate([f32_bits(boundary_set(e)) for e in EXPONENTS] + [random_patterns()[:1 << 16], bf16_tie_patterns()])
    ok = ~is_nan_bits(b)
    for e in EXPONENTS:
        assert (dump("e4m3", b[ok], e, exe=exe) == ia.quantize_fp8_e4m3(b[ok].view(np.float32), scale_exp=e)[0]).all()
        assert ((dump("e4m3", b[~ok], e, exe=exe) & 0x7F) == 0x7F).all()  # a NaN has no code: the format's own NaN
    assert (dump("bf16", b, exe=exe) == ia.f32_to_bf16_bits(b.view(np.float32))).all()
    tops, want = scale_tops()
    assert dump("scale", f32_bits(tops), exe=exe).tolist() == want


# ---------------------------------------------------------------- the ABI
def test_header_exports_and_abi_version():
    hdr = open(os.path.join(ROOT, "include", "islands_amd.h")).read()
    assert re.search(r"#define ISL_ABI_VERSION 3\b", hdr) and "#define ISL_FP8_SCALE_AUTO INT32_MIN" in hdr
    lib = _ffi.lib()
    assert lib.isl_abi_version() == 3  # additions only
    for name in NEW_SYMBOLS:
        assert re.search(r"isl_status %s\(" % name, hdr) and hasattr(lib, name) and name in _ffi.SIGNATURES, name
        assert getattr(lib, name).restype is C.c_int32
    assert [len(getattr(lib, n).argtypes) for n in NEW_SYMBOLS] == [9, 7, 3, 5]
    assert ia.FP8_SCALE_AUTO == AUTO
    for name in ("f32_to_bf16_bits", "quantize_fp8_e4m3_device", "round_bf16_device"):
        assert name in ia.__all__
    hpp = open(os.path.join(ROOT, "include", "islands_amd.hpp")).read()
    assert "void convert_rows(int32_t dtype" in hpp and "read_rows(uint64_t first, uint64_t count) const" in hpp


def status(st):
    lib = _ffi.lib()
    return lib.isl_status_name(st).decode(), lib.isl_last_error_message().decode()


def ring_index():
    g = ia.CsrGraph()
    for i in range(6):
        g.add_node([(i + 1) % 6, (i + 5) % 6], 0)
    return ia.LeannIndex.from_csr(g, dimension=16)


def test_stand_alone_calls_check_their_arguments_before_any_device_call():
    lib = _ffi.lib()
    x = np.ones((2, 16), np.float32)
    codes = np.full((2, 16), 0xAA, np.uint8)
    half = np.full((2, 16), 0xAAAA, np.uint16)
    e = C.c_int32(77)
    px, pc, ph = x.ctypes.data, codes.ctypes.data, half.ctypes.data
    # NULL buffers with n * d > 0
    for rows, out in ((None, pc), (px, None)):
        kind, msg = status(lib.isl_quantize_fp8_e4m3(rows, 2, 16, 0, out, C.byref(e), 0, 0, None))
        assert kind == "InvalidArgument" and "NULL" in msg
    for rows, out in ((None, ph), (px, None)):
        kind, msg = status(lib.isl_round_bf16(rows, 2, 16, out, 0, 0, None))
        assert kind == "InvalidArgument" and "NULL" in msg
    # an unknown mem
    for mem in (2, -1):
        kind, msg = status(lib.isl_quantize_fp8_e4m3(px, 2, 16, 0, pc, C.byref(e), mem, 0, None))
        assert kind == "InvalidArgument" and "mem" in msg
        kind, msg = status(lib.isl_round_bf16(px, 2, 16, ph, mem, 0, None))
        assert kind == "InvalidArgument" and "mem" in msg
    # an exponent that is neither AUTO nor in range
    for bad in (33, -33, 1000, AUTO + 1):
        kind, msg = status(lib.isl_quantize_fp8_e4m3(px, 2, 16, bad, pc, C.byref(e), 0, 0, None))
        assert kind == "InvalidArgument" and "scale_exp" in msg
    assert e.value == 77 and (codes == 0xAA).all() and (half == 0xAAAA).all()  # nothing was written
    # nothing to do: ISL_OK without a device, even one that does not exist
    for n, d in ((0, 16), (2, 0), (0, 0)):
        assert status(lib.isl_quantize_fp8_e4m3(None, n, d, AUTO, None, C.byref(e), 0, 99, None))[0] == "Ok"
        assert e.value == -32
        assert status(lib.isl_quantize_fp8_e4m3(None, n, d, 7, None, C.byref(e), 0, 99, None))[0] == "Ok"
        assert e.value == 7
        assert status(lib.isl_quantize_fp8_e4m3(None, n, d, AUTO, None, None, 1, 99, None))[0] == "Ok"
        assert status(lib.isl_round_bf16(None, n, d, None, 0, 99, None))[0] == "Ok"
    codes0, e0 = ia.quantize_fp8_e4m3_device(np.zeros((0, 16), np.float32), device=99)
    assert codes0.shape == (0, 16) and codes0.dtype == np.uint8 and e0 == -32
    assert ia.round_bf16_device(np.zeros((0, 16), np.float32), device=99).shape == (0, 16)
    # well-formed work for a device that does not exist: the device error, not a host fall-back
    with pytest.raises(ia.CoreError) as err:
        ia.quantize_fp8_e4m3_device(x, device=4096)
    assert err.value.kind == "Device"
    with pytest.raises(ia.CoreError) as err:
        ia.round_bf16_device(x, device=4096)
    assert err.value.kind == "Device"


def test_index_calls_check_in_their_order():
    lib = _ffi.lib()
    full = ring_index()
    blob = full.to_bytes()
    out = np.full((6, 16), 7.0, np.float32)
    po = out.ctypes.data
    hnsw = ia.HnswGraph.build(np.zeros((0, 0), np.float32), m=4, m0=8, ef_construction=16)
    core = C.c_void_p.from_address(hnsw._h.value)  # isl_hnsw's first member: the layer-0 isl_index
    # 1. NULL idx, an unknown dtype, target fp8 with an exponent out of range -- before the handle is looked at
    assert status(lib.isl_index_convert_rows(None, 0, 0))[0] == "InvalidArgument"
    for handle in (full._h, core):
        for dtype in (3, -1, 99):
            kind, msg = status(lib.isl_index_convert_rows(handle, dtype, 0))
            assert kind == "InvalidArgument" and "dtype" in msg
        for bad in (33, -33, AUTO + 1):
            kind, msg = status(lib.isl_index_convert_rows(handle, 2, bad))
            assert kind == "InvalidArgument" and "scale_exp" in msg
    # (scale_exp is read for fp8 only: any value passes this check for the other types)
    # 2. the core index of an HnswGraph -- before its missing rows are noticed
    for dtype, e in ((0, 0), (1, 12345), (2, AUTO), (2, 5)):
        kind, msg = status(lib.isl_index_convert_rows(core, dtype, e))
        assert kind == "Unsupported" and "HnswGraph" in msg
    # 3. no resident rows (never uploaded, nothing attached)
    for dtype, e in ((0, 0), (1, 12345), (2, AUTO), (2, -32), (2, 32)):
        kind, msg = status(lib.isl_index_convert_rows(full._h, dtype, e))
        assert kind == "Unsupported" and "resident" in msg
    for kind_name in ("f32", "bf16", "fp8"):
        with pytest.raises(ia.CoreError) as err:
            full.convert_rows(kind_name)
        assert err.value.kind == "Unsupported"
    with pytest.raises(ValueError):
        full.convert_rows("int8")
    with pytest.raises(ia.CoreError) as err:
        full.convert_rows("fp8", scale_exp=40)
    assert err.value.kind == "InvalidArgument"
    # isl_index_read_rows: NULL arguments and an unknown mem, then the residency check of the conversion
    assert status(lib.isl_index_read_rows(None, 0, 1, po, 0))[0] == "InvalidArgument"
    assert status(lib.isl_index_read_rows(full._h, 0, 1, None, 0))[0] == "InvalidArgument"
    kind, msg = status(lib.isl_index_read_rows(full._h, 0, 1, po, 5))
    assert kind == "InvalidArgument" and "mem" in msg
    for first, count in ((0, 1), (0, 0), (100, 1)):
        kind, msg = status(lib.isl_index_read_rows(full._h, first, count, po, 0))
        assert kind == "Unsupported" and "resident" in msg
    with pytest.raises(ia.CoreError) as err:
        full.read_rows()
    assert err.value.kind == "Unsupported"
    assert (out == 7.0).all() and full.to_bytes() == blob and full.row_storage()["block_bytes"] == 0
