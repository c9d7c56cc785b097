"""isl_index_build_rows (LeannIndex::build from f32 or bf16 rows) without a device: the symbol and its
declarations, every check that comes before a device call, the empty index, and the LDS arithmetic of the
builder kernels' bf16 instantiations (build_plan.hpp) against a restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import islands_amd as ia
from islands_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = 0, 1


def to_bf16_bits(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def widen(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def call(rows, dtype, n, d, cfg=None, opts="default", out=True):
    """(status, handle value) of one raw call; the handle starts as a sentinel so that a write shows"""
    c = (cfg or ia.LeannConfig())._to_c()
    o = None
    if opts is not None:
        o = _ffi.BuildOptionsC()
        _ffi.lib().isl_build_options_default(C.byref(o))
        if opts != "default":
            for k, v in opts.items():
                setattr(o, k, v)
    h = C.c_void_p(0xDEAD)
    rp = None if rows is None else rows.ctypes.data_as(C.c_void_p)
    st = _ffi.lib().isl_index_build_rows(C.byref(c), None if o is None else C.byref(o), rp, dtype, n, d, None, 0, 0,
                                         C.byref(h) if out else None)
    return st, h.value


def kind(st):
    with pytest.raises(ia.CoreError) as e:
        ia._check(st)
    return e.value.kind


def test_symbol_is_exported_and_declared():
    assert "isl_index_build_rows" in _ffi.SIGNATURES
    fn = _ffi.lib().isl_index_build_rows
    assert fn.restype is C.c_int32 and len(fn.argtypes) == 10
    header = open(os.path.join(ROOT, "include", "islands_amd.h")).read()
    assert ("isl_status isl_index_build_rows(const isl_leann_config* cfg, const isl_build_options* opts, "
            "const void* rows,") in header
    assert "build_bf16" in open(os.path.join(ROOT, "include", "islands_amd.hpp")).read()
    assert _ffi.lib().isl_abi_version() == 3  # an addition


def test_checks_before_any_device_call():
    bits = to_bf16_bits(np.ones((4, 8), np.float32))
    for dtype in (F32, BF16):
        rows = widen(bits) if dtype == F32 else bits
        st, h = call(rows, dtype, 4, 8, out=False)
        assert kind(st) == "InvalidArgument"
        st, h = call(None, dtype, 4, 8)
        assert kind(st) == "InvalidArgument" and h == 0xDEAD
        st, h = call(rows, dtype, 4, 8, opts={"struct_size": 8})
        assert kind(st) == "InvalidArgument" and h == 0xDEAD
        st, h = call(rows, dtype, 4, 8, opts={"select_rule": 7})
        assert kind(st) == "InvalidArgument" and h == 0xDEAD
        st, h = call(rows, dtype, 4, 8, opts={"select_rule": 1, "alpha": 0.5})
        assert kind(st) == "InvalidConfig" and h == 0xDEAD
        st, h = call(rows, dtype, 4, 0)
        assert kind(st) == "EmptyCollection" and h == 0xDEAD
        st, h = call(rows, dtype, 4, 8, cfg=ia.LeannConfig(m=64, m0=129, ef_construction=200))
        assert kind(st) == "Unsupported" and h == 0xDEAD
        st, h = call(rows, dtype, 4, 8, cfg=ia.LeannConfig(m=0))
        assert kind(st) == "InvalidConfig" and h == 0xDEAD
    for dtype in (2, -1, 7):
        st, h = call(bits, dtype, 4, 8)
        assert kind(st) == "InvalidArgument" and h == 0xDEAD
    # the order: options, then the dtype, then the config, then the data
    st, h = call(bits, 9, 4, 8, opts={"select_rule": 1, "alpha": 0.5})
    assert kind(st) == "InvalidConfig"
    st, h = call(bits, 9, 4, 0, cfg=ia.LeannConfig(m=0))
    assert kind(st) == "InvalidArgument"
    st, h = call(bits, BF16, 0, 0, cfg=ia.LeannConfig(m=0))
    assert kind(st) == "InvalidConfig"
    st, h = call(bits, BF16, 4, 0, cfg=ia.LeannConfig(m=64, m0=129, ef_construction=200))
    assert kind(st) == "EmptyCollection"


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_no_rows_is_an_empty_index(dtype):
    c = ia.LeannConfig(m=8, m0=16, ef_construction=40)._to_c()
    h = C.c_void_p()
    assert _ffi.lib().isl_index_build_rows(C.byref(c), None, None, dtype, 0, 0, None, 0, 0, C.byref(h)) == 0
    idx = ia.LeannIndex(_handle=h)
    assert idx.is_empty() and len(idx) == 0 and idx.entry_point is None
    assert ia.LeannIndex.from_bytes(idx.to_bytes()).to_bytes() == idx.to_bytes()
    assert idx.to_bytes() == ia.LeannIndex.build(np.zeros((0, 0), np.float32),
                                                 ia.LeannConfig(m=8, m0=16, ef_construction=40)).to_bytes()


def test_python_mirror():
    e = ia.LeannIndex.build_bf16(np.zeros((0, 0), np.uint16))
    assert e.is_empty()
    with pytest.raises(ia.CoreError) as ex:
        ia.LeannIndex.build_bf16(np.ones((4, 8), np.uint16), ia.LeannConfig(m=64, m0=129, ef_construction=200))
    assert ex.value.kind == "Unsupported"
    with pytest.raises(ia.CoreError) as ex:
        ia.LeannIndex.build_bf16(np.ones((4, 8), np.uint16), select="diverse", alpha=0.5)
    assert ex.value.kind == "InvalidConfig"
    with pytest.raises(ValueError):
        ia.LeannIndex.build_bf16(np.ones((4, 8), np.uint16), select="nearest")


def test_build_without_a_device_is_a_device_error():
    """No CPU fallback: with no gfx950 a real build reports Device and writes no handle.  (Beside a device
    the same call builds; the GPU tests say what.)"""
    bits = to_bf16_bits(np.arange(32, dtype=np.float32).reshape(4, 8))
    if ia.device_count() == 0:
        for dtype, rows in ((BF16, bits), (F32, widen(bits))):
            st, h = call(rows, dtype, 4, 8)
            assert kind(st) == "Device" and h == 0xDEAD
    else:
        assert len(ia.LeannIndex.build_bf16(bits)) == 4


# ---------------------------------------------------------------- LDS of the bf16 instantiations
def want_lds(d, nmax, M):
    """The query as f32 in whole steps of 32 elements (the tile-free distance routine fetches the operand of
    every step whole) plus 16 floats of slack, no tile; a selection adds four lists of nmax and a row of M."""
    qf = -(-d // 32) * 32 + 16
    return qf, qf * 4, qf * 4 + nmax * 16 + M * 4


def test_bf16_lds_formula():
    exe = os.path.join(ROOT, "islands_amd", "lib", "build_lds_dump")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "build_lds_dump.cpp"),
                           "-o", exe])
    cases = [(d, nmax, M) for d in (3, 100, 768, 4096) for nmax in (40, 129, 512) for M in (16, 128)]
    text = "".join(f"{d} {nmax} {M}\n" for d, nmax, M in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60, check=True).stdout
    got = [tuple(int(x) for x in ln.split()) for ln in out.splitlines()]
    assert len(got) == len(cases)
    for (d, nmax, M), row in zip(cases, got):
        assert row == (d, nmax, M) + want_lds(d, nmax, M), (d, nmax, M)
        qf = row[3]
        assert qf % 4 == 0 and qf >= (d + 31) // 32 * 32  # the lists behind the query start 16-byte aligned
        assert row[5] <= 64 * 1024                        # one wave's share fits the default LDS limit
