"""isl_index_reserve / isl_index_capacity without a device: the symbols, every refusal that needs no device in its
order (an earlier check wins when two apply) with the stated words in the message, and the fresh handle."""
import ctypes as C
import os

import numpy as np
import pytest

import islands_amd as ia
from islands_amd import _ffi
from test_index_insert_cpu import error_of, ring

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, FP8 = ia.DTYPE_F32, ia.DTYPE_BF16, ia.DTYPE_FP8_E4M3


def raw(idx, capacity, d, dtype):
    lib = _ffi.lib()
    st = lib.isl_index_reserve(idx, capacity, d, dtype)
    return (lib.isl_status_name(st).decode(), lib.isl_last_error_message().decode(),
            (lib.isl_last_error_expected(), lib.isl_last_error_actual()))


def capacity_of(h):
    rows, allocs = C.c_uint64(77), C.c_uint64(77)
    assert _ffi.lib().isl_status_name(_ffi.lib().isl_index_capacity(h, C.byref(rows), C.byref(allocs))) == b"Ok"
    return rows.value, allocs.value


def test_symbols_are_exported_and_declared():
    assert {"isl_index_reserve", "isl_index_capacity"} <= set(_ffi.SIGNATURES)
    lib = _ffi.lib()
    assert lib.isl_index_reserve.restype is C.c_int32 and len(lib.isl_index_reserve.argtypes) == 4
    assert lib.isl_index_capacity.restype is C.c_int32 and len(lib.isl_index_capacity.argtypes) == 3
    header = open(os.path.join(ROOT, "include", "islands_amd.h")).read()
    assert "isl_status isl_index_reserve(isl_index* idx, uint64_t capacity, uint64_t d, int32_t dtype);" in header
    assert ("isl_status isl_index_capacity(const isl_index* idx, uint64_t* capacity_rows, uint64_t* row_allocations);"
            in header)
    assert "ONE COPY A RESERVATION COSTS" in header and "ROWS ARE THEN UNDEFINED" in header
    mirror = open(os.path.join(ROOT, "include", "islands_amd.hpp")).read()
    assert "void reserve(uint64_t capacity, uint64_t d" in mirror and "Capacity capacity() const" in mirror


def test_fresh_handle_has_no_capacity_and_no_allocation():
    idx = ia.LeannIndex(ia.LeannConfig(m=8, m0=16, ef_construction=40))
    assert capacity_of(idx._h) == (0, 0)
    assert idx.capacity == {"rows": 0, "row_allocations": 0}
    assert ring().capacity == {"rows": 0, "row_allocations": 0}  # lists, no rows
    lib = _ffi.lib()
    assert lib.isl_status_name(lib.isl_index_capacity(None, None, None)) == b"InvalidArgument"
    assert lib.isl_status_name(lib.isl_index_capacity(idx._h, None, None)) == b"Ok"  # either pointer may be NULL


def test_refusals_in_their_order():
    empty = ia.LeannIndex(ia.LeannConfig(m=8, m0=16, ef_construction=40))
    full = ring()
    blobs = empty.to_bytes(), full.to_bytes()
    hnsw = ia.HnswGraph.build(np.zeros((0, 0), np.float32), m=4, m0=8, ef_construction=16)
    core = C.c_void_p.from_address(hnsw._h.value)  # isl_hnsw's first member: the layer-0 isl_index
    big = 2 ** 31
    # 1. NULL idx -- before the dtype
    assert raw(None, 512, 16, 9)[0] == "InvalidArgument"
    # 2. an unknown dtype -- before the handle is looked at
    for h in (core, full._h, empty._h):
        kind, msg, _ = raw(h, big, 0, 9)
        assert kind == "InvalidArgument" and "dtype" in msg
    assert raw(empty._h, 512, 16, -1)[0] == "InvalidArgument"
    # 3. the core index of an HnswGraph -- before d == 0 and the capacity
    for dtype in (F32, BF16, FP8):
        kind, msg, _ = raw(core, big, 0, dtype)
        assert kind == "Unsupported" and "HnswGraph" in msg
    # (4. a recompute provider needs a device: tests/test_gpu_index_reserve.py)
    # 5. a non-empty index without resident rows -- before the capacity and before d is compared
    for cap, d in ((512, 16), (big, 16), (512, 12), (0, 0)):
        kind, msg, _ = raw(full._h, cap, d, F32)
        assert kind == "Unsupported" and "resident" in msg
    e = error_of(full.reserve, 512)
    assert e.kind == "Unsupported" and "resident" in str(e)
    # 6. d == 0 on an empty handle -- before the capacity
    assert raw(empty._h, big, 0, F32)[0] == "EmptyCollection"
    assert error_of(empty.reserve, 512).kind == "EmptyCollection"  # d is not optional for an empty handle
    assert error_of(empty.reserve, 512, 0, "bf16").kind == "EmptyCollection"
    # 7. a capacity above the device id range -- before the device is looked for
    for cap in (0x7FFFFFF0, big, 2 ** 63):
        kind, msg, _ = raw(empty._h, cap, 16, F32)
        assert kind == "Unsupported" and "capacity" in msg
    assert error_of(empty.reserve, big, 16).kind == "Unsupported"
    # ... an empty handle reserves f32 or bf16 rows, the types isl_index_insert takes
    kind, msg, _ = raw(empty._h, 512, 16, FP8)
    assert kind == "Unsupported" and "fp8" in msg
    with pytest.raises(ValueError):
        empty.reserve(512, 16, "f16")
    # nothing changed, nothing was allocated
    assert (empty.to_bytes(), full.to_bytes()) == blobs
    assert empty.capacity == full.capacity == {"rows": 0, "row_allocations": 0}


def test_without_a_device_the_handle_is_unchanged():
    if ia.device_count():
        pytest.skip("a device is visible: the reservation succeeds (tests/test_gpu_index_reserve.py)")
    empty = ia.LeannIndex(ia.LeannConfig(m=8, m0=16, ef_construction=40))
    blob = empty.to_bytes()
    assert error_of(empty.reserve, 512, 16).kind == "Device"
    assert empty.to_bytes() == blob and empty.capacity == {"rows": 0, "row_allocations": 0} and len(empty) == 0
