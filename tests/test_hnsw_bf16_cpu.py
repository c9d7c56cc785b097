"""An HnswGraph over bf16 rows, what needs no device: the four new symbols are exported and declared in every
mirror, every pre-device check of isl_hnsw_build_rows / isl_hnsw_insert_rows answers in the documented order
without writing its out pointer, and the empty graph is the f32 empty graph.  (build_plan.hpp gained no LDS
formula: the builder's descent over bf16 rows is launched with link_lds_bf16, which
tests/test_build_bf16_cpu.py restates already.)"""
import ctypes as C
import os

import numpy as np
import pytest

import islands_amd as ia
from islands_amd import _ffi
from test_hnsw_bytes import hnsw_to_bincode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["isl_hnsw_build_rows", "isl_hnsw_insert_rows", "isl_hnsw_from_layers_rows", "isl_hnsw_row_storage"]
F32, BF16, FP8 = 0, 1, 2
SENTINEL = 0x5A5A5A5A


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def name(st):
    return _ffi.lib().isl_status_name(st).decode()


# ---------------------------------------------------------------- 1. the symbols
def test_symbols_are_exported_and_declared():
    lib = _ffi.lib()  # binds every entry of SIGNATURES: a missing export raises here
    header, mirror = read("include", "islands_amd.h"), read("include", "islands_amd.hpp")
    for sym in NEW:
        assert sym in _ffi.SIGNATURES, sym
        assert getattr(lib, sym) is not None
        assert f"isl_status {sym}(" in header, sym
    for sym in ("isl_hnsw_build_rows", "isl_hnsw_insert_rows", "isl_hnsw_row_storage"):
        assert sym + "(" in mirror, sym
    for method in ("build_bf16", "insert_bf16", "row_storage"):
        assert method + "(" in mirror and hasattr(ia.HnswGraph, method), method
    assert hasattr(ia.HnswGraph, "from_layers_bf16")
    assert lib.isl_abi_version() == 3 and "#define ISL_ABI_VERSION 3" in header
    # the header says what to_bytes writes for bf16 rows
    assert "widened" in header


# ---------------------------------------------------------------- 2. the checks before any device call
def config(**kw):
    c = _ffi.HnswConfigC()
    _ffi.lib().isl_hnsw_config_default(C.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def options(**kw):
    o = _ffi.BuildOptionsC()
    _ffi.lib().isl_build_options_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


ROWS = np.full((8, 4), 0x3F80, np.uint16)  # eight rows of ones


def build_rows(cfg=None, opts=None, rows=ROWS, dtype=BF16, n=8, d=4, levels=None, out=True):
    """(status name, the handle afterwards) of one isl_hnsw_build_rows call whose handle starts as a sentinel"""
    h = C.c_void_p(SENTINEL)
    lv = None if levels is None else np.ascontiguousarray(levels, dtype=np.uint64)
    st = _ffi.lib().isl_hnsw_build_rows(
        None if cfg is None else C.byref(cfg), None if opts is None else C.byref(opts),
        None if rows is None else rows.ctypes.data_as(C.c_void_p), dtype, n, d,
        None if lv is None else lv.ctypes.data_as(C.c_void_p), 0, ia.MEM_HOST, 0, C.byref(h) if out else None)
    return name(st), h.value


def test_build_rows_checks_in_the_documented_order():
    # each check on its own
    assert build_rows(out=False)[0] == "InvalidArgument"
    assert build_rows(rows=None) == ("InvalidArgument", SENTINEL)
    assert build_rows(opts=options(select_rule=7)) == ("InvalidArgument", SENTINEL)
    assert build_rows(opts=options(struct_size=4)) == ("InvalidArgument", SENTINEL)
    assert build_rows(opts=options(select_rule=1, alpha=0.5)) == ("InvalidConfig", SENTINEL)
    assert build_rows(dtype=7) == ("InvalidArgument", SENTINEL)
    assert build_rows(dtype=-1) == ("InvalidArgument", SENTINEL)
    assert build_rows(dtype=FP8) == ("Unsupported", SENTINEL)
    assert build_rows(cfg=config(m=0)) == ("InvalidConfig", SENTINEL)
    assert build_rows(cfg=config(m=16, m0=8)) == ("InvalidConfig", SENTINEL)
    assert build_rows(d=0) == ("EmptyCollection", SENTINEL)
    assert build_rows(levels=[0, 1, 16, 0, 0, 0, 0, 0]) == ("InvalidArgument", SENTINEL)
    assert build_rows(cfg=config(max_layers=3), levels=[0, 1, 3, 0, 0, 0, 0, 0]) == ("InvalidArgument", SENTINEL)
    assert build_rows(cfg=config(m0=129)) == ("Unsupported", SENTINEL)
    assert build_rows(cfg=config(ef_construction=513)) == ("Unsupported", SENTINEL)
    # the order: NULL, options, dtype, config, (n == 0), d == 0, levels, shape
    assert build_rows(rows=None, opts=options(alpha=0.5, select_rule=1)) == ("InvalidArgument", SENTINEL)
    assert build_rows(opts=options(select_rule=1, alpha=0.5), dtype=FP8) == ("InvalidConfig", SENTINEL)
    assert build_rows(dtype=FP8, cfg=config(m=0)) == ("Unsupported", SENTINEL)
    assert build_rows(dtype=7, cfg=config(m=0)) == ("InvalidArgument", SENTINEL)
    assert build_rows(cfg=config(m=0), d=0) == ("InvalidConfig", SENTINEL)
    assert build_rows(d=0, levels=[99] * 8) == ("EmptyCollection", SENTINEL)
    assert build_rows(cfg=config(m0=129), levels=[99] * 8) == ("InvalidArgument", SENTINEL)
    # the dtype is checked in front of n == 0, and a bad config too
    assert build_rows(dtype=FP8, n=0, rows=None) == ("Unsupported", SENTINEL)
    assert build_rows(cfg=config(m=0), n=0, rows=None) == ("InvalidConfig", SENTINEL)
    # F32 is isl_hnsw_build: the same answers
    f32 = np.ones((8, 4), np.float32)
    assert build_rows(rows=f32, dtype=F32, d=0) == ("EmptyCollection", SENTINEL)
    assert build_rows(rows=f32, dtype=F32, levels=[16] * 8) == ("InvalidArgument", SENTINEL)


def insert_rows(g, opts=None, rows=ROWS, dtype=BF16, n=8, d=4, levels=None, handle=True):
    first = C.c_uint64(SENTINEL)
    lv = None if levels is None else np.ascontiguousarray(levels, dtype=np.uint64)
    st = _ffi.lib().isl_hnsw_insert_rows(
        g._h if handle else None, None if opts is None else C.byref(opts),
        None if rows is None else rows.ctypes.data_as(C.c_void_p), dtype, n, d,
        None if lv is None else lv.ctypes.data_as(C.c_void_p), 0, ia.MEM_HOST, C.byref(first))
    return name(st), first.value


def test_insert_rows_checks_in_the_documented_order():
    g = ia.HnswGraph.build_bf16(np.zeros((0, 0), np.uint16), m=8, m0=16, ef_construction=64, max_layers=4)
    blob = g.to_bytes()
    assert insert_rows(g, handle=False) == ("InvalidArgument", SENTINEL)
    assert insert_rows(g, rows=None) == ("InvalidArgument", SENTINEL)
    assert insert_rows(g, opts=options(select_rule=7)) == ("InvalidArgument", SENTINEL)
    assert insert_rows(g, opts=options(select_rule=1, alpha=float("nan"))) == ("InvalidConfig", SENTINEL)
    assert insert_rows(g, dtype=9) == ("InvalidArgument", SENTINEL)
    assert insert_rows(g, dtype=FP8) == ("Unsupported", SENTINEL)
    assert insert_rows(g, d=0) == ("EmptyCollection", SENTINEL)
    assert insert_rows(g, levels=[0, 0, 4, 0, 0, 0, 0, 0]) == ("InvalidArgument", SENTINEL)  # max_layers = 4
    # the order: NULL, options, dtype, n_new == 0, d == 0, levels
    assert insert_rows(g, rows=None, opts=options(select_rule=7), dtype=FP8) == ("InvalidArgument", SENTINEL)
    assert insert_rows(g, opts=options(select_rule=1, alpha=0.5), dtype=FP8) == ("InvalidConfig", SENTINEL)
    assert insert_rows(g, dtype=FP8, n=0, rows=None) == ("Unsupported", SENTINEL)
    assert insert_rows(g, dtype=9, d=0) == ("InvalidArgument", SENTINEL)
    assert insert_rows(g, d=0, levels=[4] * 8) == ("EmptyCollection", SENTINEL)
    # no rows: ISL_OK, *first_id = len, nothing changed
    assert insert_rows(g, n=0, rows=None, d=0) == ("Ok", 0)
    assert len(g) == 0 and g.to_bytes() == blob
    # the Python mirror: one level per row, and the kinds above as CoreError
    with pytest.raises(ValueError):
        g.insert_bf16(ROWS, levels=[0, 0])
    with pytest.raises(ia.CoreError) as e:
        g.insert_bf16(ROWS, levels=[4] * 8)
    assert e.value.kind == "InvalidArgument" and len(g) == 0 and g.to_bytes() == blob


def test_from_layers_rows_checks_its_dtype_first():
    lib = _ffi.lib()
    h = C.c_void_p(SENTINEL)
    args = (16, 32, 200, 0, 0, 0, 0, None, None, None, 0, 0, 0, None)
    assert name(lib.isl_hnsw_from_layers_rows(*args, FP8, 0, C.byref(h))) == "Unsupported" and h.value == SENTINEL
    assert name(lib.isl_hnsw_from_layers_rows(*args, 5, 0, C.byref(h))) == "InvalidArgument" and h.value == SENTINEL
    assert name(lib.isl_hnsw_from_layers_rows(*args, BF16, 0, None)) == "InvalidArgument"
    assert name(lib.isl_hnsw_from_layers_rows(0, 32, 200, 0, 0, 0, 0, None, None, None, 0, 0, 0, None, BF16, 0,
                                              C.byref(h))) == "InvalidConfig" and h.value == SENTINEL
    assert name(lib.isl_hnsw_row_storage(None, None, None)) == "InvalidArgument"


# ---------------------------------------------------------------- 3. the empty graph
def test_empty_bf16_build_is_the_f32_empty_graph():
    kw = dict(m=8, m0=16, ef_construction=64, metric=1, ml=1.0 / np.log(8))
    g = ia.HnswGraph.build_bf16(np.zeros((0, 0), np.uint16), **kw)
    assert len(g) == 0 and g.entry_point is None and g.max_level == 0 and g.levels().size == 0
    empty = hnsw_to_bincode(np.zeros((0, 0), np.float32), [[]], [], None, 0, m=8, m0=16, ef_construction=64,
                            metric=1, dimension=None)
    assert g.to_bytes() == empty == ia.HnswGraph.build(np.zeros((0, 0), np.float32), **kw).to_bytes()
    assert g.row_storage() == {"dtype": F32, "block_bytes": 0}
    assert g.neighbors(0, 0) is None and g.get_vector(0) is None
    # handed over without nodes: the same
    e = ia.HnswGraph.from_layers_bf16(np.zeros((0, 0), np.uint16), [], [], None, 0)
    assert len(e) == 0 and e.row_storage() == {"dtype": F32, "block_bytes": 0}
