"""Refined search without a GPU: the new ABI symbols and their declarations, every refusal that is answered before
a device call in the order include/islands_amd.h states, and the host arithmetic of
islands_amd/csrc/search_refine_plan.hpp through tests/cpp/search_refine_plan_dump.cpp (g++ alone, and once more as a
stand-alone program under -fsanitize=address,undefined) against a Python restatement of the grid, the LDS, the
scratch and the order of the argument checks."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import islands_amd as ia
from islands_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "search_refine_plan_dump.cpp")
DECLARED = {
    "isl_index_set_refine_rows": "isl_index* idx, const void* rows, uint64_t n, uint64_t d, int32_t dtype, int32_t mem, "
                                 "int32_t placement",
    "isl_index_refine_storage": "const isl_index* idx, int32_t* dtype, int32_t* placement, uint64_t* rows, "
                                "uint64_t* block_bytes",
    "isl_rescore_device": "const isl_index* idx, const float* d_queries, uint64_t nq, uint64_t d, "
                          "const uint64_t* d_cand_ids, const uint32_t* d_cand_count, uint64_t pitch, uint64_t k, "
                          "uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count, void* stream",
    "isl_rescore": "const isl_index* idx, const float* queries, uint64_t nq, uint64_t d, const uint64_t* cand_ids, "
                   "const uint32_t* cand_count, uint64_t pitch, uint64_t k, uint64_t* out_ids, float* out_dist, "
                   "uint32_t* out_count",
    "isl_search_refined_batch_device": "const isl_index* idx, const float* d_queries, uint64_t nq, uint64_t d, uint64_t k, "
                                       "uint64_t candidates, uint64_t ef, uint64_t* d_out_ids, float* d_out_dist, "
                                       "uint32_t* d_out_count, void* stream",
    "isl_search_refined_batch": "const isl_index* idx, const float* queries, uint64_t nq, uint64_t d, uint64_t k, "
                                "uint64_t candidates, uint64_t ef, uint64_t* out_ids, float* out_dist, uint32_t* out_count",
}
OK, EMPTY, DIM, INVALID, UNSUPPORTED = 0, 2, 1, 101, 102  # isl_status
F32, BF16, FP8 = 0, 1, 2
# isl_refine::Why
(PASS, NULL, ENUM, WHY_FP8, HNSW, NO_DEVICE, ROW_COUNT, NO_DIM, DIM_MISMATCH, DIM_LIMIT, NO_TABLE, ZERO_K, K_ABOVE,
 CAND_ABOVE_EF, CAND_LIMIT, RECOMPUTE, QUERY_LIMIT) = range(17)


# ------------------------------------------------------------------ the ABI
def test_symbols_and_declarations():
    lib = _ffi.lib()
    hdr = open(os.path.join(ROOT, "include", "islands_amd.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    for name, args in DECLARED.items():
        assert hasattr(lib, name), name
        assert f"isl_status {name}({args});" in flat, name
        res, argtypes = _ffi.SIGNATURES[name]
        assert res is _ffi.i32 and len(argtypes) == args.count(",") + 1, name
    assert lib.isl_abi_version() == 3
    assert "enum { ISL_REFINE_DEVICE = 0, ISL_REFINE_HOST = 1 };" in flat
    assert re.search(r"#define ISL_REFINE_MAX_CANDIDATES 512u\b", hdr)
    assert (ia.REFINE_DEVICE, ia.REFINE_HOST, ia.REFINE_MAX_CANDIDATES) == (0, 1, 512)
    for name in ("set_refine_rows", "refine_storage", "search_refined_batch", "search_refined_batch_ptr", "rescore",
                 "rescore_ptr"):
        assert callable(getattr(ia.LeannIndex, name)), name
    hpp = open(os.path.join(ROOT, "include", "islands_amd.hpp")).read()
    for name in ("set_refine_rows", "refine_storage", "search_refined_batch", "rescore"):
        assert re.search(rf"\b{name}\(", hpp), name
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in DECLARED:
        assert name in integration, name
    for s in (1, 2, 101, 102):  # the statuses this file names
        assert lib.isl_status_name(s)
    names = {s: lib.isl_status_name(s).decode() for s in (DIM, EMPTY, INVALID, UNSUPPORTED)}
    assert names == {DIM: "DimensionMismatch", EMPTY: "EmptyCollection", INVALID: "InvalidArgument",
                     UNSUPPORTED: "Unsupported"}


def host_ring(n=5, d=4):
    g = ia.CsrGraph()
    for i in range(n):
        g.add_node([(i + 1) % n], 0)
    g.entry_point = 0
    return ia.LeannIndex.from_csr(g, dimension=d)


def test_set_refine_rows_refusals_before_a_device_call():
    lib = _ffi.lib()
    host = host_ring()
    before = host.to_bytes()
    rows = np.zeros((5, 4), np.float32)
    p = rows.ctypes.data
    call = lib.isl_index_set_refine_rows
    # NULL idx / NULL rows with n > 0 come first, whatever else is wrong
    assert call(None, p, 5, 4, 9, 9, 9) == INVALID
    assert call(host._h, None, 5, 4, 9, 9, 9) == INVALID
    assert b"NULL" in lib.isl_last_error_message()
    # then the three enumerations, before fp8 and before the residency
    assert call(host._h, p, 5, 4, 3, 0, 0) == INVALID
    assert call(host._h, p, 5, 4, -1, 0, 0) == INVALID
    assert call(host._h, p, 5, 4, FP8, 2, 0) == INVALID
    assert call(host._h, p, 5, 4, FP8, 0, 2) == INVALID
    assert b"unknown" in lib.isl_last_error_message()
    # fp8 before "not on a device"
    assert call(host._h, p, 5, 4, FP8, 0, 0) == UNSUPPORTED
    assert b"fp8" in lib.isl_last_error_message()
    # an index that is not on a device: before the row count, d == 0 and the dimension
    for n, d in ((5, 4), (4, 4), (5, 0), (5, 9), (0, 0)):
        assert call(host._h, p, n, d, F32, 0, 1) == UNSUPPORTED, (n, d)
        assert b"isl_index_upload" in lib.isl_last_error_message()
    with pytest.raises(ia.CoreError) as e:
        host.set_refine_rows(rows, placement="host")
    assert e.value.kind == "Unsupported"
    with pytest.raises(ValueError):
        host.set_refine_rows(rows, placement="managed")
    assert host.to_bytes() == before
    assert host.refine_storage() == {"dtype": 0, "placement": "device", "rows": 0, "block_bytes": 0}
    assert lib.isl_index_refine_storage(None, None, None, None, None) == INVALID
    assert lib.isl_index_refine_storage(host._h, None, None, None, None) == OK


def test_refined_search_refusals_before_a_device_call():
    lib = _ffi.lib()
    host = host_ring()
    q = np.zeros((2, 4), np.float32)
    ids, dist, cnt = np.zeros((2, 4), np.uint64), np.zeros((2, 4), np.float32), np.zeros(2, np.uint32)
    cand, cc = np.zeros((2, 8), np.uint64), np.full(2, 8, np.uint32)
    a = lambda x: x.ctypes.data
    # NULL idx, NULL buffers with nq > 0
    assert lib.isl_search_refined_batch(None, a(q), 2, 4, 2, 4, 8, a(ids), a(dist), a(cnt)) == INVALID
    assert lib.isl_search_refined_batch(host._h, None, 2, 4, 2, 4, 8, a(ids), a(dist), a(cnt)) == INVALID
    assert lib.isl_search_refined_batch(host._h, a(q), 2, 4, 2, 4, 8, a(ids), None, a(cnt)) == INVALID
    assert lib.isl_search_refined_batch_device(host._h, a(q), 2, 4, 2, 4, 8, a(ids), a(dist), None, None) == INVALID
    assert lib.isl_rescore_device(host._h, a(q), 2, 4, None, a(cc), 8, 2, a(ids), a(dist), a(cnt), None) == INVALID
    assert lib.isl_rescore(host._h, a(q), 2, 4, a(cand), None, 8, 2, a(ids), a(dist), a(cnt)) == INVALID
    assert b"NULL" in lib.isl_last_error_message()
    # no refine table: before k, candidates, ef, the cap and the dimension, and it says how to set one
    for k, c, ef, d in ((2, 4, 8, 4), (0, 4, 8, 4), (5, 4, 8, 4), (2, 9, 8, 4), (2, 600, 600, 4), (2, 4, 8, 7)):
        assert lib.isl_search_refined_batch(host._h, a(q), 2, d, k, c, ef, a(ids), a(dist), a(cnt)) == INVALID, (k, c, ef)
        assert b"isl_index_set_refine_rows" in lib.isl_last_error_message()
        assert lib.isl_search_refined_batch_device(host._h, a(q), 2, d, k, c, ef, a(ids), a(dist), a(cnt), None) == INVALID
        assert lib.isl_rescore(host._h, a(q), 2, d, a(cand), a(cc), c, k, a(ids), a(dist), a(cnt)) == INVALID
        assert lib.isl_rescore_device(host._h, a(q), 2, d, a(cand), a(cc), c, k, a(ids), a(dist), a(cnt), None) == INVALID
        assert b"isl_index_set_refine_rows" in lib.isl_last_error_message()
    with pytest.raises(ia.CoreError) as e:
        host.search_refined_batch(q, 2, 8)
    assert e.value.kind == "InvalidArgument" and "set_refine_rows" in str(e.value)
    with pytest.raises(ia.CoreError) as e:
        host.rescore(q, cand, cc, 2)
    assert e.value.kind == "InvalidArgument"


# ------------------------------------------------------------------ the plan header
def build(flags, name):
    exe = os.path.join(ROOT, "islands_amd", "lib", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", *flags, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def exes():
    return (build(["-O1"], "search_refine_plan_dump"),
            build(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                  "search_refine_plan_dump_san"))


def dump(exe, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1")
    text = "".join(" ".join(str(int(v)) if not isinstance(v, str) else v for v in ln) + "\n" for ln in lines)
    pr = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60, env=env)
    assert pr.returncode == 0 and "Sanitizer" not in pr.stderr and "runtime error" not in pr.stderr, pr.stderr[-2000:]
    out = [ln.split() for ln in pr.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def restated_geo(d, pitch, nq, c):
    padded = -(-d // 32) * 32
    lds = padded * 4 + pitch * 12          # the query, then an 8-byte key and a 4-byte score per slot
    passes = -(-c // 64)
    return [padded, lds, nq, passes, passes * c, nq * pitch, nq * pitch, nq, nq * pitch * 12 + nq * 4]


def restated_set(null_idx, is_hnsw, on_device, has_dim, length, dimension, rows_null, n, d, dtype, mem, placement):
    if null_idx or (rows_null and n > 0):
        return [INVALID, NULL, 0]
    if dtype not in (F32, BF16, FP8) or mem not in (0, 1) or placement not in (0, 1):
        return [INVALID, ENUM, 0]
    if dtype == FP8:
        return [UNSUPPORTED, WHY_FP8, 0]
    if is_hnsw:
        return [UNSUPPORTED, HNSW, 0]
    if not on_device:
        return [UNSUPPORTED, NO_DEVICE, 0]
    if n == 0:
        return [OK, PASS, 1]
    if n != length:
        return [INVALID, ROW_COUNT, 0]
    if d == 0:
        return [EMPTY, NO_DIM, 0]
    if has_dim and d != dimension:
        return [DIM, DIM_MISMATCH, 0]
    if d > 32768:
        return [UNSUPPORTED, DIM_LIMIT, 0]
    return [OK, PASS, 0]


def restated_ref(null_idx, is_hnsw, recompute, table_rows, table_d, buffers_null, nq, d, k, candidates, ef):
    if null_idx or (buffers_null and nq > 0):
        return [INVALID, NULL]
    if table_rows == 0:
        return [INVALID, NO_TABLE]
    if k == 0:
        return [INVALID, ZERO_K]
    if k > candidates:
        return [INVALID, K_ABOVE]
    if candidates > ef:
        return [INVALID, CAND_ABOVE_EF]
    if candidates > 512:
        return [UNSUPPORTED, CAND_LIMIT]
    if d != table_d:
        return [DIM, DIM_MISMATCH]
    if recompute:
        return [UNSUPPORTED, RECOMPUTE]
    if is_hnsw:
        return [UNSUPPORTED, HNSW]
    if nq > 0x7FFFFFFF:
        return [INVALID, QUERY_LIMIT]
    return [OK, PASS]


def test_geometry_against_its_restatement(exes):
    cases = [(d, pitch, nq, c) for d in (1, 24, 31, 32, 33, 50, 768, 832, 32768) for pitch in (1, 64, 65, 512)
             for nq, c in ((1, 1), (70, min(pitch, 63)), (4096, pitch))]
    out = [dump(exe, [["geo", *c] for c in cases]) for exe in exes]
    assert out[0] == out[1]
    for c, ln in zip(cases, out[0]):
        assert ln == ["geo"] + [str(v) for v in restated_geo(*c)], (c, ln)
    # the largest workgroup the checks let through fits the 160 KiB of a CU's LDS
    assert restated_geo(32768, 512, 1, 512)[1] == 128 * 1024 + 6 * 1024 <= 160 * 1024


def test_set_rows_checks_in_the_stated_order(exes):
    cases = []
    for null_idx, is_hnsw, on_device, rows_null in itertools.product((0, 1), repeat=4):
        for n, d in ((0, 0), (5, 4), (4, 4), (5, 0), (5, 9), (5, 32769)):
            for dtype, mem, placement in ((F32, 0, 0), (BF16, 1, 1), (FP8, 0, 1), (3, 0, 0), (F32, 2, 0), (F32, 0, 2),
                                          (-1, 0, 0)):
                for has_dim in ((0, 1) if d in (9, 32769) else (1,)):
                    cases.append((null_idx, is_hnsw, on_device, has_dim, 5, 4, rows_null, n, d, dtype, mem, placement))
    out = [dump(exe, [["set", *c] for c in cases]) for exe in exes]
    assert out[0] == out[1]
    seen = set()
    for c, ln in zip(cases, out[0]):
        want = restated_set(*c)
        assert ln == ["set"] + [str(v) for v in want], (c, ln)
        seen.add(want[1])
    assert seen == {PASS, NULL, ENUM, WHY_FP8, HNSW, NO_DEVICE, ROW_COUNT, NO_DIM, DIM_MISMATCH, DIM_LIMIT}


def test_refined_checks_in_the_stated_order(exes):
    cases = []
    for null_idx, is_hnsw, recompute, buffers_null in itertools.product((0, 1), repeat=4):
        for table_rows in (0, 5):
            for nq in (0, 3, 1 << 31):
                for d in (4, 7):
                    for k, cand, ef in ((2, 4, 8), (0, 4, 8), (5, 4, 8), (2, 9, 8), (2, 513, 600), (512, 512, 512),
                                        (1, 1, 1), (600, 513, 512)):
                        cases.append((null_idx, is_hnsw, recompute, table_rows, 4, buffers_null, nq, d, k, cand, ef))
    out = [dump(exe, [["ref", *c] for c in cases]) for exe in exes]
    assert out[0] == out[1]
    seen = set()
    for c, ln in zip(cases, out[0]):
        want = restated_ref(*c)
        assert ln == ["ref"] + [str(v) for v in want], (c, ln)
        seen.add(want[1])
    assert seen == {PASS, NULL, NO_TABLE, ZERO_K, K_ABOVE, CAND_ABOVE_EF, CAND_LIMIT, DIM_MISMATCH, RECOMPUTE, HNSW,
                    QUERY_LIMIT}
