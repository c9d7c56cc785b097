"""isl_index_insert without a device: every argument check in its order (an earlier check wins when two apply),
the call that changes nothing, the Device error that leaves the handle serialisable, the symbol, the planner
entered at a step boundary for all-zero levels (plan_steps_from of build_plan.hpp through
tests/cpp/insert_plan_dump.cpp, g++ alone), and the same checks under AddressSanitizer in a stand-alone program
(tests/cpp/index_insert_host.cpp over the library's own sources, host code instrumented)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import islands_amd as ia
from islands_amd import _ffi
from _data import uniform_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ring(n=12, dimension=16, **cfg):
    """a non-empty index that needs no device: a ring, not uploaded, no rows"""
    g = ia.CsrGraph(node_offsets=np.arange(n + 1, dtype=np.uint64), neighbors=(np.arange(n, dtype=np.uint64) + 1) % n,
                    levels=np.zeros(n, np.uint64), entry_point=0, num_nodes=n, degree_counts=np.ones(n, np.uint64))
    return ia.LeannIndex.from_csr(g, ia.LeannConfig(**cfg), dimension=dimension)


def error_of(call, *a, **kw):
    with pytest.raises(ia.CoreError) as e:
        call(*a, **kw)
    return e.value


def raw(idx, rows, dtype, n_new, d, opts=None, first=None):
    lib = _ffi.lib()
    st = lib.isl_index_insert(idx, opts, None if rows is None else rows.ctypes.data_as(C.c_void_p), dtype, n_new, d,
                              None, 0, first)
    return lib.isl_status_name(st).decode(), lib.isl_last_error_message().decode()


def test_checks_in_their_order():
    v = uniform_vectors(8, 16, 1)
    empty = ia.LeannIndex(ia.LeannConfig(m=8, m0=16, ef_construction=40))
    full = ring()
    blobs = empty.to_bytes(), full.to_bytes()
    first = C.c_uint64(77)
    # 1. NULL idx, NULL rows with n_new > 0 -- before the options and the dtype
    bad = _ffi.BuildOptionsC()
    _ffi.lib().isl_build_options_default(C.byref(bad))
    bad.select_rule = 7
    assert raw(None, v, 9, 8, 16, C.byref(bad), C.byref(first))[0] == "InvalidArgument"
    assert raw(full._h, None, 0, 8, 16)[0] == "InvalidArgument"
    kind, msg = raw(full._h, None, 9, 8, 16, C.byref(bad))
    assert kind == "InvalidArgument" and "NULL" in msg
    # 2. the options, as isl_index_build_ex checks them -- before the dtype and before n_new == 0
    assert error_of(ia.LeannIndex.build, v, select=7).kind == error_of(full.insert, v, select=7).kind == "InvalidArgument"
    assert (error_of(ia.LeannIndex.build, v, select="diverse", alpha=0.5).kind
            == error_of(full.insert, v, select="diverse", alpha=0.5).kind == "InvalidConfig")
    bad.select_rule, bad.alpha = 1, 0.5
    assert raw(full._h, v, 9, 0, 16, C.byref(bad))[0] == "InvalidConfig"
    # 3. an unknown dtype -- before n_new == 0
    kind, msg = raw(full._h, v, 9, 0, 16)
    assert kind == "InvalidArgument" and "dtype" in msg
    # 4. no rows: ISL_OK, nothing changed -- before the handle and the dimension are looked at
    hnsw = ia.HnswGraph.build(np.zeros((0, 0), np.float32), m=4, m0=8, ef_construction=16)
    core = C.c_void_p.from_address(hnsw._h.value)  # isl_hnsw's first member: the layer-0 isl_index
    assert raw(core, v, 0, 0, 5, None, C.byref(first))[0] == "Ok" and first.value == 0
    first.value = 77
    assert full.insert(np.zeros((0, 5), np.float32)) == 12 and empty.insert_bf16(np.zeros((0, 5), np.uint16)) == 0
    # 5. the core index of an HnswGraph -- before the dimension (here 0) is looked at
    kind, msg = raw(core, v, 0, 8, 0, None, C.byref(first))
    assert kind == "Unsupported" and "isl_hnsw_insert" in msg and first.value == 77
    # 6. a non-empty index and another dimension, with the payload -- before d == 0 and before the rows are missed
    e = error_of(full.insert, uniform_vectors(8, 12, 1))
    assert e.kind == "DimensionMismatch" and (e.expected, e.actual) == (16, 12)
    e = error_of(full.insert, np.zeros((4, 0), np.float32))
    assert e.kind == "DimensionMismatch" and (e.expected, e.actual) == (16, 0)
    # 7. d == 0 -- before the shape limits
    wide = ia.LeannIndex(ia.LeannConfig(m=64, m0=129, ef_construction=200))
    assert error_of(empty.insert, np.zeros((4, 0), np.float32)).kind == "EmptyCollection"
    assert error_of(wide.insert, np.zeros((4, 0), np.float32)).kind == "EmptyCollection"
    # 8. a non-empty index without resident rows -- before the stored type and the shape limits
    e = error_of(full.insert, v)
    assert e.kind == "Unsupported" and "resident" in str(e)
    e = error_of(full.insert_bf16, v.view(np.uint16)[:, :16])
    assert e.kind == "Unsupported" and "resident" in str(e)
    e = error_of(ring(m=64, m0=129, ef_construction=200).insert, v)
    assert e.kind == "Unsupported" and "resident" in str(e)
    # (9. the stored type needs resident rows: tests/test_gpu_index_insert.py)
    # 10. the shape limits -- before any device call
    e = error_of(wide.insert, v)
    assert e.kind == "Unsupported" and "m0 <= 128" in str(e)
    e = error_of(ia.LeannIndex(ia.LeannConfig(m=8, m0=16, ef_construction=513)).insert, v)
    assert e.kind == "Unsupported" and "ef_construction" in str(e)
    with pytest.raises(ValueError):
        full.insert(v, levels=[0, 0])
    assert (empty.to_bytes(), full.to_bytes()) == blobs and len(full) == 12 and len(empty) == 0


def test_no_rows_is_ok_and_changes_nothing():
    full = ring()
    blob = full.to_bytes()
    first = C.c_uint64(77)
    assert raw(full._h, None, 0, 0, 16, None, C.byref(first))[0] == "Ok" and first.value == 12
    assert raw(full._h, None, 1, 0, 3)[0] == "Ok"  # first_id may be NULL; neither d nor the type is looked at
    assert full.to_bytes() == blob and len(full) == 12 and full.entry_point == 0


def test_insert_without_a_device_leaves_the_handle():
    """No CPU fallback: with no gfx950 a non-empty insert reports Device and the handle is as it was and
    serialisable.  (Where this runs beside a device the same call succeeds; the GPU tests say what it built.)"""
    idx = ia.LeannIndex(ia.LeannConfig(m=8, m0=16, ef_construction=40))
    blob = idx.to_bytes()
    v = uniform_vectors(8, 4, 1)
    if ia.device_count() == 0:
        assert error_of(idx.insert, v).kind == "Device"
        assert len(idx) == 0 and idx.entry_point is None and idx.dimension() is None and idx.to_bytes() == blob
        assert ia.LeannIndex.from_bytes(blob).to_bytes() == blob
    else:
        assert idx.insert(v) == 0 and len(idx) == 8 and idx.entry_point == 0


def test_symbol_is_exported_and_declared():
    assert "isl_index_insert" in _ffi.SIGNATURES
    fn = _ffi.lib().isl_index_insert
    assert fn.restype is C.c_int32 and len(fn.argtypes) == 9
    header = open(os.path.join(ROOT, "include", "islands_amd.h")).read()
    assert "isl_status isl_index_insert(isl_index* idx, const isl_build_options* opts, const void* rows" in header
    assert _ffi.lib().isl_abi_version() == 3


@pytest.fixture(scope="module")
def plan_from():
    exe = os.path.join(ROOT, "islands_amd", "lib", "insert_plan_dump")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "insert_plan_dump.cpp"),
                           "-o", exe])

    def run(levels, n0, max_level0, batch):
        text = f"{batch} {n0} {max_level0} {len(levels)}\n" + " ".join(str(int(x)) for x in levels) + "\n"
        out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60, check=True).stdout
        lines = out.splitlines()
        steps = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("step")]
        order = [int(x) for x in next(ln for ln in lines if ln.startswith("order")).split()[1:]]
        return steps, order

    return run


@pytest.mark.parametrize("n", [2, 9, 333, 3000])
@pytest.mark.parametrize("batch", [1, 7, 256, 4096])
def test_plan_from_a_step_boundary_is_the_tail(plan_from, n, batch):
    """LeannIndex::build's plan: all-zero levels, never cut, `order` the identity.  From any boundary of the full
    plan the planner gives the tail of the full plan: the batched split build runs the steps of the one-call
    build when it is split at one."""
    lv = [0] * n
    full_steps, full_order = plan_from(lv, 1, 0, batch)
    assert full_order == list(range(n)) and all(top == 0 for _, _, top in full_steps)
    assert sum(c for _, c, _ in full_steps) == n - 1 and full_steps[0][0] == 1
    assert plan_from(lv, 0, 0, batch) == (full_steps, full_order)  # the empty index starts like it
    bounds = [f for f, _, _ in full_steps]
    for n0 in sorted(set(bounds[:8] + bounds[::max(1, len(bounds) // 16)] + bounds[-3:])):
        steps, order = plan_from(lv, n0, 0, batch)
        assert steps == [s for s in full_steps if s[0] >= n0] and order == full_order, n0
    assert plan_from(lv, n, 0, batch)[0] == []  # nothing left to insert


@pytest.mark.timeout(900)
def test_host_paths_under_address_sanitizer():
    csrc = os.path.join(ROOT, "islands_amd", "csrc")
    exe = os.path.join(ROOT, "islands_amd", "lib", "asan", "index_insert_host")
    subprocess.check_call(["make", "-C", csrc, exe.replace(os.path.join(ROOT, "islands_amd"), ".."), "-j", "4", "-s"])
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1:halt_on_error=1")
    # without a gfx950 the program also takes the way out of a non-empty insert at its first device call
    mode = ["nodevice"] if ia.device_count() == 0 else []
    pr = subprocess.run([exe] + mode, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = pr.stdout.decode(errors="replace")
    assert pr.returncode == 0 and "index insert host: ok" in out and "AddressSanitizer" not in out, out[-3000:]
