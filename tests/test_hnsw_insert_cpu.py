"""isl_hnsw_insert without a device: the planner that starts at node n0 (plan_steps_from of build_plan.hpp,
through tests/cpp/insert_plan_dump.cpp built with g++ alone) and every part of the entry point that needs no
GPU (argument checks in their order, the empty graph, the symbol)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import islands_amd as ia
import _hnsw_build_ref as ref
from islands_amd import _ffi
from _data import random_levels, uniform_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def forced_levels(n=300):
    lv = np.zeros(n, np.uint64)
    lv[5], lv[40], lv[100], lv[101], lv[200] = 3, 1, 5, 5, 2
    return lv


LEVELS = [("forced", forced_levels), ("random9", lambda: random_levels(9, 16, 49)),
          ("random400", lambda: random_levels(400, 4, 71)), ("random233", lambda: random_levels(233, 2, 5))]


@pytest.mark.parametrize("batch", [1, 7, 256])
@pytest.mark.parametrize("levels", [c[1] for c in LEVELS], ids=[c[0] for c in LEVELS])
def test_plan_from_a_step_boundary_is_the_tail(plan_from, levels, batch):
    lv = levels()
    full_steps, full_order = plan_from(lv, 1, int(lv[0]), batch)
    assert [(0, 1)] + [(f, c) for f, c, _ in full_steps] == ref.plan_steps(lv, batch)  # n0 = 1 is plan_steps
    assert plan_from(lv, 0, 0, batch) == (full_steps, full_order)  # the empty graph starts like it
    for n0 in [f for f, _, _ in full_steps]:  # every boundary of the full plan
        steps, order = plan_from(lv, n0, int(lv[:n0].max()), batch)
        tail = [s for s in full_steps if s[0] >= n0]
        assert steps == tail, n0
        assert order[:n0] == list(range(n0)) and order[n0:] == full_order[n0:], n0


@pytest.mark.parametrize("batch", [1, 7, 256])
def test_plan_from_anywhere(plan_from, batch):
    lv = random_levels(400, 3, 17)
    n = len(lv)
    for n0 in (1, 2, 3, 8, 9, 17, 63, 64, 100, 255, 256, 399, 400):
        steps, order = plan_from(lv, n0, int(lv[:n0].max()), batch)
        assert sorted(order) == list(range(n)) and order[:n0] == list(range(n0))
        at, top = n0, int(lv[:n0].max())
        for first, count, stop in steps:  # the steps partition [n0, n)
            assert first == at and 1 <= count <= min(batch, max(1, first // 8))
            ids = order[first:first + count]
            assert sorted(ids) == list(range(first, first + count))
            lvs = [int(lv[i]) for i in ids]
            assert lvs == sorted(lvs, reverse=True) and stop == lvs[0]  # inside a step levels descend
            assert ids == sorted(range(first, first + count), key=lambda i: -int(lv[i]))  # ... equal levels in id order
            if stop > top:  # a node above the running max level is alone
                assert count == 1
            top = max(top, stop)
            at += count
        assert at == n


def empty_graph(**kw):
    cfg = dict(m=8, m0=16, ef_construction=64, metric=1, ml=1.0 / np.log(8))
    cfg.update(kw)
    return ia.HnswGraph.build(np.zeros((0, 0), np.float32), **cfg)


def kind_of(g, *a, **kw):
    with pytest.raises(ia.CoreError) as e:
        g.insert(*a, **kw)
    return e.value.kind


def test_insert_checks_without_a_device():
    lib = _ffi.lib()
    v = uniform_vectors(8, 4, 1)
    first = C.c_uint64(77)
    st = lib.isl_hnsw_insert(None, None, v.ctypes.data_as(C.c_void_p), 8, 4, None, 0, 0, C.byref(first))
    assert lib.isl_status_name(st).decode() == "InvalidArgument"
    g = empty_graph()
    blob = g.to_bytes()
    st = lib.isl_hnsw_insert(g._h, None, None, 8, 4, None, 0, 0, None)  # NULL rows, n_new > 0
    assert lib.isl_status_name(st).decode() == "InvalidArgument"
    # the options, as isl_hnsw_build checks them
    with pytest.raises(ia.CoreError) as e:
        ia.HnswGraph.build(v, select=7)
    assert kind_of(g, v, select=7) == e.value.kind == "InvalidArgument"
    with pytest.raises(ia.CoreError) as e:
        ia.HnswGraph.build(v, select="diverse", alpha=0.5)
    assert kind_of(g, v, select="diverse", alpha=0.5) == e.value.kind == "InvalidConfig"
    assert kind_of(g, v, select=7, levels=[99] * 8) == "InvalidArgument"  # options before the data
    # no rows: ISL_OK, nothing changed (before the dimension is looked at)
    assert g.insert(np.zeros((0, 5), np.float32)) == 0 and len(g) == 0 and g.to_bytes() == blob
    assert kind_of(g, np.zeros((4, 0), np.float32)) == "EmptyCollection"
    assert kind_of(g, v, levels=[0, 1, 16, 0, 0, 0, 0, 0]) == "InvalidArgument"
    assert kind_of(empty_graph(max_layers=3), v, levels=[0, 1, 3, 0, 0, 0, 0, 0]) == "InvalidArgument"
    # levels before the shape limits
    wide = empty_graph(m=16, m0=129, ef_construction=200)
    assert kind_of(wide, v, levels=[99] * 8) == "InvalidArgument"
    assert kind_of(wide, v, levels=[0] * 8) == "Unsupported"
    with pytest.raises(ValueError):
        g.insert(v, levels=[0, 0])
    assert g.to_bytes() == blob


def test_insert_without_a_device_leaves_the_empty_graph():
    """No CPU fallback: with no gfx950 a non-empty insert reports Device and the empty graph is still empty and
    serialisable.  (Where this runs beside a device the same call succeeds; the GPU tests say what it built.)"""
    g = empty_graph()
    blob = g.to_bytes()
    v = uniform_vectors(8, 4, 1)
    if ia.device_count() == 0:
        assert kind_of(g, v, levels=[0] * 8) == "Device"
        assert len(g) == 0 and g.entry_point is None and g.to_bytes() == blob
        assert ia.HnswGraph.from_bytes(blob).to_bytes() == blob
    else:
        assert g.insert(v, levels=[0] * 8) == 0 and len(g) == 8 and g.entry_point == 0


def test_symbol_is_exported_and_declared():
    assert "isl_hnsw_insert" in _ffi.SIGNATURES
    fn = _ffi.lib().isl_hnsw_insert
    assert fn.restype is C.c_int32 and len(fn.argtypes) == 9
    header = open(os.path.join(ROOT, "include", "islands_amd.h")).read()
    assert "isl_status isl_hnsw_insert(isl_hnsw* h, const isl_build_options* opts" in header
