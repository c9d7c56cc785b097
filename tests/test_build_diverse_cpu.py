"""No GPU: the ABI additions of the diverse selection rule (isl_build_options, isl_index_build_ex,
isl_select_neighbors), their argument checks, and the Python restatement of the rule against a
case worked out by hand."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import islands_amd as ia
from islands_amd import _ffi

import _diverse_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("isl_build_options_default", "isl_index_build_ex", "isl_select_neighbors")


def test_symbols_are_exported_and_declared():
    l = _ffi.lib()
    header = open(os.path.join(ROOT, "include", "islands_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(l, name)
        assert name in _ffi.SIGNATURES
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert "ISL_SELECT_REFERENCE = 0" in header and "ISL_SELECT_DIVERSE = 1" in header
    assert l.isl_abi_version() == 3  # additions only


def test_default_options():
    o = _ffi.BuildOptionsC()
    _ffi.lib().isl_build_options_default(C.byref(o))
    assert (o.select_rule, o.alpha, o.keep_pruned, o.batch) == (ia.SELECT_REFERENCE, 1.0, 1, 1)
    assert o.struct_size == C.sizeof(_ffi.BuildOptionsC) == 24


def _build_ex(opts, v):
    cfg = ia.LeannConfig()._to_c()
    h = C.c_void_p()
    st = _ffi.lib().isl_index_build_ex(C.byref(cfg), C.byref(opts), v.ctypes.data_as(C.c_void_p), v.shape[0],
                                       v.shape[1], None, 0, 0, C.byref(h))
    assert not h.value
    return _ffi.lib().isl_status_name(st).decode()


@pytest.mark.parametrize("alpha", [0.5, math.nan, math.inf])
def test_bad_alpha_is_invalid_config(alpha):
    v = np.ones((4, 8), np.float32)
    with pytest.raises(ia.CoreError) as ex:
        ia.LeannIndex.build(v, select="diverse", alpha=alpha)
    assert ex.value.kind == "InvalidConfig"


def test_unknown_rule_and_short_struct_are_invalid_argument():
    v = np.ones((4, 8), np.float32)
    o = _ffi.BuildOptionsC()
    _ffi.lib().isl_build_options_default(C.byref(o))
    o.select_rule = 7
    assert _build_ex(o, v) == "InvalidArgument"
    _ffi.lib().isl_build_options_default(C.byref(o))
    o.struct_size = 4
    assert _build_ex(o, v) == "InvalidArgument"
    with pytest.raises(ValueError):
        ia.LeannIndex.build(v, select="nearest")


def test_rule_from_the_environment(monkeypatch):
    monkeypatch.setenv("ISL_BUILD_SELECT", "diverse")
    assert ia.LeannIndex._build_options(None, 1.0, True).select_rule == ia.SELECT_DIVERSE
    monkeypatch.delenv("ISL_BUILD_SELECT")
    assert ia.LeannIndex._build_options(None, 1.0, True).select_rule == ia.SELECT_REFERENCE
    assert ia.LeannIndex._build_options("diverse", 1.2, False, 64).batch == 64


def test_empty_input_builds_an_empty_index():
    e = ia.LeannIndex.build(np.zeros((0, 0), np.float32), select="diverse")
    assert e.is_empty() and len(e) == 0


def test_select_neighbors_argument_checks():
    idx = ia.LeannIndex()  # no rows anywhere
    with pytest.raises(ia.CoreError) as ex:
        idx.select_neighbors([0], [[1, 2]], 2, alpha=0.5)
    assert ex.value.kind == "InvalidConfig"
    with pytest.raises(ia.CoreError) as ex:
        idx.select_neighbors([0], [[1, 2]], 129)
    assert ex.value.kind == "Unsupported"
    with pytest.raises(ia.CoreError) as ex:
        idx.select_neighbors([0], [[1, 2]], 2)
    assert ex.value.kind == "Unsupported"  # no float32 rows on a device


def test_reference_select_on_a_hand_made_case(orc):
    """Base 0 at the origin, Euclidean.  By distance from the base: 1 (1.0), 3 (1.5), 2 (2.0), 4 (3.0),
    5 (4.0).  2 lies on the ray through 1: d(1, 2) = 1 <= 2, occluded.  3 and 4 are far from what is
    kept before them (d(1, 3) = 1.80 > 1.5; d(1, 4) = 4, d(3, 4) = 3.35 > 3).  5 sits behind 3:
    d(3, 5) = 2.5 <= 4, occluded.  The occluded ones come back only as fillers, after the kept."""
    v = np.array([[0, 0], [1, 0], [2, 0], [0, 1.5], [-3, 0], [0, 4]], dtype=np.float32)
    e = int(ia.DistanceMetric.Euclidean)
    cand = [5, 4, 3, 2, 1]  # any order
    assert ref.select(orc, v, e, 0, cand, 5) == [1, 3, 4, 2, 5]
    assert ref.select(orc, v, e, 0, cand, 4) == [1, 3, 4, 2]
    assert ref.select(orc, v, e, 0, cand, 4, keep_pruned=False) == [1, 3, 4]
    assert ref.select(orc, v, e, 0, cand, 2) == [1, 3]
    assert ref.select(orc, v, e, 0, cand, 1) == [1]
    # alpha = 2: 2 * d(1, 2) = 2 <= 2 still occludes 2 (equality occludes); 2 * d(3, 5) = 5 > 4 frees 5
    assert ref.select(orc, v, e, 0, cand, 4, alpha=2.0) == [1, 3, 4, 5]
    assert ref.select(orc, v, e, 0, cand, 5, alpha=2.0, keep_pruned=False) == [1, 3, 4, 5]
    # a repeated id is a second entry at distance 0 from the first: occluded by it
    assert ref.select(orc, v, e, 0, [3, 1, 3], 3) == [1, 3, 3]
    assert ref.select(orc, v, e, 0, [3, 1, 3], 3, keep_pruned=False) == [1, 3]
    assert ref.select(orc, v, e, 0, [], 3) == []


def test_reference_build_on_a_line(orc):
    """Five points on a line, m0 = 2: under the diverse rule with no fill a node keeps one neighbour
    per side (everything further along the ray is occluded), so the graph is the path."""
    v = np.array([[0, 0], [1, 0], [2, 0], [3, 0], [4, 0]], dtype=np.float32)
    g = ref.build(orc, v, 2, 8, metric=int(ia.DistanceMetric.Euclidean), keep_pruned=False)
    rows = [sorted(g.get_neighbors(i)) for i in range(5)]
    assert rows == [[1], [0, 2], [1, 3], [2, 4], [3]]
    assert g.entry_point == 0 and g.max_level == 0
