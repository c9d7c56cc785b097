"""isl_index_remove without a device: the symbol, every argument check a handle without resident rows can reach
in its order (an earlier check wins when two apply), the call that changes nothing, properties of the Python
definition alone (tests/_remove_ref.py over small random graphs, distances through the oracle), the planning
header through tests/cpp/remove_plan_dump.cpp (g++ alone), and the same argument checks under AddressSanitizer in
a stand-alone program (tests/cpp/index_remove_host.cpp over the library's own sources, host code instrumented)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import islands_amd as ia
import _remove_ref as rref
from islands_amd import _ffi
from _data import uniform_vectors
from test_index_insert_cpu import error_of, ring

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REMOVED = rref.REMOVED


def raw(idx, ids, n_ids, opts=None, remap=None, out_len=None):
    lib = _ffi.lib()
    st = lib.isl_index_remove(idx, opts, None if ids is None else ids.ctypes.data_as(C.c_void_p), n_ids,
                              None if remap is None else remap.ctypes.data_as(C.c_void_p), out_len)
    return lib.isl_status_name(st).decode(), lib.isl_last_error_message().decode()


def test_symbol_is_exported_and_declared():
    assert "isl_index_remove" in _ffi.SIGNATURES
    fn = _ffi.lib().isl_index_remove
    assert fn.restype is C.c_int32 and len(fn.argtypes) == 6
    header = open(os.path.join(ROOT, "include", "islands_amd.h")).read()
    assert "isl_status isl_index_remove(isl_index* idx, const isl_build_options* opts, const uint64_t* ids" in header
    assert "#define ISL_REMOVED UINT64_MAX" in header and "#define ISL_REMOVE_MAX_CANDIDATES 512u" in header
    assert _ffi.lib().isl_abi_version() == 3
    assert ia.REMOVED == REMOVED == 2 ** 64 - 1 and rref.MAX_CANDIDATES == 512


def test_checks_in_their_order():
    empty = ia.LeannIndex(ia.LeannConfig(m=8, m0=16, ef_construction=40))
    full = ring()
    blobs = empty.to_bytes(), full.to_bytes()
    ids = np.array([3, 99, 5], np.uint64)
    remap = np.full(12, 77, np.uint64)
    out_len = C.c_uint64(77)
    bad = _ffi.BuildOptionsC()
    _ffi.lib().isl_build_options_default(C.byref(bad))
    bad.select_rule = 7
    # 1. NULL idx, NULL ids with n_ids > 0 -- before the options
    assert raw(None, ids, 3, C.byref(bad), remap, C.byref(out_len))[0] == "InvalidArgument"
    kind, msg = raw(full._h, None, 3, C.byref(bad), remap, C.byref(out_len))
    assert kind == "InvalidArgument" and "NULL" in msg
    # 2. the options, as isl_index_build_ex checks them -- before n_ids == 0 and before the ids are looked at
    v = uniform_vectors(8, 16, 1)
    assert error_of(ia.LeannIndex.build, v, select=7).kind == error_of(full.remove, [99], select=7).kind == "InvalidArgument"
    assert (error_of(ia.LeannIndex.build, v, select="diverse", alpha=0.5).kind
            == error_of(full.remove, [99], select="diverse", alpha=0.5).kind == "InvalidConfig")
    assert raw(full._h, ids, 0, C.byref(bad), remap, C.byref(out_len))[0] == "InvalidArgument"
    bad.select_rule, bad.alpha = 1, float("nan")
    assert raw(full._h, ids, 0, C.byref(bad), remap, C.byref(out_len))[0] == "InvalidConfig"
    assert remap.tolist() == [77] * 12 and out_len.value == 77
    # 3. no ids: ISL_OK, nothing changed, the identity -- before the handle is looked at
    hnsw = ia.HnswGraph.build(np.zeros((0, 0), np.float32), m=4, m0=8, ef_construction=16)
    core = C.c_void_p.from_address(hnsw._h.value)  # isl_hnsw's first member: the layer-0 isl_index
    assert raw(core, ids, 0, None, remap, C.byref(out_len))[0] == "Ok" and out_len.value == 0
    assert full.remove([]).tolist() == list(range(12)) and empty.remove([]).tolist() == []
    out_len.value = 77
    # 4. the core index of an HnswGraph -- before the ids are compared with len (here 0)
    kind, msg = raw(core, ids, 3, None, remap, C.byref(out_len))
    assert kind == "Unsupported" and "HnswGraph" in msg and out_len.value == 77
    # 5. an id that is not below len, with the payload -- before the rows are missed and before m0 is looked at
    e = error_of(full.remove, ids)
    assert e.kind == "NodeNotFound" and e.node == 99
    e = error_of(full.remove, [12])
    assert e.kind == "NodeNotFound" and e.node == 12
    e = error_of(empty.remove, [0])
    assert e.kind == "NodeNotFound" and e.node == 0
    wide = ring(m=64, m0=129, ef_construction=200)
    assert error_of(wide.remove, [4, 12]).kind == "NodeNotFound"
    # 6. a non-empty index without resident rows -- before m0 > 128
    for idx in (full, wide):
        e = error_of(idx.remove, [3, 5, 3])
        assert e.kind == "Unsupported" and "resident" in str(e)
    kind, _ = raw(full._h, np.array([3], np.uint64), 1, None, remap, C.byref(out_len))
    assert kind == "Unsupported" and remap.tolist() == [77] * 12 and out_len.value == 77  # written only on ISL_OK
    # (7. m0 > 128 and 8. a busy lane need resident rows: tests/test_gpu_index_remove.py)
    assert (empty.to_bytes(), full.to_bytes()) == blobs and len(full) == 12 and len(empty) == 0


def test_no_ids_is_ok_and_changes_nothing():
    full = ring()
    blob = full.to_bytes()
    remap = np.full(12, 77, np.uint64)
    out_len = C.c_uint64(77)
    assert raw(full._h, None, 0, None, remap, C.byref(out_len))[0] == "Ok"
    assert remap.tolist() == list(range(12)) and out_len.value == 12
    assert raw(full._h, None, 0)[0] == "Ok"  # out_remap and out_len may be NULL
    assert full.to_bytes() == blob and len(full) == 12 and full.entry_point == 0


# ---------------------------------------------------------------- the Python definition alone
def random_graph(orc, n, m0, seed, levels=None):
    """lists of up to m0 distinct ids without self loops, as an oracle Csr"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        k = int(rng.integers(0, m0 + 1))
        rows.append([int(x) for x in rng.permutation(np.delete(np.arange(n), i))[:k]])
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    g = orc.Csr(off, np.array([x for r in rows for x in r], np.uint64), 0)
    if levels is not None:
        g.levels = np.asarray(levels, np.uint64)
        g.max_level = int(g.levels[0])
    return g, rows


@pytest.mark.parametrize("rule", ["reference", "diverse"])
@pytest.mark.parametrize("count", [1, 9, 40])
def test_definition_properties(orc, rule, count):
    n, m0 = 60, 6
    v = uniform_vectors(n, 8, 3)
    g, rows = random_graph(orc, n, m0, 11)
    rng = np.random.default_rng(count)
    ids = rng.choice(n, count, replace=False)
    gone = set(ids.tolist())
    out, remap = rref.remove(orc, g, v, ids, m0, 1, rule)
    keep = [i for i in range(n) if i not in gone]
    assert out.num_nodes == n - count and remap.shape == (n,)
    assert [int(remap[i]) for i in keep] == list(range(n - count)) and all(remap[i] == REMOVED for i in gone)
    new = rref.lists_of(out)
    back = {int(remap[i]): i for i in keep}
    for p, r in enumerate(new):
        old = [back[x] for x in r]  # ids < new len, or this raises
        assert len(r) <= m0 and len(set(r)) == len(r) and p not in r and not gone & set(old)
        if not gone & set(rows[back[p]]):  # untouched: the old list through the remap
            assert old == rows[back[p]]
    assert out.degree_counts.tolist() == [len(r) for r in new]


def test_removing_twice_never_leaves_a_removed_id(orc):
    n, m0 = 50, 5
    v = uniform_vectors(n, 8, 4)
    g, _ = random_graph(orc, n, m0, 12)
    a, b = [3, 17, 20, 21, 40], [0, 5, 16, 30]  # b in the ids after the first removal
    g1, remap1 = rref.remove(orc, g, v, a, m0, 0, "diverse")
    keep1 = [i for i in range(n) if remap1[i] != REMOVED]
    g2, remap2 = rref.remove(orc, g1, v[keep1], b, m0, 0, "diverse")
    origin = [keep1[i] for i in range(len(keep1)) if remap2[i] != REMOVED]  # new id -> first id
    dead = set(a) | {keep1[i] for i in b}
    assert g2.num_nodes == n - 9 and not dead & set(origin)
    for p, r in enumerate(rref.lists_of(g2)):
        assert not dead & {origin[x] for x in r} and p not in r and len(r) <= m0


def test_entry_point_rule(orc):
    n = 12
    lv = [0, 2, 5, 1, 3, 3, 0, 5, 2, 0, 3, 1]
    v = uniform_vectors(n, 4, 5)
    g, _ = random_graph(orc, n, 3, 13, lv)
    g.entry_point, g.max_level = 2, 5
    out, remap = rref.remove(orc, g, v, [0, 4], 3)
    assert (out.entry_point, out.max_level) == (1, 5)  # it survives: kept, remapped
    out, _ = rref.remove(orc, g, v, [2], 3)
    assert (out.entry_point, out.max_level) == (6, 5)  # node 7 holds the highest level left
    out, _ = rref.remove(orc, g, v, [2, 7, 0], 3)
    assert (out.entry_point, out.max_level) == (2, 3)  # nodes 4, 5, 10 share level 3: the lowest new id
    assert out.levels.tolist() == [2, 1, 3, 3, 0, 2, 0, 3, 1]
    out, _ = rref.remove(orc, g, v, list(range(n)), 3)
    assert out.num_nodes == 0 and out.entry_point is None and out.max_level == 0
    g.entry_point = None
    out, _ = rref.remove(orc, g, v, [2], 3)
    assert out.entry_point is None


# ---------------------------------------------------------------- the planning header
@pytest.fixture(scope="module")
def plan():
    exe = os.path.join(ROOT, "islands_amd", "lib", "remove_plan_dump")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "remove_plan_dump.cpp"),
                           "-o", exe])

    def run(n0, entry, max_level, levels, ids):
        text = (f"{n0} {0 if entry is None else 1} {entry or 0} {max_level} {0 if levels is None else 1} {len(ids)}\n"
                + " ".join(str(int(x)) for x in (levels if levels is not None else [])) + "\n"
                + " ".join(str(int(x)) for x in ids) + "\n")
        out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60, check=True).stdout
        return [ln.split() for ln in out.splitlines()]

    return run


def test_plan_header(plan):
    rng = np.random.default_rng(2)
    for n0, count in ((1, 1), (12, 3), (12, 12), (300, 1), (300, 170)):
        lv = rng.integers(0, 4, n0).tolist()
        ids = rng.choice(n0, count, replace=False).tolist()
        ids += ids[:2]  # repeated ids count once
        entry = int(np.argmax(lv))
        lines = plan(n0, entry, max(lv), lv, ids)
        remap, keep = rref.remap_of(n0, set(ids))
        want_entry, want_top = rref.entry_after(lv, keep, remap, entry, max(lv))
        got = {ln[0]: ln[1:] for ln in lines if ln[0] in ("len", "remap", "survivors", "entry", "levels", "cap")}
        assert int(got["len"][0]) == len(keep) and [int(x) for x in got["survivors"]] == keep
        assert [int(x) for x in got["remap"]] == [-1 if r == REMOVED else int(r) for r in remap]
        assert [int(x) for x in got["entry"]] == [0 if want_entry is None else 1, want_entry or 0, want_top]
        assert [int(x) for x in got["levels"]] == [lv[i] for i in keep]
        assert got["cap"] == ["512"]
    # an entry point that goes: the lowest new id of the highest level; levels absent: all 0, new id 0
    lines = {ln[0]: ln[1:] for ln in plan(6, 2, 9, [0, 4, 9, 4, 1, 4], [2, 0])}
    assert lines["entry"] == ["1", "0", "4"]
    assert {ln[0]: ln[1:] for ln in plan(6, 2, 0, None, [2, 0])}["entry"] == ["1", "0", "0"]
    assert {ln[0]: ln[1:] for ln in plan(6, None, 0, None, [2])}["entry"][0] == "0"
    assert plan(6, 0, 0, None, [1, 6, 9]) == [["unknown", "6"]]
    # the worst emission and the LDS of the repair kernel: tile + query + four lists of 512 + a row of m0
    rows = plan(1, 0, 0, None, [0])
    assert [ln[1:] for ln in rows if ln[0] == "worst"] == [[str(m), str(m + m * m)] for m in (8, 64, 96, 128)]
    assert ["worst", "128", "16512"] in rows
    tile = 16 * 80 * 4
    for ln in rows:
        if ln[0] == "lds":
            d, m0, got = int(ln[2]), int(ln[3]), int(ln[4])
            query = ((d + 3) // 4 * 4 + 16) if ln[1] == "f32" else ((d + 31) // 32 * 32 + 16)
            assert got == (tile if ln[1] == "f32" else 0) + query * 4 + 512 * 16 + m0 * 4
            assert got < 64 * 1024  # a wave's share of a CU's LDS leaves room for several waves


@pytest.mark.timeout(900)
def test_host_paths_under_address_sanitizer():
    csrc = os.path.join(ROOT, "islands_amd", "csrc")
    exe = os.path.join(ROOT, "islands_amd", "lib", "asan", "index_remove_host")
    subprocess.check_call(["make", "-C", csrc, exe.replace(os.path.join(ROOT, "islands_amd"), ".."), "-j", "4", "-s"])
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1:halt_on_error=1")
    pr = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = pr.stdout.decode(errors="replace")
    assert pr.returncode == 0 and "index remove host: ok" in out and "AddressSanitizer" not in out, out[-3000:]
