"""isl_hnsw_remove without a device: the symbol, every argument check a handle without a device can reach in its
order (an earlier check wins when two apply; out-parameters untouched on failure), the call that changes nothing,
properties of the Python definition alone (tests/_hnsw_remove_ref.py over small random multi-layer graphs,
distances through the oracle), the seeds of the GPU tests against that definition, the planning header through
tests/cpp/hnsw_remove_plan_dump.cpp (g++ alone), and the argument checks under AddressSanitizer in a stand-alone
program (tests/cpp/hnsw_remove_host.cpp over the library's own sources, host code instrumented)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import islands_amd as ia
import _hnsw_build_ref as ref
import _hnsw_remove_ref as href
import _remove_ref as rref
from islands_amd import _ffi
from _data import random_levels, uniform_vectors
from test_hnsw_insert_cpu import empty_graph
from test_index_insert_cpu import error_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REMOVED = href.REMOVED


def raw(h, ids, n_ids, opts=None, remap=None, out_len=None):
    lib = _ffi.lib()
    st = lib.isl_hnsw_remove(h, opts, None if ids is None else ids.ctypes.data_as(C.c_void_p), n_ids,
                             None if remap is None else remap.ctypes.data_as(C.c_void_p), out_len)
    return lib.isl_status_name(st).decode(), lib.isl_last_error_message().decode()


def test_symbol_is_exported_and_declared():
    assert "isl_hnsw_remove" in _ffi.SIGNATURES
    fn = _ffi.lib().isl_hnsw_remove
    assert fn.restype is C.c_int32 and len(fn.argtypes) == 6
    header = open(os.path.join(ROOT, "include", "islands_amd.h")).read()
    assert "isl_status isl_hnsw_remove(isl_hnsw* h, const isl_build_options* opts, const uint64_t* ids" in header
    assert _ffi.lib().isl_abi_version() == 3
    assert ia.REMOVED == REMOVED == 2 ** 64 - 1
    assert callable(ia.HnswGraph.remove)
    mirror = open(os.path.join(ROOT, "include", "islands_amd.hpp")).read()
    assert "isl_hnsw_remove(h_, &opts" in mirror


def test_checks_in_their_order():
    g = empty_graph()
    blob = g.to_bytes()
    ids = np.array([3, 99, 5], np.uint64)
    remap = np.full(12, 77, np.uint64)
    out_len = C.c_uint64(77)
    bad = _ffi.BuildOptionsC()
    _ffi.lib().isl_build_options_default(C.byref(bad))
    bad.select_rule = 7
    # 1. NULL h, NULL ids with n_ids > 0 -- before the options
    assert raw(None, ids, 3, C.byref(bad), remap, C.byref(out_len))[0] == "InvalidArgument"
    kind, msg = raw(g._h, None, 3, C.byref(bad), remap, C.byref(out_len))
    assert kind == "InvalidArgument" and "NULL" in msg
    # 2. the options, as isl_hnsw_build checks them -- before n_ids == 0 and before the ids are looked at
    v = uniform_vectors(8, 4, 1)
    assert error_of(ia.HnswGraph.build, v, select=7).kind == error_of(g.remove, [99], select=7).kind == "InvalidArgument"
    assert (error_of(ia.HnswGraph.build, v, select="diverse", alpha=0.5).kind
            == error_of(g.remove, [99], select="diverse", alpha=0.5).kind == "InvalidConfig")
    assert raw(g._h, ids, 0, C.byref(bad), remap, C.byref(out_len))[0] == "InvalidArgument"
    bad.select_rule, bad.alpha = 1, float("nan")
    assert raw(g._h, ids, 0, C.byref(bad), remap, C.byref(out_len))[0] == "InvalidConfig"
    assert remap.tolist() == [77] * 12 and out_len.value == 77
    # 3. no ids: ISL_OK, nothing changed, the identity -- before the ids or the handle's rows are looked at
    assert raw(g._h, ids, 0, None, remap, C.byref(out_len))[0] == "Ok" and out_len.value == 0
    assert remap.tolist() == [77] * 12 and g.remove([]).tolist() == []
    out_len.value = 77
    # 4. an id that is not below len (here 0), with the payload -- before m0 is looked at
    e = error_of(g.remove, ids)
    assert e.kind == "NodeNotFound" and e.node == 3
    wide = empty_graph(m=16, m0=129, ef_construction=200)
    e = error_of(wide.remove, [0, 4])
    assert e.kind == "NodeNotFound" and e.node == 0
    kind, _ = raw(g._h, ids, 3, None, remap, C.byref(out_len))
    assert kind == "NodeNotFound" and remap.tolist() == [77] * 12 and out_len.value == 77  # written only on ISL_OK
    # (5. - 8. need a graph with nodes: tests/cpp/hnsw_remove_host.cpp for 5, tests/test_gpu_hnsw_remove.py)
    assert g.to_bytes() == blob and len(g) == 0 and g.entry_point is None
    # isl_index_remove on the core index of an HnswGraph stays refused
    core = C.c_void_p.from_address(g._h.value)  # isl_hnsw's first member: the layer-0 isl_index
    st = _ffi.lib().isl_index_remove(core, None, ids.ctypes.data_as(C.c_void_p), 3, None, None)
    assert _ffi.lib().isl_status_name(st).decode() == "Unsupported"


def test_no_ids_is_ok_and_changes_nothing():
    g = empty_graph()
    blob = g.to_bytes()
    out_len = C.c_uint64(77)
    assert raw(g._h, None, 0, None, None, C.byref(out_len))[0] == "Ok" and out_len.value == 0
    assert raw(g._h, None, 0)[0] == "Ok"  # out_remap and out_len may be NULL
    assert g.to_bytes() == blob and len(g) == 0


# ---------------------------------------------------------------- the Python definition alone
def random_layers(n, m, m0, levels, seed, strays=True):
    """per layer, for every node that has it, a list of up to M_L distinct ids of other nodes that have it; with
    `strays` a few upper lists also name a node that lacks the layer (what HnswGraph::insert leaves behind a node
    that rises above the top layer)"""
    rng = np.random.default_rng(seed)
    top = int(max(levels))
    layers = []
    for L in range(top + 1):
        have = [i for i in range(n) if levels[i] >= L]
        cap = m0 if L == 0 else m
        rows = [[] for _ in range(n)]
        for i in have:
            others = [x for x in have if x != i]
            k = int(rng.integers(min(cap, len(others)) // 2, min(cap, len(others)) + 1))
            rows[i] = [int(x) for x in rng.permutation(others)[:k]]
            lack = [x for x in range(n) if levels[x] < L]
            if strays and L and lack and len(rows[i]) < cap and rng.random() < 0.3:
                rows[i].insert(int(rng.integers(0, len(rows[i]) + 1)), int(rng.choice(lack)))
        layers.append(rows)
    return layers


def small_graph(seed, n=60, m=3, m0=6):
    lv = [int(x) for x in random_levels(n, 3, seed)]
    top = max(lv)
    entry = lv.index(top)
    return lv, random_layers(n, m, m0, lv, seed + 1), entry, top


@pytest.mark.parametrize("rule", ["reference", "diverse"])
@pytest.mark.parametrize("count", [1, 9, 40])
def test_definition_properties(orc, rule, count):
    n, m, m0 = 60, 3, 6
    v = uniform_vectors(n, 8, 3)
    lv, layers, entry, top = small_graph(21)
    assert top >= 2
    ids = np.random.default_rng(count).choice(n, count, replace=False)
    gone = set(ids.tolist())
    stats = []
    s = href.remove(orc, layers, lv, entry, top, v, ids, m, m0, 1, rule, stats=stats)
    keep = [i for i in range(n) if i not in gone]
    assert len(s) == n - count and s.remap.shape == (n,)
    assert [int(s.remap[i]) for i in keep] == list(range(n - count)) and all(s.remap[i] == REMOVED for i in gone)
    assert s.levels == [lv[i] for i in keep]  # levels are kept
    assert len(s.layers) == s.max_level + 1 and s.max_level == max(s.levels)
    for L, rows in enumerate(s.layers):
        cap = m0 if L == 0 else m
        assert len(rows) == len(keep)
        for p, r in enumerate(rows):
            old = [keep[x] for x in r]  # ids below the new len, or this raises
            assert len(r) <= cap and len(set(r)) == len(r) and p not in r and not gone & set(old), (L, p)
            if s.levels[p] < L:
                assert r == []
            elif not gone & set(layers[L][keep[p]]):  # untouched: the old list through the remap
                assert old == layers[L][keep[p]], (L, p)
    assert stats and all(lv[p] >= L and p not in gone for L, p, _ in stats)
    if count == 9:  # some list outgrew its cap on layer 0 and above it: the sort and the rule ran
        assert max(c for L, _, c in stats if L == 0) > m0 and max(c for L, _, c in stats if L >= 1) > m


def test_a_removed_node_that_lacks_the_layer_emits_nothing(orc):
    """node 0 has level 0 and is named on layer 1 by node 1; its layer-0 list must not leak into layer 1"""
    lv = [0, 1, 1, 0]
    layers = [[[1, 2, 3], [0, 2], [1], [0]], [[], [0, 2], [1, 0], []]]
    v = uniform_vectors(4, 4, 1)
    s = href.remove(orc, layers, lv, 1, 1, v, [0], 2, 4)
    assert s.layers == [[[1, 2], [0], [0, 1]], [[1], [0], []]] and (s.entry, s.max_level) == (0, 1)
    # a surviving node that lacks the layer stays where it is named
    s = href.remove(orc, layers, lv, 1, 1, v, [3], 2, 4)
    assert s.layers[1] == [[], [0, 2], [1, 0]] and s.layers[0] == [[1, 2], [0, 2], [1]]


def test_entry_point_rule(orc):
    n = 12
    lv = [0, 2, 3, 1, 2, 2, 0, 3, 2, 0, 2, 1]
    v = uniform_vectors(n, 4, 5)
    layers = random_layers(n, 2, 4, lv, 13)
    s = href.remove(orc, layers, lv, 2, 3, v, [0, 4], 2, 4)
    assert (s.entry, s.max_level, len(s.layers)) == (1, 3, 4)  # the entry survives: kept, remapped
    s = href.remove(orc, layers, lv, 2, 3, v, [2], 2, 4)
    assert (s.entry, s.max_level, len(s.layers)) == (6, 3, 4)  # removed, node 7 shares the top level
    s = href.remove(orc, layers, lv, 2, 3, v, [2, 7, 0], 2, 4)
    assert (s.entry, s.max_level, len(s.layers)) == (0, 2, 3)  # the top level emptied: max_level drops
    assert s.levels == [2, 1, 2, 2, 0, 2, 0, 2, 1] and all(r == [] for r in s.layers[2][1:2])
    s = href.remove(orc, layers, lv, 2, 3, v, [i for i in range(n) if lv[i] >= 1], 2, 4)
    assert (s.entry, s.max_level, len(s.layers)) == (0, 0, 1)
    s = href.remove(orc, layers, lv, 2, 3, v, list(range(n)), 2, 4)
    assert (len(s), s.entry, s.max_level, s.layers) == (0, None, 0, [])


def test_the_definition_seeds_a_graph_that_searches_and_grows(orc):
    n, m, m0 = 80, 3, 6
    v = uniform_vectors(n + 5, 8, 9)
    lv = random_levels(n + 5, 3, 4)
    g = ref.build(orc, v[:n], lv[:n], m, m0, 20, 1, "diverse")
    s = href.remove(orc, href.layers_of_graph(g, n), lv[:n], g.entry, g.max_level, v[:n], [g.entry, 3, 4], m, m0, 1,
                    "diverse")
    rows = np.concatenate([v[:n][s.remap != REMOVED], v[n:]])
    seeded = href.seed_graph(ref.Graph(orc, rows, m, m0, 20, 1, "diverse"), s, rows)
    ids, dd = seeded.search(uniform_vectors(1, 8, 2)[0], 5, 20)
    assert len(ids) == 5 and all(0 <= i < n - 3 for i in ids) and list(dd) == sorted(dd)
    levels = s.levels + [int(x) for x in lv[n:]]
    for i in range(n - 3, n + 2):
        seeded.insert_step([i], levels)
    assert len(seeded.conn) == n + 2 and all(len(seeded.conn[i][0]) > 0 for i in range(n - 3, n + 2))


def test_seeds_of_the_gpu_tests_reach_the_sort_on_an_upper_layer(orc):
    """tests/test_gpu_hnsw_remove.py removes these ids from the device's graph of these rows, which with one node
    per step is this one (tests/test_gpu_hnsw_insert.py compares them): 333 removed ids push a list past M_L on
    layer 0 and on a layer above, every count touches some list."""
    from test_gpu_hnsw_remove import BASE, base_rows, pick_ids
    v, lv = base_rows()
    g = ref.build(orc, v, lv, BASE["m"], BASE["m0"], BASE["ef_construction"], 1, "diverse")
    assert g.max_level >= 3
    layers = href.layers_of_graph(g, 600)
    for count in (1, 20, 333):
        stats = []
        href.remove(orc, layers, lv, g.entry, g.max_level, v, pick_ids(layers, 600, count), BASE["m"], BASE["m0"], 1,
                    "diverse", stats=stats)
        assert stats
        if count == 333:
            assert max(c for L, _, c in stats if L == 0) > BASE["m0"]
            assert max(c for L, _, c in stats if L >= 1) > BASE["m"]


# ---------------------------------------------------------------- the planning header
@pytest.fixture(scope="module")
def plan():
    exe = os.path.join(ROOT, "islands_amd", "lib", "hnsw_remove_plan_dump")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "hnsw_remove_plan_dump.cpp"),
                           "-o", exe])

    def run(entry, max_level, levels, ids):
        text = (f"{len(levels)} {0 if entry is None else 1} {entry or 0} {max_level} {len(ids)}\n"
                + " ".join(str(int(x)) for x in levels) + "\n" + " ".join(str(int(x)) for x in ids) + "\n")
        out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60, check=True).stdout
        return [ln.split() for ln in out.splitlines()]

    return run


def test_plan_header(plan):
    rng = np.random.default_rng(2)
    for n0, count in ((1, 1), (12, 3), (12, 12), (300, 1), (300, 170), (300, 290)):
        lv = rng.integers(0, 5, n0).tolist()
        ids = rng.choice(n0, count, replace=False).tolist()
        ids += ids[:2]  # repeated ids count once
        entry, top = int(np.argmax(lv)), max(lv)
        lines = plan(entry, top, lv, ids)
        remap, keep = rref.remap_of(n0, set(ids))
        want_entry, want_top = rref.entry_after(lv, keep, remap, entry, top)
        got = {ln[0]: [int(x) for x in ln[1:]] for ln in lines if ln[0] in ("len", "entry", "layers", "members", "capacity")}
        assert got["len"] == [len(keep)]
        assert got["entry"] == [0 if want_entry is None else 1, want_entry or 0, want_top]
        assert got["layers"] == [top + 1, want_top + 1 if keep else 1]
        members = [sum(1 for i in keep if lv[i] >= L) for L in range(top + 1)]
        assert got["members"] == members and got["capacity"] == [sum(members)]
    rows = plan(0, 0, [0], [0])
    pairs = [[int(x) for x in ln[1:]] for ln in rows if ln[0] == "pair"]
    assert len(pairs) == 12 and len({p[2] for p in pairs}) == 12  # no two pairs share a code
    for layer, node, packed, layer_back, node_back in pairs:
        assert (layer_back, node_back) == (layer, node) and packed == (layer << 32) | node
    assert [ln[1:] for ln in rows if ln[0] == "cap"] == [["0", "4", "8", "8"], ["1", "4", "8", "4"], ["9", "4", "8", "4"]]
    assert ["max_layers", "64"] in rows
    # LDS of the one repair launch: tile + query + four lists of 512 + a row of the larger of m0 and m
    tile = 16 * 80 * 4
    lds = [[int(x) for x in ln[1:]] for ln in rows if ln[0] == "lds"]
    assert len(lds) == 18
    for d, m, m0, got in lds:
        assert got == tile + ((d + 3) // 4 * 4 + 16) * 4 + 512 * 16 + max(m, m0) * 4
        assert got < 64 * 1024


@pytest.mark.timeout(900)
def test_host_paths_under_address_sanitizer():
    csrc = os.path.join(ROOT, "islands_amd", "csrc")
    exe = os.path.join(ROOT, "islands_amd", "lib", "asan", "hnsw_remove_host")
    subprocess.check_call(["make", "-C", csrc, exe.replace(os.path.join(ROOT, "islands_amd"), ".."), "-j", "4", "-s"])
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1:halt_on_error=1")
    pr = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = pr.stdout.decode(errors="replace")
    assert pr.returncode == 0 and "hnsw remove host: ok" in out and "AddressSanitizer" not in out, out[-3000:]
