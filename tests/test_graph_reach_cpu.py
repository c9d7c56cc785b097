"""Graph reachability without a GPU: the three ABI symbols, their declarations and the report's size, every error
that is answered before a device call, the host arithmetic of islands_amd/csrc/graph_reach_plan.hpp through
tests/cpp/graph_reach_plan_dump.cpp (g++ alone, and once more as a stand-alone program under
-fsanitize=address,undefined) against a Python restatement, and tests/_reach_ref.py against answers worked out by
hand on the hand graphs tests/test_gpu_graph_reach.py runs on the device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import islands_amd as ia
from islands_amd import _ffi

import _reach_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "graph_reach_plan_dump.cpp")
DECLARED = {
    "isl_index_reachability": "const isl_index* idx, const uint64_t* sources, uint64_t n_sources, uint32_t* out_depth, "
                              "uint32_t* out_in_degree, int32_t mem, isl_reach_report* report",
    "isl_hnsw_reachability": "const isl_hnsw* h, uint64_t layer, const uint64_t* sources, uint64_t n_sources, "
                             "uint32_t* out_depth, uint32_t* out_in_degree, int32_t mem, isl_reach_report* report",
    "isl_index_cover_entry_seeds": "isl_index* idx, uint64_t max_seeds, uint64_t* out_ids, uint64_t* out_count, "
                                   "uint64_t* out_unreached",
}
INVALID, UNSUPPORTED, NODE_NOT_FOUND = 101, 102, 5  # isl_status
NONE = 0xFFFFFFFF


# ------------------------------------------------------------------ the ABI
def test_symbols_declarations_and_struct_size():
    lib = _ffi.lib()
    hdr = open(os.path.join(ROOT, "include", "islands_amd.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    for name, args in DECLARED.items():
        assert hasattr(lib, name), name
        assert f"isl_status {name}({args});" in flat, name
        res, argtypes = _ffi.SIGNATURES[name]
        assert res is _ffi.i32 and len(argtypes) == args.count(",") + 1, name
    assert re.search(r"#define ISL_DEPTH_UNREACHED 0xFFFFFFFFu\b", hdr)
    assert re.search(r"#define ISL_DEPTH_ABSENT 0xFFFFFFFEu\b", hdr)
    assert (ia.DEPTH_UNREACHED, ia.DEPTH_ABSENT) == (rr.UNREACHED, rr.ABSENT) == (0xFFFFFFFF, 0xFFFFFFFE)
    fields = re.search(r"typedef struct isl_reach_report \{(.*?)\} isl_reach_report;", flat).group(1)
    names = [f.strip() for f in fields.replace("uint64_t", "").strip(" ;").split(",")]
    assert tuple(names) == rr.REPORT_FIELDS == tuple(n for n, _ in _ffi.ReachReportC._fields_)
    assert C.sizeof(_ffi.ReachReportC) == 64 and "64 bytes" in hdr
    assert lib.isl_abi_version() == 3
    assert callable(ia.LeannIndex.reachability) and callable(ia.LeannIndex.cover_entry_seeds)
    assert callable(ia.HnswGraph.reachability)
    for text in (open(os.path.join(ROOT, "include", "islands_amd.hpp")).read(),
                 open(os.path.join(ROOT, "INTEGRATION.md")).read()):
        for name in DECLARED:
            assert name in text, name
    # the guarantee is stated for what it is
    assert "reachable from SOME seed" in hdr and "PICKED" in hdr


def host_ring(n=5, entry=2):
    g = ia.CsrGraph()
    for i in range(n):
        g.add_node([(i + 1) % n], 0)
    g.entry_point = entry
    return ia.LeannIndex.from_csr(g, dimension=4)


def test_errors_answered_before_a_device_call():
    lib = _ffi.lib()
    rep = _ffi.ReachReportC()
    n, un = C.c_uint64(7), C.c_uint64(7)
    src = np.array([1], np.uint64)
    assert lib.isl_index_reachability(None, None, 0, None, None, 0, C.byref(rep)) == INVALID
    assert lib.isl_hnsw_reachability(None, 0, None, 0, None, None, 0, C.byref(rep)) == INVALID
    assert lib.isl_index_cover_entry_seeds(None, 4, None, C.byref(n), C.byref(un)) == INVALID
    assert (n.value, un.value) == (0, 0)
    host = host_ring()
    before = host.to_bytes()
    assert lib.isl_index_reachability(host._h, src.ctypes.data, 1, None, None, 7, C.byref(rep)) == INVALID  # mem
    assert lib.isl_index_reachability(host._h, None, 3, None, None, 0, C.byref(rep)) == INVALID  # NULL list of 3

    def kind(call):
        with pytest.raises(ia.CoreError) as e:
            call()
        return e.value

    empty = ia.LeannIndex.with_defaults()
    assert kind(lambda: empty.reachability()).kind == "EmptyCollection"
    assert kind(lambda: empty.reachability(sources=[0])).kind == "EmptyCollection"  # before the source check
    assert kind(lambda: empty.cover_entry_seeds()).kind == "EmptyCollection"
    assert kind(lambda: empty.cover_entry_seeds(65537)).kind == "Unsupported"       # the cap comes first
    assert kind(lambda: host.cover_entry_seeds(65537)).kind == "Unsupported"
    # a source that names no node: before the residency check, with the id
    e = kind(lambda: host.reachability(sources=[1, 1, 9, 2]))
    assert e.kind == "NodeNotFound" and e.node == 9
    # no entry point and no sources
    g = ia.CsrGraph()
    g.add_node([1], 0)
    g.add_node([0], 0)
    g.entry_point = None
    noentry = ia.LeannIndex.from_csr(g, dimension=4)
    assert kind(lambda: noentry.reachability()).kind == "IndexNotBuilt"
    # a graph that is not on a device: the status of the neighbouring device-only calls
    assert kind(lambda: noentry.reachability(sources=[1])).kind == "Unsupported"
    assert kind(lambda: host.reachability()).kind == "Unsupported"
    assert kind(lambda: host.select_entry_seeds(2)).kind == kind(lambda: host.cover_entry_seeds()).kind == "Unsupported"
    assert host.to_bytes() == before and host.entry_seeds().size == 0
    with pytest.raises(ValueError):
        host.reachability(sources=[])


# ------------------------------------------------------------------ the plan header
def build(flags, name):
    exe = os.path.join(ROOT, "islands_amd", "lib", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", *flags, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def exes():
    return (build(["-O1"], "graph_reach_plan_dump"),
            build(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                  "graph_reach_plan_dump_san"))


def dump(exe, length, layer, levels, sources, table, entry, max_seeds, cover_len, reached0, steps):
    nums = [length, layer, len(levels), *levels, len(sources), *sources, len(table), *table, entry, max_seeds,
            cover_len, len(steps), reached0]
    for found, after in steps:
        nums += [found, after]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1")
    pr = subprocess.run([exe], input=" ".join(str(int(v)) for v in nums) + "\n", capture_output=True, text=True,
                        timeout=60, env=env)
    assert pr.returncode == 0 and "Sanitizer" not in pr.stderr and "runtime error" not in pr.stderr, pr.stderr[-2000:]
    return [ln.split() for ln in pr.stdout.splitlines()]


def restated_sources(length, layer, levels, sources):
    for s in sources:
        if s >= length or (levels[s] if s < len(levels) else 0) < layer:
            return [NODE_NOT_FOUND, s, 0]
    return [0, 0, len(set(sources)), *sources]


def restated_blocks(kind, elements, cus):
    per = 4 if kind == "expand" else 256
    return max(1, min(-(-elements // per), max(cus, 1) * 8))


def restated_cover(table, entry, max_seeds, length, reached, steps, window=1 << 20):
    seeds = list(table) or [entry]
    initial, cursor, scans = len(seeds), 0, 0
    wants = lambda: reached < length and len(seeds) < max_seeds
    out = [["cover", "start", initial, "wants", int(wants())]]
    for found, after in steps:
        if not wants():
            break
        count = min(window, length - cursor) if cursor < length else 0
        out.append(["window", cursor, count])
        if not count:
            break
        scans += 1
        took = found != NONE and cursor <= found < cursor + count
        if took:
            seeds.append(found)
            cursor = found + 1
            reached = after
        else:
            cursor += count
        out.append(["take", int(took), "cursor", cursor, "seeds", len(seeds), "wants", int(wants())])
    out.append(["cover", "end", "added", len(seeds) - initial, "installs", int(len(seeds) > initial), "unreached",
                length - reached, "scans", scans, "seeds", *seeds])
    return [[str(v) for v in ln] for ln in out]


COVER_CASES = {
    # name: (table, entry, max_seeds, len, reached after S, [(scan answer, reached after its walk)])
    "nothing_to_add": ([], 3, 16, 70, 70, [(NONE, 70)]),
    "three_islands": ([], 0, 16, 30, 10, [(10, 20), (20, 30), (NONE, 30)]),
    "capped": ([], 0, 2, 30, 10, [(10, 20), (20, 30)]),
    "table_is_the_prefix": ([7, 3, 7], 0, 16, 30, 12, [(0, 25), (26, 30)]),
    "table_above_the_cap": ([1, 2, 3], 0, 2, 30, 12, [(0, 25)]),
    "no_seeds_allowed": ([], 0, 0, 30, 10, [(10, 20)]),
    "windows": ([], 0, 16, (1 << 21) + 5, 5, [(NONE, 0), (NONE, 0), ((1 << 21) + 2, (1 << 21) + 5)]),
    "answer_outside_the_window": ([], 0, 16, (1 << 20) + 9, 5, [((1 << 20) + 3, 9), ((1 << 20) + 3, (1 << 20) + 9)]),
    "script_runs_out": ([], 0, 16, 30, 10, [(10, 20)]),
}


@pytest.mark.parametrize("name", list(COVER_CASES))
def test_cover_loop_against_its_restatement(exes, name):
    table, entry, max_seeds, length, reached, steps = COVER_CASES[name]
    out = [dump(exe, 4, 0, [], [0], table, entry, max_seeds, length, reached, steps) for exe in exes]
    assert out[0] == out[1]
    got = [ln for ln in out[0] if ln[0] in ("cover", "window", "take")]
    assert got == restated_cover(table, entry, max_seeds, length, reached, steps), name
    end = got[-1]
    if name == "nothing_to_add":
        assert end[3] == "0" and end[5] == "0" and end[7] == "0"  # nothing added, nothing installed, none unreached
    if name == "capped":
        assert end[3] == "1" and end[7] == "10" and end[11:] == ["0", "10"]
    if name == "table_is_the_prefix":
        assert end[11:] == ["7", "3", "7", "0", "26"] and end[7] == "0"


def test_sources_and_geometry_against_their_restatement(exes):
    levels = [0, 2, 1, 0, 3, 1, 0, 0]
    cases = [(8, 0, [], [3]), (8, 0, [], [3, 3, 7, 0, 3]), (8, 0, [], [3, 8]), (8, 0, levels, [1, 4, 6]),
             (8, 1, levels, [1, 4, 2, 1]), (8, 1, levels, [1, 0]), (8, 2, levels, [4, 1, 5]), (8, 3, levels, [4]),
             (8, 1, levels[:3], [1, 2]), (8, 1, levels[:3], [1, 4]), (1 << 40, 0, [], [(1 << 40) - 1, 1 << 40])]
    for i, (length, layer, lv, src) in enumerate(cases):
        lines = dump(exes[i % 2], length, layer, lv, src, [], 0, 4, 8, 8, [])
        want = restated_sources(length, layer, lv, src)
        if length > (1 << 32) and want[0] == 0:
            continue
        assert lines[0] == ["sources"] + [str(v) for v in want], (i, lines[0])
    geo = [ln for ln in lines if ln[0] in ("expand", "stream")]
    assert len(geo) == 2 * 4 * 10
    for kind, elements, cus, _, got in geo:
        assert int(got) == restated_blocks(kind, int(elements), int(cus)), (kind, elements, cus, got)
        assert 1 <= int(got) <= max(int(cus), 1) * 8
    assert dump(exes[1], 8, 0, [], [9], [], 0, 4, 8, 8, [])[0][:3] == ["sources", "5", "9"]


# ------------------------------------------------------------------ the definitions, by hand
def test_reference_on_one_node_and_a_ring():
    depth, indeg, rep = rr.reach([[]], [0])
    assert depth.tolist() == [0] and indeg.tolist() == [0]
    assert rep == dict(nodes=1, sources=1, reached=1, levels=1, edges=0, dangling_edges=0, no_inbound=1, max_in_degree=0)
    ring = [[(i + 1) % 70] for i in range(70)]
    depth, indeg, rep = rr.reach(ring, [5])
    assert depth.tolist() == [(i - 5) % 70 for i in range(70)] and indeg.tolist() == [1] * 70
    assert rep == dict(nodes=70, sources=1, reached=70, levels=70, edges=70, dangling_edges=0, no_inbound=0,
                       max_in_degree=1)
    assert rr.cover(ring, [5], 16) == ([5], 0, 0)


def test_reference_on_dangling_edges_self_loops_and_repeats():
    # 0 -> 1 -> {2, 9 (no such node)} -> 3; 3 lists itself; 4 is apart and lists 0 twice (one edge: distinct ids)
    lists = [[1], [2, 9], [3], [3], rr.distinct([0, 0])]
    depth, indeg, rep = rr.reach(lists, [0, 0])
    assert depth.tolist() == [0, 1, 2, 3, rr.UNREACHED]
    assert indeg.tolist() == [1, 1, 1, 2, 0]  # the self-loop counts, the repeat does not, the dangling id nowhere
    assert rep == dict(nodes=5, sources=1, reached=4, levels=4, edges=4, dangling_edges=1, no_inbound=1,
                       max_in_degree=2)
    assert rr.cover(lists, [0], 16) == ([0, 4], 1, 0)
    assert rr.cover(lists, [0], 1) == ([0], 0, 1)


def test_reference_on_two_rings_joined_downstream():
    # ring A = 0..3, ring B = 4..6, one edge A -> B (2 -> 4); entered in B, A stays unreached
    lists = [[1], [2], [3, 4], [0], [5], [6], [4]]
    depth, indeg, rep = rr.reach(lists, [5])
    assert depth.tolist() == [rr.UNREACHED] * 4 + [2, 0, 1]
    assert indeg.tolist() == [1, 1, 1, 1, 2, 1, 1]
    assert (rep["reached"], rep["levels"], rep["edges"], rep["no_inbound"]) == (3, 3, 3, 0)
    assert rr.cover(lists, [5], 16) == ([5, 0], 1, 0)   # the smallest unreached id, and from it everything
    assert rr.reach(lists, [0])[2]["reached"] == 7


def test_reference_on_a_layer_with_absent_nodes():
    # population {0, 2, 3}; 0 lists 1 (below the layer: dangling) and 2; 3 is not reached
    member = [True, False, True, True]
    depth, indeg, rep = rr.reach([[1, 2], [], [0], [2]], [0], member)
    assert depth.tolist() == [0, rr.ABSENT, 1, rr.UNREACHED] and indeg.tolist() == [1, 0, 2, 0]
    assert rep == dict(nodes=3, sources=1, reached=2, levels=2, edges=2, dangling_edges=1, no_inbound=1,
                       max_in_degree=2)


def test_reference_on_the_contended_graph():
    import test_gpu_graph_reach as g
    lists = g.contended_lists()
    depth, indeg, rep = rr.reach(lists, [0])
    assert len(lists) == 400 and sum(len(l) for l in lists[1:201]) == 30000
    assert (depth[1:201] == 1).all() and (depth[201:351] == 2).all() and (depth[351:] == rr.UNREACHED).all()
    assert rep["reached"] == 351 and rep["levels"] == 3 and rep["edges"] == 200 + 30000
    assert rep["max_in_degree"] == 200 and rep["no_inbound"] == 50  # node 0 and the 49 isolated ones
    # ... with a tail 350 -> 351 -> 352 hung off node 350: a node that entered the frontier twice would have its
    # list followed twice
    depth, indeg, rep = rr.reach(g.contended_lists(tail=True), [0])
    assert depth[351] == 3 and depth[352] == 4 and (depth[353:] == rr.UNREACHED).all()
    assert rep["reached"] == 353 and rep["levels"] == 5 and rep["edges"] == 200 + 30000 + 2
