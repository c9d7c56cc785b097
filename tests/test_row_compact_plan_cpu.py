"""The in-place row compaction of a reserved index without a device: the plan of islands_amd/csrc/row_compact_plan.hpp
through tests/cpp/row_compact_plan_dump.cpp (g++ alone, and once more as a stand-alone program under
-fsanitize=address,undefined), replayed on a numpy array with a move's semantics, the capacity arithmetic of
row_table_plan.hpp against a Python restatement, and the row table's capacity and view over fake allocators in a
stand-alone program under AddressSanitizer (tests/cpp/row_capacity_host.cpp)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "row_compact_plan_dump.cpp")
N = 300
STAGES = (1, 7, 64, 300)


def removals(n=N):
    """the id sets the GPU test removes too (tests/test_gpu_index_reserve.py)"""
    return {
        "first": [0],
        "last": [n - 1],
        "middle": [n // 2],
        "every_other": list(range(0, n, 2)),
        "block": list(range(100, 200)),
        "all_but_last": list(range(n - 1)),
        "all": list(range(n)),
        "none": [],
    }


def build(flags, name):
    exe = os.path.join(ROOT, "islands_amd", "lib", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", *flags, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def exes():
    return (build(["-O1"], "row_compact_plan_dump"),
            build(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                  "row_compact_plan_dump_san"))


def dump(exe, survivors, stage):
    text = f"{len(survivors)} {stage}\n" + " ".join(str(int(x)) for x in survivors) + "\n"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1")
    pr = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60, env=env)
    assert pr.returncode == 0 and "Sanitizer" not in pr.stderr and "runtime error" not in pr.stderr, pr.stderr[-2000:]
    return [ln.split() for ln in pr.stdout.splitlines()]


def replay(lines, survivors, n0, stage):
    """runs the moves on rows 0 .. n0-1 of a [n0, 2] array (a row and its norm) and checks every rule of the plan"""
    s = np.asarray(survivors, np.int64)
    n = len(s)
    rows = np.stack([np.arange(n0, dtype=np.int64) * 7 + 1, np.arange(n0, dtype=np.int64) + 1000], 1)
    want = rows[s].copy()
    first = int([ln for ln in lines if ln[0] == "first"][0][1])
    gone = sorted(set(range(n0)) - set(s.tolist()))
    assert first == (min(gone[0], n) if gone else n)
    written = np.zeros(n0, bool)
    at = first
    launches = 0
    for ln in (ln for ln in lines if ln[0] == "move"):
        j, count, staged = int(ln[1]), int(ln[2]), int(ln[3])
        assert j == at and count >= 1 and j + count <= n  # ascending new ids, no gap, no overlap
        src, dst = s[j:j + count], np.arange(j, j + count)
        assert (src >= dst).all()
        assert not written[src].any()  # no source of a move was the destination of an earlier one
        if staged:
            assert count <= stage
            stage_buf = rows[src].copy()  # every source is read ...
            rows[dst] = stage_buf         # ... before any destination is written
            launches += 2
        else:
            assert int(src[0]) >= j + count and not set(src.tolist()) & set(dst.tolist())
            for a, b in zip(dst.tolist(), src.tolist()):  # any order: the sets are disjoint
                rows[a] = rows[b]
            launches += 1
        written[dst] = True
        at = j + count
    assert at == n
    assert (rows[:n] == want).all()
    assert not written[:first].any() and (rows[:first, 0] == np.arange(first) * 7 + 1).all()
    # every move but the last takes at least `stage` rows: a small gap near the start of the table does not cost a
    # launch per row
    assert launches <= 2 * (-(-max(n - first, 0) // stage))
    return launches


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("name", list(removals()))
def test_plan_replayed(exes, name, stage):
    gone = set(removals()[name])
    survivors = [i for i in range(N) if i not in gone]
    out = [dump(exe, survivors, stage) for exe in exes]
    assert out[0] == out[1]
    replay(out[0], survivors, N, stage)
    if name in ("none", "last", "all"):
        assert not [ln for ln in out[0] if ln[0] == "move"]  # nothing moves


def test_plan_random_subsets(exes):
    rng = np.random.default_rng(7)
    for i in range(200):
        n0 = int(rng.integers(1, N + 1))
        keep = rng.random(n0) < rng.random()
        survivors = np.nonzero(keep)[0].tolist()
        stage = int(rng.choice([1, 2, 7, 64, 300]))
        replay(dump(exes[i % 2], survivors, stage), survivors, n0, stage)


def test_one_removed_id_in_a_large_table_is_few_launches(exes):
    n0, stage = 20000, 4096
    survivors = [i for i in range(n0) if i != 5]
    assert replay(dump(exes[0], survivors, stage), survivors, n0, stage) == 2 * 5  # ceil(19994 / 4096) staged moves


def restated_stage_rows(row_bytes, n, env):
    rows = max(1, (64 << 20) // max(1, row_bytes))
    if env not in ("-", "empty") and int(env) > 0:
        rows = int(env)
    return max(1, min(rows, max(1, n)))


def test_stage_rows_and_capacity_arithmetic(exes):
    lines = dump(exes[1], [0, 1, 2], 1)
    es = {0: 4, 1: 2, 2: 1}
    stride = lambda dt, d: -(-d // (16 // es[dt])) * (16 // es[dt])
    slack = lambda dt: 1024 // es[dt]
    seen = set()
    for ln in lines:
        kind, a, got = ln[0], ln[1:-2], int(ln[-1])
        seen.add(kind)
        if kind == "stage":
            assert got == restated_stage_rows(int(a[0]), int(a[1]), a[2]), ln
        elif kind == "alloc":
            dt, d, cap = map(int, a)
            assert got == cap * stride(dt, d) + slack(dt), ln
        elif kind == "tail":
            dt, d, cap, first = map(int, a)
            assert got == (cap - first) * stride(dt, d) + slack(dt), ln
            assert first * stride(dt, d) + got == cap * stride(dt, d) + slack(dt)  # it ends where the block ends
        elif kind == "fill":
            dt, cap, first, count = map(int, a)
            assert got == (slack(dt) if first + count == cap else 0), ln
        elif kind == "vacated":
            dt, d, n, n0 = map(int, a)
            assert got == (n0 - n) * stride(dt, d), ln
    assert seen >= {"stage", "alloc", "tail", "fill", "vacated"}
    # the figures the issue names: bf16 rows of d = 100 sit 104 apart, f32 rows of d = 3 are guarded to 4
    assert ["alloc", "1", "100", "512", "->", str(512 * 104 + 512)] in lines
    assert ["alloc", "0", "3", "512", "->", str(512 * 4 + 256)] in lines
    assert ["alloc", "2", "768", "512", "->", str(512 * 768 + 1024)] in lines


@pytest.mark.timeout(600)
def test_capacity_and_view_under_address_sanitizer():
    csrc = os.path.join(ROOT, "islands_amd", "csrc")
    exe = os.path.join(ROOT, "islands_amd", "lib", "asan", "row_capacity_host")
    subprocess.check_call(["make", "-C", csrc, "../lib/asan/row_capacity_host", "-s"])
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1:halt_on_error=1")
    pr = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = pr.stdout.decode(errors="replace")
    assert pr.returncode == 0 and "row capacity host: ok" in out and "Sanitizer" not in out, out[-3000:]
