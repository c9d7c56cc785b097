"""What one enqueue launches (islands_amd/csrc/search_launch_plan.hpp: the kernels of a search call in stream order,
each with its grid, LDS, instantiation and the nq it is told) over a grid of calls.  No device is needed: the driver
(tests/cpp/launch_plan_dump.cpp) is host-only and built by `make -C islands_amd/csrc launch_plan`.

Two checks.  The named cases below were written by hand from search_enqueue_impl as it stood when the launches were
still issued between its nested conditions (they do not come from running the plan): the step kinds in order, each with
its grid, the geometry figure its LDS comes from and the nq the kernel is told, as literals.  Then the whole output is
compared with tests/golden/search_launch_plan.txt, recorded from the plan: a change of any line is a change of what
runs on the card and has to be meant -- re-record the fixture with it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# selectors of a step, in the order the driver prints them
SEL = ("S", "wide", "dtype", "resume", "qh", "bf16", "hnsw", "metric")


def step(kind, grid, lds, nq, **sel):
    """lds: the name of the geometry figure on the case's header line (fg, fgq, tl, tlq, exact, descent) or 0"""
    return (kind, grid, lds, nq, sel)


# d = 100, k = 10, 256 compute units, 32 slots of the heap-exact kernel's pool; nq = 70 unless the case says otherwise
EXACT70 = step("Exact", 32, "exact", 70)
EXPECTED = {
    "plain f32 deg=64 ef=128 nq=70": [step("Fast", 70, "fg", 70, S=2, wide=0, dtype=0, resume=0, qh=0), EXACT70],
    "plain f32 deg=64 ef=10 nq=1": [step("Fast", 1, "fg", 1, S=1), step("Exact", 1, "exact", 1)],
    # bf16 rows of up to 64 ids: classify, the bf16-query kernel, the float32-query kernel over the others
    "plain bf16 deg=64 ef=128 nq=70": [step("Classify", 70, 0, 70), step("Fast", 70, "fgq", 70, qh=1, dtype=1, qsel_mode=0),
                                       step("Fast", 70, "fg", 70, qh=0, dtype=1, qsel_mode=1), EXACT70],
    "plain bf16 deg=64 ef=128 nq=5000": [step("Classify", 2048, 0, 5000), step("Fast", 4096, "fgq", 5000, qh=1),
                                         step("Fast", 4096, "fg", 5000, qsel_mode=1), step("Exact", 32, "exact", 5000)],
    "plain bf16 deg=65 ef=128 nq=70": [step("Fast", 70, "fg", 70, wide=1, qh=0, dtype=1), EXACT70],
    "plain bf16 deg=128 ef=512 nq=70": [step("Fast", 70, "fg", 70, wide=1, qh=0, S=8), EXACT70],
    "plain fp8 deg=64 ef=128 nq=70": [step("Fast", 70, "fg", 70, dtype=2, qh=0, wide=0), EXACT70],
    # no fast kernel: the host queues every query for the heap-exact kernel
    "plain f32 deg=64 ef=513 nq=70": [step("FillRedoAll", 0, 0, 70), EXACT70],
    "plain f32 deg=129 ef=128 nq=70": [step("FillRedoAll", 0, 0, 70), EXACT70],
    "plain bf16 deg=129 ef=128 nq=70": [step("FillRedoAll", 0, 0, 70), EXACT70],
    "hnsw2 f32 deg=64 ef=128 nq=70": [step("Descent", 70, "descent", 70, bf16=0), step("Fast", 70, "fg", 70),
                                      step("Exact", 32, "exact", 70, hnsw=1)],
    "hnsw2 bf16 deg=64 ef=128 nq=5000": [step("Descent", 5000, "descent", 5000, bf16=1), step("Classify", 2048, 0, 5000),
                                         step("Fast", 4096, "fgq", 5000, qh=1), step("Fast", 4096, "fg", 5000, qsel_mode=1),
                                         step("Exact", 32, "exact", 5000, hnsw=1)],
    "hnsw0 f32 deg=64 ef=128 nq=70": [step("Fast", 70, "fg", 70), step("Exact", 32, "exact", 70, hnsw=1)],
    "seeds f32 deg=64 ef=128 nq=70": [step("EntryPick", 0, 0, 70), step("Fast", 70, "fg", 70), EXACT70],
    # the construction search of an HnswGraph with two upper layers: no descent, never seeded
    "build f32 deg=64 ef=128 nq=70": [step("Fast", 70, "fg", 70), step("Exact", 32, "exact", 70, hnsw=1)],
    "build+seeds f32 deg=64 ef=128 nq=70": [step("Fast", 70, "fg", 70), EXACT70],
    "tl f32 deg=64 ef=128 nq=70": [step("PqTables", 0, 0, 70), step("TwoLevel", 70, "tl", 70, bf16=0, resume=0, qh=0)],
    "tl+seeds f32 deg=64 ef=128 nq=70": [step("PqTables", 0, 0, 70), step("TwoLevel", 70, "tl", 70)],
    "tl bf16 deg=64 ef=128 nq=70": [step("PqTables", 0, 0, 70), step("Classify", 70, 0, 70),
                                    step("TwoLevel", 70, "tlq", 70, bf16=1, resume=0, qh=1, qsel_mode=0),
                                    step("TwoLevel", 70, "tl", 70, bf16=1, resume=0, qh=0, qsel_mode=1)],
    # a retry: 35 listed queries alone, the tables of the first launch kept
    "tl-retry4 f32 deg=64 ef=128 nq=70": [step("TwoLevel", 35, "tl", 35, resume=0)],
    "tl-retry4 bf16 deg=64 ef=128 nq=70": [step("TwoLevel", 35, "tl", 35, bf16=1, qh=0, qsel_mode=0)],
    # rounds of the recompute provider: the traversal kernel is told the round's queries, the exact kernel the call's
    "rec-first f32 deg=64 ef=128 nq=70": [step("Fast", 70, "fg", 70, resume=1), EXACT70],
    "rec-listed f32 deg=64 ef=128 nq=70": [step("SeedRedo", 1, 0, 3), step("Fast", 35, "fg", 35, resume=1), EXACT70],
    "rec-exact-only f32 deg=64 ef=128 nq=70": [step("SeedRedo", 1, 0, 5), EXACT70],
    "rec-listed f32 deg=64 ef=513 nq=70": [step("SeedRedo", 1, 0, 3), EXACT70],
    "rec-rerun f32 deg=64 ef=513 nq=70": [step("FillRedoAll", 0, 0, 70), EXACT70],
    "rec-tl-first f32 deg=64 ef=128 nq=70": [step("PqTables", 0, 0, 70), step("TwoLevel", 70, "tl", 70, resume=1)],
    "rec-tl-resume f32 deg=64 ef=128 nq=70": [step("TwoLevel", 35, "tl", 35, resume=1, qh=0)],
    # warm launches: one workgroup, nq = 0, no tables, no host-filled queue; the qh pair, the descent and the exact
    # kernel still run
    "warm-plain f32 deg=64 ef=128 nq=0": [step("Fast", 1, "fg", 0, resume=0), step("Exact", 1, "exact", 0)],
    "warm-plain f32 deg=64 ef=513 nq=0": [step("Exact", 1, "exact", 0)],
    "warm-plain bf16 deg=64 ef=128 nq=0": [step("Classify", 1, 0, 0), step("Fast", 1, "fgq", 0, qh=1),
                                           step("Fast", 1, "fg", 0, qsel_mode=1), step("Exact", 1, "exact", 0)],
    "warm-seeds f32 deg=64 ef=128 nq=0": [step("Fast", 1, "fg", 0), step("Exact", 1, "exact", 0)],
    "warm-hnsw2 f32 deg=64 ef=128 nq=0": [step("Descent", 1, "descent", 0), step("Fast", 1, "fg", 0),
                                          step("Exact", 1, "exact", 0, hnsw=1)],
    "warm-tl f32 deg=64 ef=128 nq=0": [step("TwoLevel", 1, "tl", 0, resume=0)],
    "warm-tl bf16 deg=64 ef=128 nq=0": [step("TwoLevel", 1, "tl", 0, bf16=1, resume=0, qh=0)],
    # the two-level warm launch on a recompute index: the RESUME instantiation, which its rounds run
    "warm-rec-tl f32 deg=64 ef=128 nq=0": [step("TwoLevel", 1, "tl", 0, resume=1)],
    "warm-rec f32 deg=64 ef=128 nq=0": [step("Fast", 1, "fg", 0, resume=0), step("Exact", 1, "exact", 0)],
}

# call-level facts of some of those cases: flags that must be set / must not be, figures
EXPECTED_PLAN = {
    "plain f32 deg=64 ef=128 nq=70": ({"use_fast", "prepare_lane", "wants_ell", "measures", "publishes"},
                                      {"lane_slots": 70, "nq": 70, "q_entry_words": 0, "qlist": 0}),
    "plain bf16 deg=64 ef=128 nq=70": ({"use_fast", "prepare_lane", "wants_ell", "measures", "qsel", "publishes"}, {}),
    "plain f32 deg=129 ef=128 nq=70": ({"prepare_lane", "measures", "publishes"}, {}),
    "seeds f32 deg=64 ef=128 nq=70": ({"use_fast", "seeded", "prepare_lane", "wants_ell", "measures", "entry_given",
                                       "publishes"}, {"q_entry_words": 280, "max_level": 0}),
    "hnsw2 f32 deg=64 ef=128 nq=70": ({"use_fast", "prepare_lane", "wants_ell", "measures", "publishes"},
                                      {"q_entry_words": 140, "max_level": 2}),
    "build f32 deg=64 ef=128 nq=70": ({"use_fast", "prepare_lane", "wants_ell", "measures", "construction", "entry_given",
                                       "publishes"}, {"q_entry_words": 0, "max_level": 0}),
    "tl f32 deg=64 ef=128 nq=70": ({"two_level", "prepare_lane", "wants_ell", "measures", "publishes"}, {"qlist": 0}),
    "tl f32 deg=129 ef=128 nq=70": ({"two_level", "prepare_lane", "measures", "publishes"}, {}),
    "tl-retry4 f32 deg=64 ef=128 nq=70": ({"two_level", "prepare_lane", "wants_ell", "measures", "publishes"},
                                          {"qlist": 2, "nq": 70}),
    "rec-first f32 deg=64 ef=128 nq=5000": ({"use_fast", "resume", "prepare_lane", "wants_ell", "measures", "publishes"},
                                            {"lane_slots": 5000, "qlist": 0}),
    "rec-listed f32 deg=64 ef=128 nq=70": ({"use_fast", "resume", "prepare_lane", "wants_ell", "measures",
                                            "exact_park_fields", "publishes"}, {"qlist": 1}),
    "rec-rerun f32 deg=64 ef=128 nq=70": ({"use_fast", "prepare_lane", "wants_ell", "measures", "publishes"},
                                          {"q_entry_words": 0}),
    "rec-tl-resume f32 deg=64 ef=128 nq=70": ({"two_level", "resume", "prepare_lane", "wants_ell", "measures", "publishes"},
                                              {"qlist": 1, "tl_prefetch": 4}),
    "rec-tl-first f32 deg=64 ef=128 nq=70": ({"two_level", "resume", "prepare_lane", "wants_ell", "measures", "publishes"},
                                             {"qlist": 0, "tl_prefetch": 4}),
    "warm-plain f32 deg=64 ef=128 nq=0": ({"use_fast", "wants_ell"}, {"nq": 0, "q_entry_words": 0}),
    "warm-build f32 deg=64 ef=128 nq=0": ({"use_fast", "wants_ell"}, {"max_level": 2, "q_entry_words": 2}),
    "warm-hnsw2 f32 deg=64 ef=128 nq=0": ({"use_fast", "wants_ell"}, {"max_level": 2, "q_entry_words": 2}),
}


def parse(lines):
    cases, cur = {}, None
    for ln in lines:
        if ln.startswith("case "):  # case <name> | lds <figures> | plan steps=N flags=a,b, <figures>; zero figures are left out
            assert " -> status " not in ln, ln  # (no call of the grid is refused by its geometry)
            head, lds, plan = ln[5:].split(" | ")
            kv = dict(x.split("=") for x in plan.split()[1:])
            cur = cases[head] = {"geom": dict(x.split("=") for x in lds.split()[1:]), "steps": [],
                                 "flags": {x for x in kv.pop("flags").split(",") if x}}
            cur["figs"] = {k: int(v) for k, v in kv.items()}
        else:
            f = ln.split()
            assert f[0] == "step", ln
            kv = dict(x.split("=") for x in f[2:])
            sel = dict(zip(SEL, (int(x) for x in kv.pop("sel").split(","))))
            cur["steps"].append((f[1], {k: int(v) for k, v in kv.items()}, sel))
    return cases


@pytest.mark.timeout(600)
def test_search_launch_plan():
    csrc = os.path.join(ROOT, "islands_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "launch_plan", "-s"])
    exe = os.path.join(ROOT, "islands_amd", "lib", "launch_plan_dump")
    # the experiment switches (ISL_HBITS, ISL_HCAP, ...) change the geometry on purpose
    env = {k: v for k, v in os.environ.items() if not k.startswith("ISL_")}
    pr = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert pr.returncode == 0, pr.stderr.decode(errors="replace")[-2000:]
    got = pr.stdout.decode().splitlines()
    cases = parse(got)

    for name, want in EXPECTED.items():
        c = cases[name]
        assert [s[0] for s in c["steps"]] == [w[0] for w in want], (name, c["steps"])
        assert c["figs"]["steps"] == len(want), name
        for (kind, vals, sel), (_, grid, lds, nq, want_sel) in zip(c["steps"], want):
            assert vals["grid"] == grid, (name, kind, vals)
            assert vals["lds"] == (int(c["geom"][lds]) if lds else 0), (name, kind, vals, lds)
            assert vals["nq"] == nq, (name, kind, vals)
            for k, v in want_sel.items():
                assert (vals[k] if k == "qsel_mode" else sel[k]) == v, (name, kind, k, vals, sel)
    for name, (flags, figs) in EXPECTED_PLAN.items():
        c = cases[name]
        assert c["flags"] == flags, (name, c["flags"])
        for k, v in figs.items():
            assert c["figs"].get(k, 0) == v, (name, k, c["figs"])

    with open(os.path.join(ROOT, "tests", "golden", "search_launch_plan.txt")) as f:
        want = f.read().splitlines()
    assert len(want) > 300
    diff = [(i + 1, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not diff, f"{len(diff)} lines differ, first: line {diff[0][0]}\n  recorded {diff[0][1]}\n  now      {diff[0][2]}"
    assert len(got) == len(want)
