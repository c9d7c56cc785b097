"""The recompute provider's round scheduler and caps (islands_amd/csrc/recompute_plan.hpp) without a device:
tests/cpp/recompute_plan_dump.cpp, built with g++ alone and a second time under AddressSanitizer and
UndefinedBehaviorSanitizer, is fed seeded scripts of per-round statuses; every round it prints is compared
with a Python restatement of the loop the scheduler was taken out of."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "recompute_plan_dump.cpp")

QS_OK, QS_NODE_NOT_FOUND, QS_SCRATCH, QS_BLOCKED, QS_BLOCKED_X = 0, 5, 0x101, 0x103, 0x104
RERUN, PARK, EXACT_QUEUE = 0, 1, 2
EF = 64


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def dump(request):
    if request.param == "plain":
        exe = os.path.join(ROOT, "islands_amd", "lib", "recompute_plan_dump")
        cmd = ["g++", "-std=c++17", "-O1", SRC, "-o", exe]
    else:  # the compiler of `make asan` (tests/test_asan_host.py), on the stand-alone driver
        exe = os.path.join(ROOT, "islands_amd", "lib", "asan", "recompute_plan_dump")
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++", "-std=c++17", "-O1", "-g",
               "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", SRC, "-o", exe]
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1:halt_on_error=1")

    def run(text):
        pr = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60, env=env)
        assert pr.returncode == 0 and "Sanitizer" not in pr.stderr and "runtime error" not in pr.stderr, \
            (pr.returncode, pr.stdout[-2000:], pr.stderr[-3000:])
        return pr.stdout.splitlines()

    return run


class Device:
    """What the kernels would report: query i blocks blocks[i] times before it ends as final[i]; a query
    that a round does not run keeps its status.  restart(ids) starts the named queries over."""

    def __init__(self, nq, kind, mixed, rng):
        self.rng, self.kind, self.mixed = rng, kind, mixed
        self.left = [int(x) for x in rng.integers(0, 4, nq)]
        self.final = [int(x) for x in rng.choice([QS_OK, QS_OK, QS_OK, QS_NODE_NOT_FOUND, QS_SCRATCH], nq)]
        self.status = [QS_OK] * nq

    def blocked(self):
        if self.kind == EXACT_QUEUE:  # parked in the heap-exact kernel
            return QS_BLOCKED_X
        if self.kind == PARK and self.mixed:  # a traversal kernel in front, some queries handed on to the parking exact kernel
            return int(self.rng.choice([QS_BLOCKED, QS_BLOCKED_X]))
        return QS_BLOCKED

    def run(self, ids):
        for i in ids:
            if self.left[i] > 0:
                self.left[i] -= 1
                self.status[i] = self.blocked()
            else:
                self.status[i] = self.final[i]

    def restart(self, ids):
        for i in ids:
            self.left[i] = int(self.rng.integers(0, 3))
            self.final[i] = QS_OK


def parent_rounds(nq, max_active, kind, tl, dev, short_sets):
    """The rounds of search_sync at commit 0243e31 (islands_amd/csrc/search.hip lines 903-1005: the first
    round's lists 906-921, the next round's lists 963-980, the two-level retry 981-995, the end 996-1004), with
    the device steps replaced by `dev`.  short_sets: what tl_collect_short names each time it is asked (the
    window_scale < 64 test is folded into it: an empty set ends the batch).
    Returns (rounds, script): rounds = [(listed, qlist, xlist, verdict)], script = the driver's stdin lines."""
    exact_only = kind in (RERUN, EXACT_QUEUE)
    resumable = kind != RERUN
    h_qlist, h_xlist = [0] * nq, [0] * nq
    active = min(nq, max_active)
    next_fresh = active
    nxl = 0
    listed = active < nq
    if not resumable:
        active, listed = 0, False
    elif exact_only:
        for i in range(active):
            h_xlist[i] = i
        nxl, active, listed = active, 0, True
    elif listed:
        for i in range(active):
            h_qlist[i] = i
    again = []
    rounds, script = [], []

    def snapshot(verdict):
        rounds.append((listed, h_qlist[:active] if listed else ("all", active), h_xlist[:nxl], verdict))

    snapshot("launch")
    short_sets = list(short_sets)
    while True:
        # search_enqueue + search_finish
        if not resumable:
            dev.run(range(nq))
        elif listed:
            dev.run(h_qlist[:active] + h_xlist[:nxl])
        else:
            dev.run(range(active))
        status = dev.status
        misses = sum(s in (QS_BLOCKED, QS_BLOCKED_X) for s in status)
        script.append(" ".join(str(s) for s in status[:nq if not resumable else next_fresh]))
        if resumable:
            na = 0
            nxl = 0
            for i in range(next_fresh):
                if status[i] == QS_BLOCKED_X:
                    h_xlist[nxl] = i
                    nxl += 1
            for i in range(next_fresh):
                if status[i] == QS_BLOCKED:
                    if exact_only:
                        h_xlist[nxl] = i
                        nxl += 1
                    else:
                        h_qlist[na] = i
                        na += 1
            while na + nxl < max_active and again:
                h_qlist[na] = again.pop()
                na += 1
            while na + nxl < max_active and next_fresh < nq:
                if exact_only:
                    h_xlist[nxl] = next_fresh
                    nxl += 1
                else:
                    h_qlist[na] = next_fresh
                    na += 1
                next_fresh += 1
            if not na and tl:
                short = sorted(short_sets.pop(0)) if short_sets else []
                script.append(" ".join(str(x) for x in [len(short)] + short))
                active, listed = na, True
                h_qlist[:len(short)] = short  # tl_collect_short writes them there
                snapshot("short")
                if short:
                    dev.restart(short)
                    again = list(short)
                    while na < max_active and again:
                        h_qlist[na] = again.pop()
                        na += 1
            active = na
            listed = True
            if not active and not nxl:
                snapshot("final")
                break
        elif not misses:
            snapshot("final")
            break
        snapshot("launch")
        assert len(rounds) < 10000
    return rounds, script


def parse(lines):
    rounds = []
    for ln in lines:
        if not ln.startswith("round "):
            continue
        head, verdict = ln.split(" -> ")
        w = head.split()
        listed = w[3] == "1"
        q, x = w[w.index("q") + 1:w.index("x")], w[w.index("x") + 1:]
        ql = [int(v) for v in q] if listed else ("all", int(q[0][3:-1]))
        rounds.append((listed, ql, [int(v) for v in x], verdict))
    return rounds


def check_properties(nq, cap, kind, rounds, script, short_sets):
    """What must hold of any schedule, whatever the restatement says."""
    status = [None] * nq  # of each query's last run
    ran = set()
    lines = iter(script)
    named = set()
    for n, (listed, q, x, verdict) in enumerate(rounds):
        if verdict == "short":
            named = set(int(v) for v in next(lines).split()[1:])
            continue
        if verdict == "final":
            assert (q == [] or q == ("all", 0)) and x == []
            break
        if kind == RERUN:
            assert not listed and q == ("all", 0) and x == []
            ids = list(range(nq))
        else:
            ids = (q if listed else list(range(q[1]))) + x
            assert 1 <= len(ids) <= cap and len(set(ids)) == len(ids)  # no more than the cap, nobody twice
            for i in ids:  # fresh, waiting for rows, or named by the retry: a finished query is never listed again
                assert status[i] in (None, QS_BLOCKED, QS_BLOCKED_X) or i in named, (n, i, status[i])
                named.discard(i)
            fresh = [i for i in ids if status[i] is None and i not in ran]
            assert fresh == list(range(len(ran), len(ran) + len(fresh)))  # started once each, in order
            parked = sorted(i for i in range(nq) if status[i] == QS_BLOCKED_X)
            assert x[:len(parked)] == parked  # those that hold a pool slot are in front of the exact list
            if kind == EXACT_QUEUE:
                assert q == []
            # every query that waits for rows runs in the very next round
            assert all(i in ids for i in range(nq) if status[i] in (QS_BLOCKED, QS_BLOCKED_X))
        ran.update(ids)
        line = [int(v) for v in next(lines).split()]
        assert len(line) == (nq if kind == RERUN else len(ran))
        for i, s in enumerate(line):
            status[i] = s
    assert ran == set(range(nq)) and not named
    assert rounds[-1][3] == "final" and all(s not in (QS_BLOCKED, QS_BLOCKED_X) for s in status)


def max_rounds(nq, in_flight, ef):  # restated (search.hip line 940 of the same commit)
    return 64 + ((nq + in_flight - 1) // in_flight) * (64 * ef + 4096)


CASES = [(RERUN, False, False), (PARK, False, False), (PARK, False, True), (PARK, True, False), (EXACT_QUEUE, False, False)]


@pytest.mark.parametrize("nq", [1, 2, 7, 64])
@pytest.mark.parametrize("kind,tl,mixed", CASES, ids=["rerun", "park", "park-exact-parks-too", "two-level", "exact-queue"])
def test_rounds_equal_the_loop_they_were_taken_from(dump, nq, kind, tl, mixed):
    for cap in (1, 2, 3, nq, nq + 5):
        # the two-level search's window retry (only it parks AND retries): none, one query, all of them
        retries = ["none", "one", "all"] if tl else ["none"]
        for retry in retries:
            for seed in range(3):
                rng = np.random.default_rng([nq, cap, kind, int(tl), int(mixed), retries.index(retry), seed])
                short_sets = {"none": [], "one": [[int(rng.integers(0, nq))]], "all": [list(range(nq))]}[retry]
                dev = Device(nq, kind, mixed, rng)
                for s in short_sets:  # (what names a query short on a device: QS_SCRATCH, payload 7)
                    for i in s:
                        dev.final[i] = QS_SCRATCH
                want, script = parent_rounds(nq, cap, kind, tl, dev, short_sets)
                out = dump("rounds %d %d %d %d %d\n" % (nq, cap, kind, int(tl), EF) + "\n".join(script) + "\n")
                got = parse(out)
                assert got == want, (cap, retry, seed)
                check_properties(nq, cap, kind, got, script, short_sets)
                n_rounds, _, most = out[-1].split()[1:]
                assert int(n_rounds) == sum(v != "short" for *_, v in want) - 1
                assert int(most) == max_rounds(nq, cap, EF) and int(n_rounds) <= int(most)  # ends within the round cap


def caps(dump, slab_rows, nvec, nq, tl, max_degree, use_fast, ef):
    out = dump("caps %d %d %d %d %d %d %d\n" % (slab_rows, nvec, nq, int(tl), max_degree, int(use_fast), ef))
    d = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in out}
    return {k: (v[0] if len(v) == 1 else v) for k, v in d.items()}


def test_caps_at_known_points(dump):
    for nq in (1, 100, 5000):  # a row for every node: the whole batch in flight, nothing parks in the exact kernel
        for slab in (1000, 1001, 1 << 20):
            c = caps(dump, slab, 1000, nq, False, 64, True, 64)
            assert c["in_flight"] == nq and c["kind"] == PARK
            assert caps(dump, slab, 1000, nq, False, 64, False, 1024)["kind"] == RERUN
    for deg in (1, 64, 128):  # a 256-row cache: one query at a time
        assert caps(dump, 256, 100000, 4096, False, deg, True, 64)["in_flight"] == 1
    assert caps(dump, 256, 100000, 4096, True, 500, False, 64)["in_flight"] == 1  # (two-level: hops of <= 128 rows)
    assert caps(dump, 255, 100000, 4096, False, 64, True, 64)["in_flight"] == 1   # never none
    assert caps(dump, 1 << 20, 10 ** 7, 10 ** 5, False, 64, True, 64)["in_flight"] == 4096
    long_rows = caps(dump, 1 << 20, 10 ** 7, 10 ** 5, False, 1024, False, 64)  # a parked hop holds a whole row
    assert long_rows["hop_rows"] == 2048 and long_rows["in_flight"] == 512 and long_rows["kind"] == EXACT_QUEUE
    assert caps(dump, 1 << 20, 10 ** 7, 10 ** 5, True, 1024, False, 64)["kind"] == PARK
    c = caps(dump, 256, 100000, 300, False, 64, True, 128)
    assert c["max_rounds"] == 64 + 300 * (64 * 128 + 4096)  # one group per query
    assert c["miss_capacity"] == 300 * 128 + 64 and c["prefetch_capacity"] == 300 * 8 + 64
    assert caps(dump, 256, 100000, 1 << 26, False, 64, True, 64)["miss_capacity"] == 0xFFFFFFF0
    assert c["stall_limit"] == 3 and caps(dump, 1000, 1000, 8, False, 64, False, 1024)["stall_limit"] == 1
    assert c["window"] == [1, 4, 16, 64]  # times 4 while below 64
