"""The planner of the grouped search launches (islands_amd/csrc/search_group_plan.hpp) without a device:
tests/cpp/search_group_plan_dump.cpp, built with g++ alone and a second time under AddressSanitizer and
UndefinedBehaviorSanitizer, is fed seeded scripts of arrivals, completions and waits; every launch it prints is
compared with a Python restatement of the rules, and with what must hold of any schedule whatever the
restatement says."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "search_group_plan_dump.cpp")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def dump(request):
    if request.param == "plain":
        exe = os.path.join(ROOT, "islands_amd", "lib", "search_group_plan_dump")
        cmd = ["g++", "-std=c++17", "-O1", SRC, "-o", exe]
    else:  # the compiler of `make asan` (tests/test_asan_host.py), on the stand-alone driver
        exe = os.path.join(ROOT, "islands_amd", "lib", "asan", "search_group_plan_dump")
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


class Model:
    """The rules as the issue states them.  A call is submitted at once while fewer than `room` queries are in
    flight, with every compatible held call, as one launch; otherwise it is held.  A held set goes out when its
    queries reach cap, when a pump finds room, or when a member is waited for; more than cap is cut in arrival
    order.  One call alone needs no workspace; several need a free one, else the set stays held (and a member
    that is waited for goes alone)."""

    def __init__(self, cap, workspaces):
        self.cap, self.ws_busy = cap, [False] * workspaces
        self.held = []      # (call, nq, key, room) in arrival order
        self.flights = {}   # id -> dict(nq, ws, calls, complete)
        self.inflight = 0
        self.next_id = 1
        self.out = []

    def _take(self, key, forced, wanted):
        pick, total = [], 0
        for h in self.held:
            if h[2] != key:
                continue
            if pick and total + h[1] > self.cap:
                break
            pick.append(h)
            total += h[1]
        if not pick:
            return False
        ws = -1
        if len(pick) > 1:
            free = [w for w, b in enumerate(self.ws_busy) if not b]
            if free:
                ws = free[0]
            elif not forced:
                return False
            else:
                pick = [h for h in self.held if h[0] == wanted]
        members, off = [], 0
        for h in pick:
            members.append((h[0], h[1], off))
            off += h[1]
            self.held.remove(h)
        if ws >= 0:
            self.ws_busy[ws] = True
        self.flights[self.next_id] = dict(nq=off, ws=ws, calls=[m[0] for m in members], complete=False)
        self.inflight += off
        self.out.append((self.next_id, ws, off, key, members))
        self.next_id += 1
        return True

    def submit(self, wanted=None):
        while True:
            if wanted is not None and not any(h[0] == wanted for h in self.held):
                wanted = None
            if wanted is not None:
                key = next(h[2] for h in self.held if h[0] == wanted)
                if not self._take(key, True, wanted):
                    break
                continue
            seen, went = [], False
            for h in list(self.held):
                if h[2] in seen:
                    continue
                seen.append(h[2])
                total = sum(x[1] for x in self.held if x[2] == h[2])
                if (total >= self.cap or self.inflight < h[3]) and self._take(h[2], False, None):
                    went = True
                    break
            if not went:
                break

    def arrive(self, call, nq, key, room):
        self.held.append((call, nq, key, room))
        self.submit()

    def complete(self, lid):
        f = self.flights.get(lid)
        if f and not f["complete"]:
            f["complete"] = True
            self.inflight -= f["nq"]

    def done(self, call):
        for lid, f in list(self.flights.items()):
            if call in f["calls"]:
                f["calls"].remove(call)
                self.complete(lid)
                if not f["calls"]:
                    if f["ws"] >= 0:
                        self.ws_busy[f["ws"]] = False
                    del self.flights[lid]
                break
        self.submit()


def parse(lines):
    launches, states = [], []
    for ln in lines:
        w = ln.split()
        if w[0] == "launch":
            members = [(int(m.split("/")[0]), int(m.split("/")[1].split("@")[0]), int(m.split("@")[1])) for m in w[w.index(":") + 1:]]
            launches.append((int(w[1]), int(w[3]), int(w[5]), (int(w[7]), int(w[8]), int(w[9])), members))
        elif w[0] == "state":
            states.append((int(w[2]), int(w[4])))
    return launches, states


def run_script(dump, cap, workspaces, room, n_calls, seed, keys):
    """A seeded life of `n_calls` lanes: calls arrive, launches complete, calls are waited for and finish.  Every
    call that arrives is eventually waited for.  Returns (launches, arrivals) after checking model == program."""
    rng = np.random.default_rng([cap, workspaces, room, n_calls, seed, len(keys)])
    model = Model(cap, workspaces)
    script = ["config %d %d" % (cap, workspaces)]
    states = [(0, 0)]  # (after "config")
    free = list(range(n_calls))
    live = {}       # call -> (nq, key): arrived, wait not over
    arrivals = {}   # (call, generation) bookkeeping for the properties
    order = []
    for step in range(200):
        r = rng.random()
        launched_calls = [c for f in model.flights.values() for c in f["calls"]]
        if free and (r < 0.5 or not live):
            call = free.pop(int(rng.integers(0, len(free))))
            nq = int(rng.choice([1, 3, 17, 40, 64, cap // 2, cap - 1, cap]))
            nq = max(1, min(nq, cap))
            key = keys[int(rng.integers(0, len(keys)))]
            live[call] = (nq, key)
            order.append(("arrive", call, nq, key, len(model.out)))
            script.append("arrive %d %d %d %d %d %d" % (call, nq, key[0], key[1], key[2], room))
            model.arrive(call, nq, key, room)
        elif r < 0.6:
            script.append("pump")
            model.submit()
        elif r < 0.75 and model.flights:
            lid = int(rng.choice(sorted(model.flights)))
            script.append("complete %d" % lid)
            model.complete(lid)
        elif live:
            call = int(rng.choice(sorted(live)))
            script.append("wait %d" % call)
            model.submit(call)
            states.append((model.inflight, len(model.held)))
            assert not any(h[0] == call for h in model.held)  # no call is held once it is waited for
            script.append("done %d" % call)
            before = len(model.out)
            model.done(call)
            order.append(("done", call, before, len(model.out)))
            del live[call]
            free.append(call)
        else:
            continue
        states.append((model.inflight, len(model.held)))
    for call in sorted(live):  # everybody is waited for in the end
        script.append("wait %d" % call)
        model.submit(call)
        states.append((model.inflight, len(model.held)))
        script.append("done %d" % call)
        before = len(model.out)
        model.done(call)
        order.append(("done", call, before, len(model.out)))
        states.append((model.inflight, len(model.held)))
    got, got_states = parse(dump("\n".join(script) + "\n"))
    assert got == model.out, (cap, workspaces, room, seed)
    assert got_states == states
    assert got_states[-1] == (0, 0)
    return got, order


def check_properties(launches, order, cap, workspaces):
    """Whatever the restatement says: one launch per call and arrival, members of one key, offsets the prefix sums,
    no launch over cap, arrival order inside a launch, a workspace for every launch of several calls and never two
    launches on one workspace while a member of the first is not finished."""
    arrived = {}     # call -> (nq, key) of its current arrival
    seq = {}         # call -> arrival number
    n_arr = 0
    busy = {}        # workspace -> set of calls not finished
    launched = set()
    li = 0

    def apply_launches(upto):
        nonlocal li
        while li < upto:
            lid, ws, nq, key, members = launches[li]
            assert 1 <= nq <= cap and nq == sum(m[1] for m in members)
            off = 0
            for call, mnq, moff in members:
                assert arrived[call] == (mnq, key) and moff == off and call not in launched
                launched.add(call)
                off += mnq
            assert [seq[m[0]] for m in members] == sorted(seq[m[0]] for m in members) or ws == -1
            if len(members) > 1:
                assert 0 <= ws < workspaces and not busy.get(ws)
                busy[ws] = set(m[0] for m in members)
            else:
                assert ws == -1
            li += 1

    # replay in program order: `order` entries carry how many launches existed before them
    for o in order:
        if o[0] == "arrive":
            _, call, nq, key, before = o
            apply_launches(before)
            arrived[call] = (nq, key)
            seq[call] = n_arr
            n_arr += 1
        else:
            _, call, before, after = o
            apply_launches(before)
            assert call in launched  # it went out, at its wait at the latest
            launched.discard(call)
            for ws in busy:
                busy[ws].discard(call)
            apply_launches(after)  # (what the pump behind the wait released, perhaps onto the workspace just freed)
    apply_launches(len(launches))
    assert not launched


KEYS_ONE = [(32, 5, 32)]
KEYS_MANY = [(32, 5, 32), (32, 5, 64), (32, 10, 32), (50, 5, 32)]


@pytest.mark.parametrize("cap", [64, 100, 4096])
@pytest.mark.parametrize("workspaces", [0, 1, 3])
def test_launches_equal_the_rules(dump, cap, workspaces):
    for room in (1, 64, 3072):
        for keys in (KEYS_ONE, KEYS_MANY):
            for seed in range(3):
                launches, order = run_script(dump, cap, workspaces, room, 8, seed, keys)
                check_properties(launches, order, cap, workspaces)
                if workspaces == 0:
                    assert all(len(m) == 1 for *_, m in launches)


def test_hold_submit_and_cap_cut_at_known_points(dump):
    key = "32 5 32"
    # room 100: the first call goes at once, the next two are held until the third makes 128 >= cap 128
    out, st = parse(dump("\n".join(["config 128 2", "arrive 0 100 %s 100" % key, "arrive 1 64 %s 100" % key,
                                    "arrive 2 64 %s 100" % key]) + "\n"))
    assert out == [(1, -1, 100, (32, 5, 32), [(0, 100, 0)]), (2, 0, 128, (32, 5, 32), [(1, 64, 0), (2, 64, 64)])]
    assert st == [(0, 0), (100, 0), (100, 1), (228, 0)]
    # a pump finds room only once the launch in flight has been seen complete
    out, st = parse(dump("\n".join(["config 128 2", "arrive 0 100 %s 100" % key, "arrive 1 10 %s 100" % key, "pump",
                                    "complete 1", "pump"]) + "\n"))
    assert [o[0] for o in out] == [1, 2] and st == [(0, 0), (100, 0), (100, 1), (100, 1), (0, 1), (10, 0)]
    # more than cap held (no workspace was free while they arrived): cut in arrival order, member offsets the prefix sums
    script = ["config 100 1", "arrive 0 100 %s 1" % key, "arrive 1 40 %s 1" % key, "arrive 2 40 %s 1" % key,
              "arrive 3 40 %s 1" % key, "arrive 4 40 %s 1" % key, "arrive 5 40 %s 1" % key, "wait 5"]
    out, st = parse(dump("\n".join(script) + "\n"))
    assert [o[4] for o in out] == [[(0, 100, 0)], [(1, 40, 0), (2, 40, 40)], [(5, 40, 0)]]  # 5 alone: no workspace left
    assert st[-1] == (220, 2)
    # calls that differ in k or ef never share a launch, and each set waits for its own trigger
    script = ["config 128 2", "arrive 0 100 32 5 32 1", "arrive 1 10 32 5 32 1", "arrive 2 10 32 5 64 1",
              "arrive 3 10 32 7 32 1", "arrive 4 10 32 5 32 1", "wait 2", "wait 4"]
    out, _ = parse(dump("\n".join(script) + "\n"))
    assert [(o[3], o[4]) for o in out] == [((32, 5, 32), [(0, 100, 0)]), ((32, 5, 64), [(2, 10, 0)]),
                                           ((32, 5, 32), [(1, 10, 0), (4, 10, 10)])]


def test_traits_and_workspaces(dump):
    def groupable(*a):
        return dump("traits " + " ".join(str(int(v)) for v in a) + "\n")[0] == "groupable 1"

    assert groupable(1, 0, 0, 0, 0, 0, 1024, 0, 4096)
    assert groupable(1, 0, 0, 0, 0, 0, 4096, 0, 4096) and not groupable(1, 0, 0, 0, 0, 0, 4097, 0, 4096)
    assert not groupable(1, 0, 0, 0, 0, 0, 1024, 1, 4096)  # ISL_NO_GROUP
    for flag in range(6):  # host buffers, recompute, two-level, HnswGraph, construction, ISL_TIMELINE / ISL_DEBUG
        a = [1, 0, 0, 0, 0, 0]
        a[flag] ^= 1
        assert not groupable(*a, 1024, 0, 4096)
    ws = lambda lanes, nq, cap: [int(v) for v in dump("workspaces %d %d %d\n" % (lanes, nq, cap))[0].split()[1::2]]
    assert ws(32, 1024, 4096) == [9, 4096]   # 32 x 1024 queries in launches of 4096, one to spare
    assert ws(32, 1024, 1024) == [16, 1024]  # never more than lanes / 2: such a launch has two members at least
    assert ws(6, 64, 4096) == [2, 384]
    assert ws(1, 1024, 4096) == [0, 1024]
