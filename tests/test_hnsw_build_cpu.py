"""isl_hnsw_build without a device: the Python restatement of the construction (tests/_hnsw_build_ref.py)
against the oracle's HnswGraph::insert, what the two selection rules leave behind, and every part of the
new entry points that needs no GPU (argument checks, seeded levels, the empty graph, to_bytes)."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import islands_amd as ia
import _hnsw_build_ref as ref
from _data import clustered_vectors, random_levels, uniform_vectors
from test_hnsw_bytes import hnsw_to_bincode


def oracle_graph(orc, v, lv, m, m0, efc, metric):
    h = orc.Hnsw(m=m, m0=m0, ef_construction=efc, metric=int(metric))
    for i in range(v.shape[0]):
        st, idx = h.insert(v[i], int(lv[i]))
        assert st == 0 and idx == i
    return h


def assert_equals_oracle(orc, v, lv, m, m0, efc, metric):
    h = oracle_graph(orc, v, lv, m, m0, efc, metric)
    g = ref.build(orc, v, lv, m, m0, efc, metric, "reference")
    assert g.entry == h.entry_point and g.max_level == h.max_level
    for i in range(v.shape[0]):
        for L in range(int(lv[i]) + 1):
            assert list(h.neighbors(i, L) or []) == list(g.conn[i][L]), (i, L)
    return h


@pytest.mark.parametrize("metric", [0, 1, 2, 3])
def test_reference_helper_is_the_oracle(orc, metric):
    h = assert_equals_oracle(orc, uniform_vectors(600, 24, 11), random_levels(600, 16, 14), 16, 32, 200, metric)
    assert h.max_level >= 1


def test_reference_helper_ties(orc):
    base = uniform_vectors(60, 8, 3)
    v = np.concatenate([base, base, base[:30], base[:60]]).astype(np.float32)  # 210 rows, equal distances
    assert_equals_oracle(orc, v, random_levels(v.shape[0], 6, 24), 6, 12, 30, 1)


def forced_levels(n=300):
    lv = np.zeros(n, np.uint64)
    lv[5], lv[40], lv[100], lv[101], lv[200] = 3, 1, 5, 5, 2
    return lv


def test_reference_helper_rising_top_layer(orc):
    lv = forced_levels()
    h = assert_equals_oracle(orc, uniform_vectors(300, 16, 9), lv, 8, 16, 64, 0)
    assert h.entry_point == 100 and h.max_level == 5
    # the first node above the top layer lists the old entry on layers that node lacks (no back link there)
    assert list(h.neighbors(100, 5)) == [5, 101] and list(h.neighbors(101, 5)) == [100, 5]
    assert h.level(5) == 3


@pytest.mark.parametrize("shape", [(32, 64, 400, 0), (64, 128, 256, 1)])
def test_reference_helper_wide_lists(orc, shape):
    m, m0, efc, metric = shape
    assert_equals_oracle(orc, uniform_vectors(400, 12, 33), random_levels(400, m, 5), m, m0, efc, metric)


def test_step_planner():
    lv = forced_levels()
    steps = ref.plan_steps(lv, 64)
    assert steps[0] == (0, 1) and sum(c for _, c in steps) == 300
    assert [s for s in steps if s[0] <= 5 < s[0] + s[1]] == [(5, 1)]
    assert [s for s in steps if s[0] <= 100 < s[0] + s[1]] == [(100, 1)]
    assert (101, 1) not in steps  # level 5 == the top layer by then: an ordinary node
    for (a, ca), (b, _) in zip(steps, steps[1:]):
        assert a + ca == b and ca <= max(1, a // 8) and ca <= 64
    assert ref.plan_steps(lv, 1) == [(i, 1) for i in range(300)]


@pytest.fixture(scope="module")
def plan_dump():
    """tests/cpp/build_plan_dump.cpp: the library's own planner (build_plan.hpp), built with g++ alone"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "islands_amd", "lib", "build_plan_dump")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "cpp", "build_plan_dump.cpp"),
                           "-o", exe])

    def run(levels, batch):
        text = f"{batch} {len(levels)}\n" + " ".join(str(int(x)) for x in levels) + "\n"
        out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60, check=True).stdout
        lines = out.splitlines()
        steps = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("step")]
        order = [int(x) for x in next(ln for ln in lines if ln.startswith("order")).split()[1:]]
        largest = int(next(ln for ln in lines if ln.startswith("largest")).split()[1])
        return steps, order, largest

    return run


PLAN_LEVELS = [("forced", forced_levels)] + [
    (f"random{n}", lambda n=n: random_levels(n, 16, 40 + n)) for n in (1, 2, 9, 300, 5000)] + [
    ("flat", lambda: np.zeros(5000, np.uint64))]  # all-zero levels: the steps of LeannIndex::build


@pytest.mark.parametrize("batch", [1, 64, 4096])
@pytest.mark.parametrize("levels", [c[1] for c in PLAN_LEVELS], ids=[c[0] for c in PLAN_LEVELS])
def test_library_step_planner(plan_dump, levels, batch):
    """plan_steps of build_plan.hpp == the tests' planner; inside a step the nodes are the step's id range in
    level order, highest first, equal levels in id order (so the nodes that have a layer are a prefix)"""
    lv = levels()
    steps, order, largest = plan_dump(lv, batch)
    assert [(0, 1)] + [(first, count) for first, count, _ in steps] == ref.plan_steps(lv, batch)
    assert len(order) == len(lv) and order[0] == 0
    for first, count, top in steps:
        want = sorted(range(first, first + count), key=lambda i: -int(lv[i]))  # sorted() is stable
        assert order[first:first + count] == want, (first, count)
        assert top == max(int(lv[i]) for i in range(first, first + count))
    assert largest == max([c for _, c, _ in steps] + [1])
    if not np.any(lv):
        assert order == list(range(len(lv)))  # the flat builder's case: no reorder


@pytest.mark.parametrize("case", [("uniform", 0), ("clustered", 1)])
def test_diverse_rule_keeps_every_node_reachable(orc, case):
    """The reference rule's prune drops the node being inserted from every full list: recorded here as the
    contrast (>= 0.9 n nodes without an inbound layer-0 edge; measured 1468 / 1469 of 1500), so that nobody
    repairs the reference rule by accident.  The diverse rule leaves none and finds every probed row."""
    kind, metric = case
    n, d, m, m0, efc = 1500, 16, 8, 16, 64
    v = uniform_vectors(n, d, 21) if kind == "uniform" else clustered_vectors(n, d, 21)
    lv = random_levels(n, m, 3)
    h = oracle_graph(orc, v, lv, m, m0, efc, metric)
    unreachable = ref.no_inbound([h.neighbors(i, 0) or [] for i in range(n)])
    print(f"{kind}: reference rule, nodes without an inbound layer-0 edge: {unreachable} of {n}")
    assert unreachable >= 0.9 * n
    g = ref.build(orc, v, lv, m, m0, efc, metric, "diverse")
    lost = ref.no_inbound([g.conn[i][0] for i in range(n)])
    probes = range(0, n, 15)
    hits = sum(1 for i in probes if g.search(v[i], 1, 64)[0][:1] == [i])
    print(f"{kind}: diverse rule, without an inbound edge: {lost}; self-query recall@1 {hits}/{len(probes)}")
    assert lost == 0
    assert hits == len(probes)


# ---------------------------------------------------------------- the entry points, no device needed
def kind_of(**kw):
    with pytest.raises(ia.CoreError) as e:
        ia.HnswGraph.build(kw.pop("vectors", uniform_vectors(8, 4, 1)), **kw)
    return e.value.kind


def test_build_argument_checks():
    assert kind_of(m=0) == "InvalidConfig"
    assert kind_of(m=16, m0=8) == "InvalidConfig"
    assert kind_of(m=16, m0=32, ef_construction=8) == "InvalidConfig"
    assert kind_of(vectors=np.zeros((4, 0), np.float32)) == "EmptyCollection"
    assert kind_of(levels=[0, 1, 16, 0, 0, 0, 0, 0]) == "InvalidArgument"
    assert kind_of(levels=[0, 1, 3, 0, 0, 0, 0, 0], max_layers=3) == "InvalidArgument"
    assert kind_of(m=16, m0=129, ef_construction=200) == "Unsupported"
    assert kind_of(ef_construction=513) == "Unsupported"
    assert kind_of(select="diverse", alpha=0.5) == "InvalidConfig"
    assert kind_of(select=7) == "InvalidArgument"
    # the order: options, then the config, then the data
    assert kind_of(select=7, m=0) == "InvalidArgument"
    assert kind_of(m=0, vectors=np.zeros((4, 0), np.float32)) == "InvalidConfig"
    assert kind_of(m0=129, levels=[99] * 8) == "InvalidArgument"
    with pytest.raises(ValueError):
        ia.HnswGraph.build(uniform_vectors(8, 4, 1), levels=[0, 0])


def test_empty_build_and_its_bytes():
    g = ia.HnswGraph.build(np.zeros((0, 0), np.float32), m=8, m0=16, ef_construction=64, metric=1,
                           ml=1.0 / np.log(8))
    assert len(g) == 0 and g.entry_point is None and g.max_level == 0 and g.levels().size == 0
    empty = hnsw_to_bincode(np.zeros((0, 0), np.float32), [[]], [], None, 0, m=8, m0=16, ef_construction=64,
                            metric=1, dimension=None)
    assert g.to_bytes() == empty
    assert g.search_batch(np.zeros((2, 4), np.float32), 3, 8) == [] or all(
        len(ids) == 0 for ids, _ in g.search_batch(np.zeros((2, 4), np.float32), 3, 8))
    assert g.neighbors(0, 0) is None and g.get_vector(0) is None


def test_to_bytes_keeps_ml_and_max_layers():
    blob = bytearray(hnsw_to_bincode(np.zeros((0, 0), np.float32), [[]], [], None, 0, m=5, m0=9,
                                     ef_construction=33, metric=3, dimension=None))
    blob[24:32] = struct.pack("<d", 0.75)
    blob[36:44] = struct.pack("<Q", 7)
    out = ia.HnswGraph.from_bytes(bytes(blob)).to_bytes()
    assert out == bytes(blob)
    assert struct.unpack("<d", out[24:32])[0] == 0.75 and struct.unpack("<Q", out[36:44])[0] == 7


def test_random_levels():
    ml = 1.0 / math.log(16)
    a = ia.HnswGraph.random_levels(100_000, seed=7)
    assert a.tolist() == ia.HnswGraph.random_levels(100_000, seed=7).tolist()
    assert a.tolist() != ia.HnswGraph.random_levels(100_000, seed=8).tolist()
    assert a[:1000].tolist() == ia.HnswGraph.random_levels(1000, seed=7).tolist()  # a function of (seed, i)
    # P(level >= 1) = P(-ln r * ml >= 1) = exp(-1 / ml)
    p = math.exp(-1.0 / ml)
    sigma = math.sqrt(p * (1 - p) / a.size)
    assert abs(float((a >= 1).mean()) - p) <= 3 * sigma
    assert int(a.max()) <= 15
    capped = ia.HnswGraph.random_levels(100_000, ml=3.0, max_layers=4, seed=1)
    assert int(capped.max()) == 3 and int(capped.min()) == 0
    assert ia.HnswGraph.random_levels(50, max_layers=1, seed=2).tolist() == [0] * 50
    # the documented generator: splitmix64 stream of the seed, r = ((x >> 11) + 0.5) * 2^-53
    M = (1 << 64) - 1

    def level(seed, i):
        z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        z ^= z >> 31
        r = ((z >> 11) + 0.5) * 2.0 ** -53
        return min(int(math.floor(-math.log(r) * ml)), 15)

    assert a[:2000].tolist() == [level(7, i) for i in range(2000)]
    with pytest.raises(ia.CoreError) as e:
        ia.HnswGraph.random_levels(4, max_layers=0)
    assert e.value.kind == "InvalidArgument"
