"""Randomised differential test of isl_hnsw_build with one node per step: random rows (optionally quantised
so that equal distances are common), n <= 300, d <= 40, m / m0 / ef_construction, levels, metric.  The
reference rule against the CPU oracle's HnswGraph::insert (bytes of the whole graph), the diverse rule
against the Python definition (tests/_hnsw_build_ref.py, every list).  Runs for `--seconds` on the GPU box:

    python tests/fuzz_hnsw_build.py --seconds 120 [--seed 0]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]  # run as a script

import numpy as np

import islands_amd as ia
import oracle as orc
import _hnsw_build_ref as ref
from _data import clustered_vectors, random_levels, uniform_vectors
from test_hnsw_bytes import hnsw_to_bincode


def one_case(rng, case):
    n = int(rng.choice([1, 2, 7, 40, 150, 300]))
    d = int(rng.choice([2, 5, 16, 33, 40]))
    seed = int(rng.integers(1 << 30))
    v = uniform_vectors(n, d, seed) if rng.random() < 0.6 else clustered_vectors(n, d, seed)
    if rng.random() < 0.3:  # equal distances everywhere: the heap-exact kernel decides
        v = (np.round(v * 2) / 2).astype(np.float32)
        v[np.abs(v).sum(1) == 0, 0] = 1.0
    m = int(rng.choice([2, 4, 8, 16, 33, 64]))
    m0 = int(rng.choice([m, 2 * m, min(128, 3 * m)]))
    efc = int(rng.choice([m0, 2 * m0, max(100, m0)]))
    metric = int(rng.integers(0, 4))
    if rng.random() < 0.7:
        lv = random_levels(n, max(2, m), seed + 5)
    else:  # a few forced climbs above the top layer
        lv = np.zeros(n, np.uint64)
        for i in rng.integers(0, n, size=min(n, 4)):
            lv[i] = int(rng.integers(1, 7))
    kw = dict(m=m, m0=m0, ef_construction=efc, metric=metric, ml=1.0 / np.log(m), levels=lv)
    if rng.random() < 0.5:
        h = orc.Hnsw(m=m, m0=m0, ef_construction=efc, metric=metric)
        for i in range(n):
            st, idx = h.insert(v[i], int(lv[i]))
            assert st == 0 and idx == i
        layers = [[(h.neighbors(i, L) or []) for i in range(n)] for L in range(h.max_level + 1)]
        want = hnsw_to_bincode(v, layers, [int(x) for x in lv], h.entry_point, h.max_level, m=m, m0=m0,
                               ef_construction=efc, metric=metric)
        got = ia.HnswGraph.build(v, **kw)
        assert got.to_bytes() == want, ("reference", case, n, d, m, m0, efc, metric, seed)
        return "reference"
    alpha = float(rng.choice([1.0, 1.1, 1.5]))
    keep = bool(rng.random() < 0.5)
    want = ref.build(orc, v, lv, m, m0, efc, metric, "diverse", alpha, keep)
    got = ia.HnswGraph.build(v, select="diverse", alpha=alpha, keep_pruned=keep, **kw)
    assert got.entry_point == want.entry and got.max_level == want.max_level, ("diverse", case)
    for i in range(n):
        for L in range(int(lv[i]) + 1):
            assert got.neighbors(i, L) == list(want.conn[i][L]), ("diverse", case, n, d, m, m0, efc, metric, seed,
                                                                  alpha, keep, i, L)
    return "diverse"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    orc.build()
    rng = np.random.default_rng(args.seed)
    t0, count = time.time(), {"reference": 0, "diverse": 0}
    while time.time() - t0 < args.seconds:
        count[one_case(rng, sum(count.values()))] += 1
        if sum(count.values()) % 20 == 0:
            print(f"{sum(count.values())} cases ok", flush=True)
    print(f"fuzz hnsw_build ok: {count['reference']} reference-rule cases equal to the oracle, "
          f"{count['diverse']} diverse-rule cases equal to the definition")


if __name__ == "__main__":
    main()
