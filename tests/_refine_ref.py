"""The rescoring of include/islands_amd.h restated in numpy on top of oracle.batch_distance and
_entry_seeds_ref.ordkey: the scores, the stable (key, position) order, the skipping of ids >= n and the count.
Nothing here touches the library under test."""
import numpy as np

from _entry_seeds_ref import ordkey


def rescore_one(orc, metric: int, q, y, cand, k: int):
    """(ids, dist) of one query: s_i = D(q, y[cand[i]]) for the candidates that name a row, the first min(k, c')
    of them in ascending (ordkey(s_i), i)."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    cand = np.asarray(cand, dtype=np.uint64)
    pos = np.flatnonzero(cand < np.uint64(y.shape[0]))  # positions that are scored, in order
    if pos.size == 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.float32)
    rows = np.ascontiguousarray(y[cand[pos].astype(np.int64)])
    s = np.asarray(orc.batch_distance(metric, np.ascontiguousarray(q, dtype=np.float32), rows), dtype=np.float32)
    order = np.argsort(ordkey(s), kind="stable")[:k]  # stable: among equal keys the earlier position
    return cand[pos[order]], s[order]


def rescore(orc, metric: int, queries, y, cand_ids, cand_count, k: int):
    """[(ids, dist)] per query over cand_ids [nq, pitch], the first cand_count[q] of row q valid."""
    queries = np.ascontiguousarray(queries, dtype=np.float32)
    cand_ids = np.asarray(cand_ids, dtype=np.uint64).reshape(queries.shape[0], -1)
    return [rescore_one(orc, metric, queries[i], y, cand_ids[i, :int(cand_count[i])], k)
            for i in range(queries.shape[0])]


def score_bits(s) -> np.ndarray:
    """The bits of f32 scores with every NaN as ONE pattern.  A finite or infinite score is compared bit for bit,
    -0.0 and +0.0 apart.  A NaN is compared as "a NaN": IEEE 754 leaves sign and payload of a propagated NaN to the
    implementation (for a row with a NaN element the device's square root and divide answer 0xFFC00000 where the
    host's pass the operand 0x7FC00000 on), and the search's total order, the definition's, holds every NaN equal."""
    s = np.ascontiguousarray(s, dtype=np.float32)
    u = s.view(np.uint32).copy()
    u[np.isnan(s)] = 0x7FC00000
    return u


def same(answer, want) -> None:
    """ids, distance BITS (score_bits) and counts of (ids, dist, count) arrays against rescore()'s list: exact."""
    ids, dist, cnt = answer
    assert len(want) == ids.shape[0] == cnt.shape[0]
    for i, (wi, wd) in enumerate(want):
        m = int(cnt[i])
        assert m == wi.size, (i, m, wi.size)
        assert ids[i, :m].tolist() == wi.tolist(), (i, ids[i, :m], wi)
        got_bits, want_bits = score_bits(dist[i, :m]), score_bits(wd)
        assert got_bits.tolist() == want_bits.tolist(), (i, [hex(v) for v in dist[i, :m].view(np.uint32)],
                                                         [hex(v) for v in wd.view(np.uint32)])
