"""The diverse (occlusion) selection rule of isl_index_build_ex restated in Python, as the tests'
definition: every pair distance goes through the oracle's f32 chain (Distance::calculate, first
argument first), the construction search is the oracle's, every sort is stable.

select(b, C, M, alpha, keep_pruned), C = candidate ids in ascending d(b, c):
  1. kept = [], dropped = [].  For each c in order: c is occluded iff some s already in kept has
     alpha * d(s, c) <= d(b, c) (f32 multiply, then compare; a NaN occludes nothing).
     Occluded -> dropped, else -> kept.  Stop when len(kept) == M.
  2. If keep_pruned and len(kept) < M: append dropped in its order until M.
  3. The row is kept, then the fillers.
"""
import numpy as np


def select_sorted(orc, v, metric, cids, dbc, M, alpha=1.0, keep_pruned=True):
    """The definition, for candidates `cids` already in ascending `dbc` = d(b, c)."""
    cids = [int(c) for c in cids]
    dbc = np.asarray(dbc, dtype=np.float32)
    alpha = np.float32(alpha)
    rows = v[np.asarray(cids, dtype=np.int64)] if cids else v[:0]
    kept, dropped = [], []  # positions in cids
    # row j: d(vec[kept[j]], vec[c]) for every candidate c (the kept one is the first argument)
    from_kept = np.zeros((max(M, 1), len(cids)), dtype=np.float32)
    for c in range(len(cids)):
        if len(kept) == M:
            break
        with np.errstate(invalid="ignore"):
            occluded = bool(np.any(alpha * from_kept[:len(kept), c] <= dbc[c]))  # f32 * f32, then compare
        if occluded:
            dropped.append(c)
        else:
            from_kept[len(kept)] = orc.batch_distance(int(metric), v[cids[c]], rows)
            kept.append(c)
    row = list(kept)
    if keep_pruned:
        for c in dropped:
            if len(row) >= M:
                break
            row.append(c)
    return [cids[c] for c in row]


def sort_by_base(orc, v, metric, base, cand):
    """d(base, c) for the candidates as given and the stable ascending order by it."""
    cand = np.asarray(cand, dtype=np.int64)
    if cand.size == 0:
        return cand, np.zeros(0, np.float32)
    dd = orc.batch_distance(int(metric), v[int(base)], v[cand])
    order = np.argsort(dd, kind="stable")
    return cand[order], dd[order]


def select(orc, v, metric, base, cand, M, alpha=1.0, keep_pruned=True):
    """select() over candidates in any order: what isl_select_neighbors computes for one base."""
    cids, dd = sort_by_base(orc, v, metric, base, cand)
    return select_sorted(orc, v, metric, cids, dd, M, alpha, keep_pruned)


def _csr(orc, rows, entry):
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    nb = np.fromiter((x for r in rows for x in r), dtype=np.uint64, count=int(off[-1]))
    return orc.Csr(off, nb, entry)


def build(orc, v, m0, ef_construction, metric=0, alpha=1.0, keep_pruned=True, levels=None):
    """The sequential build under the diverse rule: nodes in id order, the oracle's construction
    search from the entry point, select() for the new node with the search's distances, back links
    in row order with a re-select of a row that reaches m0 + 1 ids.  Returns an oracle Csr with
    levels, entry point and max level as LeannIndex::build leaves them."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    n = v.shape[0]
    lv = np.zeros(n, dtype=np.uint64) if levels is None else np.asarray(levels, dtype=np.uint64)
    rows = [[] for _ in range(n)]
    entry, max_level = 0, int(lv[0])
    for i in range(1, n):
        r = orc.leann_search(_csr(orc, rows, entry), v, v[i], ef_construction, ef_construction,
                             metric=int(metric))
        assert r.status == 0, r.status
        sel = select_sorted(orc, v, metric, r.ids, r.dist, m0, alpha, keep_pruned)
        rows[i] = list(sel)
        for s in sel:
            if i in rows[s]:
                continue
            rows[s].append(i)
            if len(rows[s]) == m0 + 1:
                cids, dd = sort_by_base(orc, v, metric, s, rows[s])
                rows[s] = select_sorted(orc, v, metric, cids, dd, m0, alpha, keep_pruned)
        if int(lv[i]) > max_level:
            entry, max_level = i, int(lv[i])
    g = _csr(orc, rows, entry)
    g.levels = lv.copy()
    g.max_level = max_level
    return g
