"""isl_index_remove restated in Python, as the tests' definition (include/islands_amd.h has the text).

Inputs: the lists L[p] of a flat index in their stored order, the rows, the set D of ids to remove, the
selection rule.

1. Repair over the old ids, every list from the OLD lists only.  For a survivor p: no id of L[p] in D ->
   L'[p] = L[p].  Otherwise C(p): walk L[p] in stored order; a survivor x emits x; a removed x emits every y of
   L[x] in stored order with y not in D and y != p; first occurrences only; stop after MAX_CANDIDATES distinct
   ids.  |C(p)| <= m0 -> L'[p] = C(p).  Otherwise d(p, c) through the oracle's f32 chain (Distance::calculate,
   p first), a stable ascending sort, and the first m0 (reference rule) or _diverse_ref.select_sorted.
2. Compaction, order kept: new id = old id minus the removed ids below it; a surviving entry point is kept,
   otherwise the lowest new id among the survivors of the highest level takes over with that level as
   max_level.
"""
import numpy as np

import _diverse_ref as dref

MAX_CANDIDATES = 512
REMOVED = 0xFFFFFFFFFFFFFFFF


def lists_of(csr):
    off = np.asarray(csr.node_offsets, dtype=np.int64)
    nb = np.asarray(csr.neighbors, dtype=np.int64)
    return [nb[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]


def candidates(lists, gone, p):
    """C(p) of a survivor p that has a removed neighbour"""
    out, seen = [], set()
    for x in lists[p]:
        for y in ([x] if x not in gone else [y for y in lists[x] if y not in gone and y != p]):
            if y not in seen:
                seen.add(y)
                out.append(y)
                if len(out) == MAX_CANDIDATES:
                    return out
    return out


def remap_of(n, gone):
    remap = np.full(n, REMOVED, dtype=np.uint64)
    keep = [i for i in range(n) if i not in gone]
    remap[keep] = np.arange(len(keep), dtype=np.uint64)
    return remap, keep


def entry_after(levels, keep, remap, entry, max_level):
    """(entry point, max_level) of the survivors `keep` (old ids, ascending)"""
    if entry is None or not keep:
        return None, (max_level if keep else 0)
    if remap[entry] != REMOVED:
        return int(remap[entry]), max_level
    lv = [int(levels[i]) for i in keep]
    top = max(lv)
    return lv.index(top), top


def repaired_lists(orc, lists, v, gone, m0, metric=0, rule="reference", alpha=1.0, keep_pruned=True, stats=None):
    """step 1: {survivor: L'[p]} over the old ids"""
    out = {}
    for p in range(len(lists)):
        if p in gone:
            continue
        if not any(x in gone for x in lists[p]):
            out[p] = list(lists[p])
            continue
        c = candidates(lists, gone, p)
        if stats is not None:
            stats.append((p, len(c)))
        if len(c) > m0:
            cids, dd = dref.sort_by_base(orc, v, metric, p, c)  # the reference rule: a stable argsort cut at m0
            if rule == "diverse":
                c = dref.select_sorted(orc, v, metric, cids, dd, m0, alpha, keep_pruned)
            else:
                c = [int(x) for x in cids[:m0]]
        out[p] = c
    return out


def remove(orc, csr, v, ids, m0, metric=0, rule="reference", alpha=1.0, keep_pruned=True, stats=None):
    """The definition: (oracle Csr of the shrunk graph, remap [old len] u64)."""
    lists = lists_of(csr)
    n = len(lists)
    gone = set(int(i) for i in ids)
    assert all(0 <= i < n for i in gone)
    v = np.ascontiguousarray(v, dtype=np.float32)
    fixed = repaired_lists(orc, lists, v, gone, m0, int(metric), rule, alpha, keep_pruned, stats)
    remap, keep = remap_of(n, gone)
    rows = [[int(remap[y]) for y in fixed[p]] for p in keep]
    levels = np.asarray(csr.levels, dtype=np.uint64)
    entry, max_level = entry_after(levels, keep, remap, csr.entry_point, int(csr.max_level))
    off = np.zeros(len(keep) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    nb = np.fromiter((x for r in rows for x in r), dtype=np.uint64, count=int(off[-1]))
    g = orc.Csr(off, nb, entry)
    g.levels = levels[keep].copy() if keep else np.zeros(0, np.uint64)
    g.max_level = max_level
    return g, remap
