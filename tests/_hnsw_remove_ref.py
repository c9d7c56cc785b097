"""isl_hnsw_remove restated in Python, as the tests' definition (include/islands_amd.h has the text).

Inputs: layers[L][p] = neighbors_at(L) of node p in stored order (empty where p lacks the layer), the levels, the
entry point and max_level, the rows, the set D of ids to remove, the selection rule, m and m0.

1. Repair, per layer, every list from the OLD lists of that layer only.  For a survivor p with level[p] >= L: no id
   of L_L[p] in D -> unchanged.  Otherwise C_L(p) = _remove_ref.candidates over layer L's lists, in which a node
   that lacks the layer has the empty list: a surviving x emits x whether or not it has the layer, a removed x
   emits its layer-L list and so nothing where it has none.  |C_L(p)| <= M_L -> C_L(p); otherwise
   _diverse_ref.sort_by_base and the first M_L (reference rule) or select_sorted.  M_L = m0 on layer 0, m above.
2. Compaction, order kept: _remove_ref.remap_of and entry_after; the layers above the new max_level go.
"""
import numpy as np

import _diverse_ref as dref
import _remove_ref as rref

REMOVED = rref.REMOVED


class Shrunk:
    """what remove() returns: layers[L][new id] (lists of new ids), levels, entry, max_level, remap [old len] u64"""

    def __init__(self, layers, levels, entry, max_level, remap):
        self.layers, self.levels, self.entry, self.max_level, self.remap = layers, levels, entry, max_level, remap

    def __len__(self):
        return len(self.levels)


def repaired_layer(orc, lists, levels, L, v, gone, cap, metric, rule, alpha, keep_pruned, stats=None):
    """step 1 on one layer: {survivor that has the layer: L'_L[p]} over the old ids.  stats: (layer, p, |C|)"""
    have = [list(r) if int(levels[p]) >= L else [] for p, r in enumerate(lists)]
    out = {}
    for p in range(len(have)):
        if p in gone or int(levels[p]) < L:
            continue
        if not any(x in gone for x in have[p]):
            out[p] = list(have[p])
            continue
        c = rref.candidates(have, gone, p)
        if stats is not None:
            stats.append((L, p, len(c)))
        if len(c) > cap:
            cids, dd = dref.sort_by_base(orc, v, metric, p, c)
            if rule == "diverse":
                c = dref.select_sorted(orc, v, metric, cids, dd, cap, alpha, keep_pruned)
            else:
                c = [int(x) for x in cids[:cap]]
        out[p] = c
    return out


def remove(orc, layers, levels, entry, max_level, v, ids, m, m0, metric=0, rule="reference", alpha=1.0,
           keep_pruned=True, stats=None):
    """The definition.  `layers` has max_level + 1 entries of n lists each."""
    n = len(levels)
    assert len(layers) == max_level + 1 and all(len(layer) == n for layer in layers)
    gone = set(int(i) for i in ids)
    assert all(0 <= i < n for i in gone)
    v = np.ascontiguousarray(v, dtype=np.float32)
    remap, keep = rref.remap_of(n, gone)
    new_entry, new_top = rref.entry_after(levels, keep, remap, entry, int(max_level))
    out = []
    for L in range(new_top + 1 if keep else 0):  # the layers above the new max_level cease to exist
        cap = m0 if L == 0 else m
        fixed = repaired_layer(orc, layers[L], levels, L, v, gone, cap, int(metric), rule, alpha, keep_pruned, stats)
        out.append([[int(remap[y]) for y in fixed[p]] if p in fixed else [] for p in keep])
    return Shrunk(out, [int(levels[p]) for p in keep], new_entry, new_top, remap)


def layers_of_graph(g, n):
    """layers[L][p] of a _hnsw_build_ref.Graph over nodes 0 .. n-1"""
    return [[list(g.row(p, L)) for p in range(n)] for L in range(g.max_level + 1)]


def seed_graph(g, s, v):
    """a _hnsw_build_ref.Graph `g` (its config and rule) made to hold the shrunk graph `s` over the rows `v` of the
    survivors: it can then be searched and grown like one built node by node"""
    g.v = np.ascontiguousarray(v, dtype=np.float32)
    g.conn = {p: [list(s.layers[L][p]) if L < len(s.layers) else [] for L in range(s.levels[p] + 1)]
              for p in range(len(s))}
    g.level = {p: s.levels[p] for p in range(len(s))}
    g.entry, g.max_level = s.entry, s.max_level
    return g
