"""HnswGraph::insert (hnsw.rs:214-329) restated in Python, as the tests' definition of isl_hnsw_build:
every distance goes through the oracle's f32 chain, the heaps are Rust's BinaryHeap (`_pyref.RustHeap`)
ordered on the distance alone, every sort is stable.

rule "reference": the reference as written -- the new node takes the first M_L search results, is appended
to each of them that has the layer, and a list longer than M_L is replaced by its entries OTHER THAN THE NEW
ID (prune_connections cannot see the node being inserted), stable-sorted by distance from the owner.
rule "diverse": select() of `_diverse_ref` for the new node's list and for a list that reaches M_L + 1 ids,
the new node taking part.

`build` inserts one node at a time; `build_batched` follows the step semantics of the batched mode: the
planner below, every selection of a step made on the graph as of the step's start (layer by layer, the
links of layer L applied after the layer-L searches), back links applied in id order (one legal order)."""
import numpy as np

from _diverse_ref import select_sorted, sort_by_base
from _pyref import RustHeap


class Graph:
    def __init__(self, orc, v, m, m0, ef_construction, metric, rule="reference", alpha=1.0, keep_pruned=True):
        self.orc, self.v = orc, np.ascontiguousarray(v, dtype=np.float32)
        self.m, self.m0, self.efc, self.metric = m, m0, ef_construction, int(metric)
        self.rule, self.alpha, self.keep_pruned = rule, alpha, keep_pruned
        self.conn, self.level, self.entry, self.max_level = {}, {}, None, 0

    def dist(self, q, ids):
        return self.orc.batch_distance(self.metric, q, self.v[np.asarray(ids, dtype=np.int64)])

    def cap(self, layer):
        return self.m0 if layer == 0 else self.m

    def row(self, node, layer):
        """neighbors_at(layer): None (here: empty) above the node's level"""
        return self.conn[node][layer] if node in self.conn and layer <= self.level[node] else []

    def search_layer(self, q, entry, ef, layer):  # hnsw.rs:332-402
        visited = {entry}
        cand = RustHeap(lambda t: -float(t[0]))
        res = RustHeap(lambda t: float(t[0]))
        ed = self.dist(q, [entry])[0]
        cand.push((ed, entry))
        res.push((ed, entry))
        while True:
            cur = cand.pop()
            if cur is None:
                break
            d, cid = cur
            if res.data and d > res.data[0][0] and len(res.data) >= ef:
                break
            new = []
            for x in self.row(cid, layer):
                if x not in visited:
                    visited.add(x)
                    new.append(x)
            if not new:
                continue
            for x, nd in zip(new, self.dist(q, new)):
                if len(res.data) < ef or nd < res.data[0][0]:
                    cand.push((nd, x))
                    res.push((nd, x))
                    if len(res.data) > ef:
                        res.pop()
        out = list(res.data)
        out.sort(key=lambda t: float(t[0]))
        return [int(t[1]) for t in out], [t[0] for t in out]

    def greedy(self, q, layer, cur, cd):  # hnsw.rs:263-282: the round's list is the round-start node's
        while True:
            changed = False
            nbs = list(self.row(cur, layer))
            if nbs:
                for x, d in zip(nbs, self.dist(q, nbs)):
                    if d < cd:
                        cur, cd, changed = x, d, True
            if not changed:
                return cur, cd

    def select(self, ids, dd, layer):
        M = self.cap(layer)
        if self.rule == "reference":
            return list(ids[:M])
        return select_sorted(self.orc, self.v, self.metric, ids, dd, M, self.alpha, self.keep_pruned)

    def link(self, i, layer, sel):
        """the new node's list and the back links of one layer, hnsw.rs:295-313"""
        M = self.cap(layer)
        self.pending[i][layer] = list(sel)
        for nb in sel:
            if nb in self.level and layer <= self.level[nb]:
                row = self.conn[nb][layer]
                row.append(i)
                if len(row) > M:
                    if self.rule == "reference":
                        c, _ = sort_by_base(self.orc, self.v, self.metric, nb, [x for x in row if x != i])
                        self.conn[nb][layer] = [int(x) for x in c][:M]
                    else:
                        c, d2 = sort_by_base(self.orc, self.v, self.metric, nb, row)
                        self.conn[nb][layer] = select_sorted(self.orc, self.v, self.metric, c, d2, M, self.alpha,
                                                             self.keep_pruned)

    def insert_step(self, ids, levels):
        """the nodes `ids` as one step: descents, then per layer search + select for all, then links"""
        if self.entry is None:
            (i,) = ids
            self.entry, self.max_level = i, int(levels[i])
            self.conn[i], self.level[i] = [[] for _ in range(int(levels[i]) + 1)], int(levels[i])
            return
        self.pending = {i: [[] for _ in range(int(levels[i]) + 1)] for i in ids}
        cur = {}
        for i in ids:
            c = self.entry
            cd = self.dist(self.v[i], [c])[0]
            for layer in range(self.max_level, int(levels[i]), -1):
                c, cd = self.greedy(self.v[i], layer, c, cd)
            cur[i] = c
        top = max(int(levels[i]) for i in ids)
        for layer in range(top, -1, -1):
            act = [i for i in ids if int(levels[i]) >= layer]
            sels = {}
            for i in act:
                found, dd = self.search_layer(self.v[i], cur[i], self.efc, layer)
                sels[i] = self.select(found, dd, layer)
            for i in act:
                self.link(i, layer, sels[i])
                if sels[i]:
                    cur[i] = sels[i][0]
        for i in ids:
            self.conn[i], self.level[i] = self.pending[i], int(levels[i])
        if top > self.max_level:  # (such a node is alone in its step)
            self.max_level, self.entry = top, ids[0]

    def layers(self):
        n = len(self.conn)
        return [[list(self.row(i, L)) for i in range(n)] for L in range(self.max_level + 1)]

    def search(self, q, k, ef):  # hnsw.rs:458-504
        cur = self.entry
        cd = self.dist(q, [cur])[0]
        for layer in range(self.max_level, 0, -1):
            cur, cd = self.greedy(q, layer, cur, cd)
        ids, dd = self.search_layer(q, cur, max(ef, k), 0)
        return ids[:k], dd[:k]


def plan_steps(levels, batch):
    """[(first id, count)]: min(batch, n - id0, max(1, id0 / 8)) nodes per step, cut so that a node above
    the current top layer is the only node of its step.  Node 0 is a step of its own."""
    n = len(levels)
    steps = [(0, 1)] if n else []
    max_level = int(levels[0]) if n else 0
    id0 = 1
    while id0 < n:
        nb = min(batch, n - id0, max(1, id0 // 8))
        if int(levels[id0]) > max_level:
            nb = 1
        else:
            for j in range(1, nb):
                if int(levels[id0 + j]) > max_level:
                    nb = j
                    break
        steps.append((id0, nb))
        max_level = max(max_level, max(int(x) for x in levels[id0:id0 + nb]))
        id0 += nb
    return steps


def build_batched(orc, v, levels, m, m0, ef_construction, metric, rule="reference", batch=1, alpha=1.0,
                  keep_pruned=True):
    g = Graph(orc, v, m, m0, ef_construction, metric, rule, alpha, keep_pruned)
    for id0, nb in plan_steps(levels, batch):
        g.insert_step(list(range(id0, id0 + nb)), levels)
    return g


def build(orc, v, levels, m, m0, ef_construction, metric, rule="reference", alpha=1.0, keep_pruned=True):
    return build_batched(orc, v, levels, m, m0, ef_construction, metric, rule, 1, alpha, keep_pruned)


def no_inbound(layer0):
    """nodes that no layer-0 list names"""
    seen = np.zeros(len(layer0), dtype=bool)
    for row in layer0:
        for x in row:
            seen[int(x)] = True
    return int((~seen).sum())
