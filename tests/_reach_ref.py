"""Graph reachability restated in Python and numpy from the definitions of include/islands_amd.h: the breadth-first
walk, the in-degree count and the cover loop over plain adjacency lists.  Nothing here touches the library under
test: the callers read the lists back (get_neighbors / neighbors(i, layer)) and hand them in."""
import numpy as np

UNREACHED, ABSENT = 0xFFFFFFFF, 0xFFFFFFFE
REPORT_FIELDS = ("nodes", "sources", "reached", "levels", "edges", "dangling_edges", "no_inbound", "max_in_degree")


def distinct(row):
    """list(u) of a LeannIndex: the distinct ids of a row, first occurrence kept."""
    return list(dict.fromkeys(int(v) for v in row))


def lists_from_csr(off, nb):
    off = np.asarray(off, dtype=np.int64)
    nb = np.asarray(nb, dtype=np.uint64)
    return [distinct(nb[off[i]:off[i + 1]]) for i in range(len(off) - 1)]


def reach(lists, sources, member=None):
    """(depth [n] u32, in_degree [n] u32, report dict).  lists[u] = list(u) ([] for a node off the layer);
    member[v] says whether v is in the population (None: every node is)."""
    n = len(lists)
    member = np.ones(n, dtype=bool) if member is None else np.asarray(member, dtype=bool)
    on = lambda v: 0 <= v < n and bool(member[v])
    depth = np.where(member, UNREACHED, ABSENT).astype(np.uint32)
    indeg = np.zeros(n, dtype=np.uint32)
    for u in range(n):
        if member[u]:
            for v in lists[u]:
                if on(v):
                    indeg[v] += 1
    frontier = []
    for s in sources:
        s = int(s)
        assert on(s), s
        if depth[s] == UNREACHED:
            depth[s] = 0
            frontier.append(s)
    n_sources = len(frontier)
    edges = dangling = levels = 0
    while frontier:
        levels += 1
        nxt = []
        for u in frontier:
            for v in lists[u]:
                if not on(v):
                    dangling += 1
                    continue
                edges += 1
                if depth[v] == UNREACHED:
                    depth[v] = levels
                    nxt.append(v)
        frontier = nxt
    pop = int(member.sum())
    report = dict(nodes=pop, sources=n_sources, reached=int((depth < ABSENT).sum()), levels=levels, edges=edges,
                  dangling_edges=dangling, no_inbound=int((indeg[member] == 0).sum()),
                  max_in_degree=int(indeg[member].max()) if pop else 0)
    return depth, indeg, report


def reachable(lists, sources):
    return reach(lists, sources)[0] != UNREACHED


def cover(lists, start, max_seeds):
    """The loop of isl_index_cover_entry_seeds: (S after the loop, ids added, rows S does not reach)."""
    n = len(lists)
    seeds = [int(s) for s in start]
    r = reachable(lists, seeds)
    added = 0
    while not r.all() and len(seeds) < max_seeds:
        j = int(np.argmin(r))  # the smallest id not in R
        seeds.append(j)
        added += 1
        r |= reachable(lists, [j])
    return seeds, added, int(n - r.sum())
