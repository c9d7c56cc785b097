"""Breadth-first walks on the host over lists read back one node per ctypes call: what HnswGraph.reachability and
LeannIndex.reachability replace.  Kept as a cross-check at sizes where it takes seconds, and as the yardstick of
tools/graph_reach_perf.py."""
import ctypes as C

import numpy as np

import islands_amd as ia


def _walk(n, off, adj, entry):
    """nodes a walk from `entry` does not meet; one level per turn, the lists of the frontier gathered at once"""
    seen = np.zeros(n, dtype=bool)
    front = np.array([entry], dtype=np.int64)
    seen[front] = True
    while front.size:
        lens = off[front + 1] - off[front]
        at = np.repeat(off[front] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(lens.sum())
        nxt = np.unique(adj[at])
        nxt = nxt[nxt < n]  # an id that names no node is not followed
        front = nxt[~seen[nxt]]
        seen[front] = True
    return int((~seen).sum())


def hnsw_unreachable(g, width=32):
    """nodes of an HnswGraph a walk over layer 0 from the entry point does not meet (lists of up to `width` ids)"""
    n = len(g)
    if not n:
        return 0
    fn, buf, cnt = ia._ffi.lib().isl_hnsw_get_neighbors, np.zeros(129, dtype=np.uint64), C.c_uint64()
    ptr, pc = C.c_void_p(buf.ctypes.data), C.byref(cnt)
    off, adj = np.zeros(n + 1, dtype=np.int64), np.zeros(n * width, dtype=np.int64)
    for i in range(n):
        fn(g._h, i, 0, ptr, 129, pc, None)
        off[i + 1] = off[i] + cnt.value
        adj[off[i]:off[i + 1]] = buf[:cnt.value]
    return _walk(n, off, adj, g.entry_point)


def index_unreachable(idx):
    """the same over the host copy of a LeannIndex's CSR (isl_index_get_neighbors, one node per call)"""
    n = len(idx)
    if not n:
        return 0
    fn, ptr, cnt = ia._ffi.lib().isl_index_get_neighbors, C.POINTER(C.c_uint64)(), C.c_size_t()
    pp, pc = C.byref(ptr), C.byref(cnt)
    off, rows = np.zeros(n + 1, dtype=np.int64), []
    for i in range(n):
        fn(idx._h, i, pp, pc)
        off[i + 1] = off[i] + cnt.value
        rows.append(np.ctypeslib.as_array(ptr, shape=(cnt.value,)).astype(np.int64) if cnt.value else np.zeros(0, np.int64))
    return _walk(n, off, np.concatenate(rows) if rows else np.zeros(0, np.int64), idx.entry_point)
