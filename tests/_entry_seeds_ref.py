"""Entry seeds restated in numpy on top of oracle.batch_distance: the greedy k-centre selection and the
nearest-seed pick exactly as include/islands_amd.h defines them, plus the clustered fixture the tests share.
Nothing here touches the library under test."""
import functools

import numpy as np

N_CLUSTERS, PER_CLUSTER, DIM = 40, 50, 16
METRICS = (0, 1, 2, 3)  # Cosine, Euclidean, DotProduct, Manhattan


def ordkey(d) -> np.ndarray:
    """The search's total order of f32 distances as u32 keys: -0 == +0, NaN greatest."""
    d = np.ascontiguousarray(d, dtype=np.float32)
    u = d.view(np.uint32).copy()
    u[u == 0x80000000] = 0
    neg = (u & 0x80000000) != 0
    key = np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    key[np.isnan(d)] = 0xFFFFFFFF
    return key


def bf16_bits(x) -> np.ndarray:
    """Round-to-nearest-even bf16 bit patterns of finite f32 values."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_image(bits) -> np.ndarray:
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def select(orc, metric: int, x, entry: int, count: int) -> list:
    """seeds[0] = entry; then the row not yet chosen that is farthest from its nearest seed, ties to the
    smaller id; D(seed, row) with the seed as a."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = x.shape[0]
    want = min(count, n)
    if want == 0:
        return []
    seeds = [int(entry)]
    mind = ordkey(orc.batch_distance(metric, x[entry], x))
    chosen = np.zeros(n, dtype=bool)
    chosen[entry] = True
    while len(seeds) < want:
        key = np.where(chosen, np.uint32(0), mind)  # no distance has key 0
        j = int(np.argmax(key))                     # first maximum = smallest id
        seeds.append(j)
        chosen[j] = True
        mind = np.minimum(mind, ordkey(orc.batch_distance(metric, x[j], x)))
    return seeds


def pick_positions(orc, metric: int, queries, x, seeds) -> np.ndarray:
    """Per query the smallest position p minimising D(q, x[seeds[p]]) in ordkey order."""
    rows = np.ascontiguousarray(np.asarray(x, dtype=np.float32)[np.asarray(seeds, dtype=np.int64)])
    queries = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, rows.shape[1])
    return np.array([int(np.argmin(ordkey(orc.batch_distance(metric, q, rows)))) for q in queries], dtype=np.int64)


def pick(orc, metric: int, queries, x, seeds) -> np.ndarray:
    return np.asarray(seeds, dtype=np.uint64)[pick_positions(orc, metric, queries, x, seeds)]


@functools.lru_cache(maxsize=None)
def fixture():
    """(rows [2000, 16], queries [64, 16]): 40 tight clusters of 50 rows in shuffled order, and queries
    next to 64 of the rows.  Read-only arrays, shared by every test."""
    r = np.random.default_rng(1)
    c = r.standard_normal((N_CLUSTERS, DIM)).astype(np.float32)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    x = (c[:, None, :] + np.float32(0.05) * r.standard_normal((N_CLUSTERS, PER_CLUSTER, DIM)).astype(np.float32))
    x = x.reshape(-1, DIM).astype(np.float32)
    x = np.ascontiguousarray(x[r.permutation(N_CLUSTERS * PER_CLUSTER)])
    r7 = np.random.default_rng(7)
    rows = r7.integers(0, N_CLUSTERS * PER_CLUSTER, 64)
    q = (x[rows] + np.float32(0.01) * r7.standard_normal((64, DIM)).astype(np.float32)).astype(np.float32)
    x.setflags(write=False)
    q.setflags(write=False)
    return x, q


_graphs = {}


def knn_csr(orc, metric: int, x, k: int = 8, tag=None):
    """For every row its k exact nearest other rows under the metric (stable argsort of oracle distances),
    entered at node 0.  `tag` caches the graph of a shared, unchanged `x`."""
    if tag is not None and (tag, metric, k) in _graphs:
        return _graphs[(tag, metric, k)]
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = x.shape[0]
    nb = np.zeros((n, k), dtype=np.uint64)
    for i in range(n):
        order = np.argsort(ordkey(orc.batch_distance(metric, x[i], x)), kind="stable")
        nb[i] = order[order != i][:k]
    csr = orc.Csr(np.arange(0, n * k + 1, k, dtype=np.uint64), nb.ravel(), entry_point=0)
    if tag is not None:
        _graphs[(tag, metric, k)] = csr
    return csr


def with_entry(orc, csr, entry: int):
    """The same CSR entered at `entry`."""
    return orc.Csr(csr.node_offsets, csr.neighbors, entry_point=int(entry), levels=csr.levels,
                   degree_counts=csr.degree_counts, max_level=csr.max_level)


def exact_topk(orc, metric: int, q, x, k: int) -> np.ndarray:
    return np.argsort(ordkey(orc.batch_distance(metric, q, x)), kind="stable")[:k]


def recall_at(orc, metric: int, queries, x, found_ids, counts, k: int) -> float:
    hit = 0
    for i, q in enumerate(queries):
        truth = set(exact_topk(orc, metric, q, x, k).tolist())
        hit += len(truth & set(int(v) for v in found_ids[i][:int(counts[i])]))
    return hit / (len(queries) * k)
