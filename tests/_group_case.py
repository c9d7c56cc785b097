"""What the grouped-launch tests share (tests/test_gpu_search_group.py, tests/test_gpu_search_group_paths.py and
the device-free tests/test_search_group_paths_inputs_cpu.py).

A Scenario is everything a test needs to know about one index and the calls made on it: the rows as their exact
f32 images and how they are installed, the LeannConfig, the graph, the entry seeds, one query block per call and
what the CPU oracle is asked with.  Building one touches numpy and the oracle only.  A Case puts a scenario on the
device: an ISL_NO_GROUP=1 index for the calls made alone, the query blocks, the matrix products that keep a first
call in flight, and the comparison every member of a shared launch has to pass."""
import contextlib
import ctypes as C
import dataclasses
import functools
import os
import typing

import numpy as np

import islands_amd as ia
from islands_amd import _ffi
from _data import clustered_vectors, knn_graph, random_csr, uniform_vectors

import _entry_seeds_ref as ref

N, DEG, EF, K = 4000, 16, 32, 5
SIZES = [1, 3, 17, 40, 64, 64]
TIED = [False, True, False, True, False, True]  # which calls ask near the duplicated rows
COUNTERS = ["queries", "expansions", "edges", "evals", "pushes", "exact_path", "replayed", "encoded_nodes",
            "recompute_rounds"]
NODE_NOT_FOUND = 5  # oracle.NODE_NOT_FOUND


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def to_bf16_bits(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def widen(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def bf16_valued(q):
    """Per query: every element is a bf16 value (what the classify kernel sorts a union's queries by)."""
    return (bits(q).reshape(len(q), -1) & 0xFFFF == 0).all(axis=1)


@contextlib.contextmanager
def switches(**env):
    """The group switches are read when an index handle is created."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def counters(idx):
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert _ffi.lib().isl_index_group_counters(idx._h, C.byref(a), C.byref(b), C.byref(c)) == 0
    return int(a.value), int(b.value), int(c.value)


# ------------------------------------------------------------------------------------------------ scenarios
def install_f32(v):
    return lambda idx: idx.set_embeddings(v)


@dataclasses.dataclass
class Scenario:
    v: np.ndarray                 # the rows' exact f32 images: what the oracle searches over
    install: typing.Callable      # idx -> None: set_embeddings / set_embeddings_bf16 / set_embeddings_fp8
    csr: typing.Any               # oracle.Csr
    q: list                       # one query block per call
    extra: np.ndarray             # the call that fills the chip
    cfg: typing.Any = None        # LeannConfig (None: the defaults)
    seeds: int = 0                # entry seeds to select (0: none)
    okw: dict = dataclasses.field(default_factory=dict)  # oracle keywords: metric, prune_ratio, strategy
    fill: tuple = (K, EF)         # (k, ef) of the call that fills the chip
    misaligned: tuple = ()        # calls whose device query pointer lies one float past a 16-byte boundary
    bad_row_of: int = -1          # the node whose adjacency row names an id without a vector (-1: none)

    @property
    def d(self):
        return self.v.shape[1]


@functools.lru_cache(maxsize=None)
def case_rows(d):
    """Half of the rows continuous, the other half quantised to a grid of 1/8 and every one of those stored twice
    (equal distances wherever a query comes near them), in clusters of their own."""
    half, quarter = N // 2, N // 4
    a = clustered_vectors(half, d, 7 + d)
    b = np.round(clustered_vectors(quarter, d, 11 + d) * 8) / 8
    b[np.abs(b).sum(1) == 0, 0] = 0.125
    v = np.concatenate([a, b, b]).astype(np.float32)
    v.setflags(write=False)
    return v


_graphs = {}


def case_graph(orc, v, tag):
    """The kNN graph over `v` (the images the index searches over, so that oracle and index see one graph)."""
    if tag not in _graphs:
        off, nb = knn_graph(v, DEG, seed=3)
        _graphs[tag] = orc.Csr(off, nb, entry_point=0)
    return _graphs[tag]


def member_queries(v, sizes, tied, seed):
    """One block per call near rows of the continuous half, or of the duplicated half where `tied`; and the two
    queries of the call that fills the chip."""
    half, n, d = len(v) // 2, len(v), v.shape[1]
    rng = np.random.default_rng(seed)
    q = []
    for nq, t in zip(sizes, tied):
        rows = rng.integers(half, n, nq) if t else rng.integers(0, half, nq)
        q.append((v[rows] + 0.05 * rng.standard_normal((nq, d))).astype(np.float32))
    extra = (v[:2] + 0.05 * rng.standard_normal((2, d))).astype(np.float32)
    return q, extra


def plain(orc, d, sizes=SIZES, tied=TIED, seed=None, **kw):
    """f32 rows, the kNN graph, no seeds, no pruning."""
    v = case_rows(d)
    q, extra = member_queries(v, sizes, tied, 100 + d if seed is None else seed)
    return Scenario(v, install_f32(v), case_graph(orc, v, ("f32", d)), q, extra, **kw)


def row_types(orc, d, kind):
    """Scenario 1.  The rows stored as f32, bf16 or fp8; the graph rebuilt over each type's images.  Over bf16 rows
    calls 1 and 3 hold bf16-valued queries only, call 2 alternates (its first and last query are not bf16-valued),
    so the kind changes inside a member and at both of its boundaries in the union."""
    v = case_rows(d)
    if kind == "f32":
        images, install = v, install_f32(v)
    elif kind == "bf16":
        b = to_bf16_bits(v)
        images, install = widen(b), lambda idx: idx.set_embeddings_bf16(b)
    else:
        codes, e = ia.quantize_fp8_e4m3(v)
        images, install = ia.fp8_e4m3_to_f32(codes, e), lambda idx: idx.set_embeddings_fp8(codes, e)
    images = np.ascontiguousarray(images, dtype=np.float32)
    q, extra = member_queries(images, SIZES, TIED, 100 + d)
    if kind == "bf16":
        for c in (1, 3):
            q[c] = widen(to_bf16_bits(q[c]))
        q[2][1::2] = widen(to_bf16_bits(q[2][1::2]))
    return Scenario(images, install, case_graph(orc, images, (kind, d)), q, extra)


MIXED = 2  # the call of row_types(.., "bf16") that holds both kinds of query


def seeded(orc, d, count=64):
    """Scenario 2: every query starts at the nearest of `count` selected seeds."""
    sc = plain(orc, d)
    sc.seeds = count
    return sc


def pruned(orc, d, strategy):
    """Scenario 3: prune_ratio 0.4, strategy 0 (Global) or 1 (Local)."""
    cfg = ia.LeannConfig(m=8, m0=16, ef_construction=40, prune_ratio=0.4, pruning_strategy=ia.PruningStrategy(strategy))
    return plain(orc, d, cfg=cfg, okw={"prune_ratio": 0.4, "strategy": int(strategy)})


WIDE_SIZES = [1, 30, 17, 33]  # 81 queries: a redo list of more than one wave's width where every query is on it


def wide(orc, deg, bf16=False):
    """Scenario 4: random adjacency rows of deg/2 .. deg ids over 1500 uniform rows.  deg = 100 is answered by the
    fast kernel's two-ids-per-lane instantiation; deg = 140 by the heap-exact kernel alone, the call that fills the
    chip included.  That call's enqueue waits on the host for the matrix products in front of it, so they cannot keep it
    in flight; it gets 512 queries at ef = 256 instead, some 85 ms in the heap-exact kernel's 32 slots on an MI355X against
    the 0.05 ms four calls take to arrive."""
    n, d = 1500, 32
    v = uniform_vectors(n, d, 60 + deg)
    install = install_f32(v)
    if bf16:
        b = to_bf16_bits(v)
        v, install = widen(b), lambda idx: idx.set_embeddings_bf16(b)
    off, nb = random_csr(n, deg, 61)
    cfg = ia.LeannConfig.accurate() if deg <= 128 else ia.LeannConfig(m=48, m0=deg, ef_construction=400)
    rng = np.random.default_rng(62 + deg)
    q = [(rng.random((nq, d), dtype=np.float32) * 2 - 1).astype(np.float32) for nq in WIDE_SIZES]
    if deg <= 128:
        return Scenario(v, install, orc.Csr(off, nb, entry_point=0), q, q[1][:2].copy(), cfg=cfg)
    extra = (rng.random((512, d), dtype=np.float32) * 2 - 1).astype(np.float32)
    return Scenario(v, install, orc.Csr(off, nb, entry_point=0), q, extra, cfg=cfg, fill=(K, 256))


BIG_SIZES = [300, 1, 520, 257, 8]  # the last one from a misaligned pointer; 8 * d is a multiple of 4


def big(orc, d):
    """Scenario 5: members of more queries than the scatter kernel has waves (256) and of more elements than one
    step of the gather kernel copies (16384 vectors of four at d = 128; at d = 50 the third member's place in the
    union is no multiple of 16 bytes, which sends its 26000 elements down the scalar path)."""
    return plain(orc, d, sizes=BIG_SIZES, tied=[False, True, False, True, False], misaligned=(4,))


TIE_SIZES, TIE_TIED = [1, 3, 17, 40, 2, 9, 64], [True, True, True, True, False, False, False]
K_EDGES = [(1, 32), (4, 32), (5, 32), (8, 8)]


ZERO_AT = [(1, 2), (3, 11)]  # (call, query): all-zero queries of the DotProduct variant


def tied_rows(orc, d, metric=0):
    """Scenario 6: four calls near the duplicated rows and three that are not.  Under Cosine (metric 0) no query of
    this shape can leave the fast kernel: rows of 16 ids, ef <= 32 and a push log of 1024 entries leave a NaN or
    -0.0 distance as the only way to the heap-exact kernel, and 1 - x is never -0.0.  Under DotProduct (metric 2)
    two calls hold an all-zero query each: every distance of such a query is -0.0, and the heap-exact kernel
    answers it."""
    sc = plain(orc, d, sizes=TIE_SIZES, tied=TIE_TIED, seed=400 + d)
    if metric:
        sc.cfg = ia.LeannConfig(m=8, m0=16, ef_construction=40, metric=ia.DistanceMetric(metric))
        sc.okw = {"metric": int(metric)}
        for c, i in ZERO_AT:
            sc.q[c][i] = 0.0
    return sc


EVICTED_SIZES = [3, 5, 2]


def evicted_twin(orc):
    """Scenario 6, k = ef = 8, the case the duplicated rows do not produce by themselves: ten rows in a plane, node 0
    (the entry, farthest from every query) names twins 8 and 9 and then nodes 1..7, each nearer than the twins and
    all at different angles; no other row names anything.  The one hop pushes all nine: the entry and one twin are
    evicted again, the other twin ends as the 8th and last result.  The push log holds that distance twice, the
    answer once, and nothing lies past the prefix: the query was not re-ordered, and must not be counted so."""
    d = 8
    v = np.zeros((10, d), dtype=np.float32)
    angle = [1.4] + [0.1 * i for i in range(1, 8)] + [1.0, 1.0]
    v[:, 0], v[:, 1] = np.cos(angle), np.sin(angle)
    csr = orc.Csr([0] + [9] * 10, [8, 9, 1, 2, 3, 4, 5, 6, 7], entry_point=0)
    rng = np.random.default_rng(88)
    q = []
    for nq in EVICTED_SIZES:
        x = 0.3 * rng.standard_normal((nq, d))
        x[:, 0], x[:, 1] = 1.0, rng.uniform(-0.03, 0.03, nq)
        q.append(x.astype(np.float32))
    return Scenario(v, install_f32(v), csr, q, q[1][:2].copy())


BAD_ID = N + 5          # an id without a vector
FAIL_SIZES = [17, 9, 24]
FAIL_AT = (1, 4)        # (call, query) that asks right at the node whose row names BAD_ID


def failing(orc, d, seed=0):
    """Scenario 7: the kNN graph with BAD_ID in place of the last id of one row, that of a node of the continuous
    half.  Call 1 has one query at that node; calls 0 and 2 ask near the duplicated half, far from it."""
    v = case_rows(d)
    good = case_graph(orc, v, ("f32", d))
    rng = np.random.default_rng(700 + d + seed)
    node = int(rng.integers(1, N // 2))
    nb = good.neighbors.copy()
    nb[int(good.node_offsets[node + 1]) - 1] = BAD_ID
    csr = orc.Csr(good.node_offsets, nb, entry_point=0)
    q, extra = member_queries(v, FAIL_SIZES, [True, True, True], 710 + d + seed)
    q[FAIL_AT[0]][FAIL_AT[1]] = v[node] + np.float32(0.01) * rng.standard_normal(d).astype(np.float32)
    extra = q[0][:2].copy()  # (the call that fills the chip must not fail either)
    return Scenario(v, install_f32(v), csr, q, extra, bad_row_of=node)


REUSE_SIZES = [1, 3, 17, 40, 64, 64, 5, 33]
REUSE_TIED = [False, True, False, True, False, True, True, False]
REUSE_ROUNDS = [[0, 1, 2, 3], [5, 4, 7], [6, 2, 3, 0, 1]]  # tied calls at union offsets 1, 21 / 0 / 0, 22, 63


def reuse(orc, d):
    """Scenario 8: eight calls, drawn on by three rounds of shared launches on one index."""
    return plain(orc, d, sizes=REUSE_SIZES, tied=REUSE_TIED, seed=800 + d)


def cap_cut(orc, d):
    """Scenario 9: four calls of 40 queries."""
    return plain(orc, d, sizes=[40] * 4, tied=[False, True, True, False], seed=900 + d)


def oracle_search(orc, sc, q, k, ef, entry=None):
    g = sc.csr if entry is None else ref.with_entry(orc, sc.csr, entry)
    return orc.leann_search(g, sc.v, q, k, ef, **sc.okw)


# ------------------------------------------------------------------------------------------------ on the device
_busy = []


class Case:
    """A scenario on the device (a bare dimension stands for plain(orc, d)).  One query block per call."""

    def __init__(self, orc, sc):
        import torch

        if not isinstance(sc, Scenario):
            sc = plain(orc, sc)
        self.torch, self.orc, self.sc, self.d = torch, orc, sc, sc.d
        self.v, self.csr, self.q, self.extra = sc.v, sc.csr, sc.q, sc.extra
        if not _busy:
            _busy.append(torch.randn(4096, 4096, device="cuda"))
            (_busy[0] @ _busy[0]).sum().item()  # (the first product loads its library: not inside a test's sequence)
        self.busy = _busy[0]
        self.alone = {}  # (call, k, ef) -> (ids, distance bits, counts, counters, failing node), made once, never changed
        metric = int(sc.okw.get("metric", 0))
        self.seed_ids = ref.select(orc, metric, sc.v, sc.csr.entry_point, sc.seeds) if sc.seeds else []
        self.ref_idx = self.index(ISL_NO_GROUP=1)
        self.entries = [ref.pick(orc, metric, q, sc.v, self.seed_ids) if sc.seeds else [None] * len(q) for q in sc.q]
        # everything a test's sequence of calls reads is on the device beforehand: a copy from the host inside the
        # sequence would wait for the card, and with it for the matrix products that keep the first call in flight
        self.dq = [self.dev(q, c in sc.misaligned) for c, q in enumerate(self.q)]
        self.dextra, self.extra_out = self.dev(self.extra), self.outputs(len(self.extra), sc.fill[0])

    def index(self, seeds=True, **env):
        """An index over the scenario, created under the switches `env`; its entry seeds selected unless not `seeds`."""
        sc = self.sc
        g = ia.CsrGraph(node_offsets=sc.csr.node_offsets, neighbors=sc.csr.neighbors, levels=sc.csr.levels,
                        entry_point=sc.csr.entry_point, max_level=sc.csr.max_level, num_nodes=sc.csr.num_nodes,
                        degree_counts=sc.csr.degree_counts)
        with switches(**env):
            idx = ia.LeannIndex.from_csr(g, sc.cfg, dimension=sc.d)
        idx.upload(0)
        sc.install(idx)
        if seeds and sc.seeds:
            self.select_seeds(idx)
        return idx

    def select_seeds(self, idx):
        assert idx.select_entry_seeds(self.sc.seeds).tolist() == self.seed_ids

    def dev(self, q, misaligned=False):
        t = self.torch
        q = np.ascontiguousarray(q, dtype=np.float32)
        if not misaligned:
            return t.from_numpy(q).cuda()
        whole = t.zeros(q.size + 1, dtype=t.float32, device="cuda")
        part = whole[1:].view(q.shape)
        part.copy_(t.from_numpy(q))
        assert part.data_ptr() % 16 == 4 and q.size % 4 == 0
        return part

    def outputs(self, nq, k):
        t = self.torch
        return (t.full((nq, max(k, 1)), -1, dtype=t.int64, device="cuda"),
                t.full((nq, max(k, 1)), -1.0, dtype=t.float32, device="cuda"), t.full((nq,), -1, dtype=t.int32, device="cuda"))

    def answer_alone(self, call, k=K, ef=EF):
        """The call made by itself through isl_search_batch_device, checked against the oracle: query for query,
        or, where the oracle fails a query, the error of the first one it fails."""
        key = (call, k, ef)
        if key not in self.alone:
            q = self.q[call]
            want = [oracle_search(self.orc, self.sc, q[i], k, ef, self.entries[call][i]) for i in range(len(q))]
            failed = [r for r in want if r.status != 0]
            dq, (ids, dist, cnt) = self.dev(q), self.outputs(len(q), k)
            args = (dq.data_ptr(), len(q), self.d, k, ef, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
            if failed:
                assert failed[0].status == NODE_NOT_FOUND
                try:
                    self.ref_idx.search_batch_device(*args)
                    raise AssertionError(("the call alone did not fail", call))
                except ia.CoreError as e:
                    assert e.kind == "NodeNotFound" and e.node == failed[0].payload, (e.kind, e.node, failed[0].payload)
                self.alone[key] = (None, None, None, None, int(failed[0].payload))
                return self.alone[key]
            self.ref_idx.search_batch_device(*args)
            st = self.ref_idx.last_stats()
            ids, dist, cnt = ids.cpu().numpy(), dist.cpu().numpy(), cnt.cpu().numpy()
            for i, r in enumerate(want):
                m = int(cnt[i])
                assert ids[i, :m].tolist() == r.ids.tolist(), (call, i)
                assert bits(dist[i, :m]).tolist() == bits(r.dist).tolist(), (call, i)
            self.alone[key] = (ids, bits(dist), cnt, {f: st[f] for f in COUNTERS}, None)
        return self.alone[key]

    def fill_the_chip(self, idx, stream):
        """The scenario's first call behind some 50 ms of matrix products on `stream`: in flight until they are done."""
        t = self.torch
        with t.cuda.stream(stream):
            x = self.busy
            for _ in range(64):
                x = (x @ self.busy) * 1e-2
        dq, o, (k, ef) = self.dextra, self.extra_out, self.sc.fill
        tok = idx.search_batch_device_async(dq.data_ptr(), len(self.extra), self.d, k, ef, o[0].data_ptr(), o[1].data_ptr(),
                                            o[2].data_ptr(), stream=stream.cuda_stream)
        return tok, x

    def buffers(self, shapes):
        """Output buffers for calls [(call, k)], made (and the card idle) before the sequence starts."""
        outs = [self.outputs(len(self.q[c]), k) for c, k in shapes]
        self.torch.cuda.synchronize()
        return outs

    def submit(self, idx, call, o, k=K, ef=EF):
        dq = self.dq[call]
        tok = idx.search_batch_device_async(dq.data_ptr(), len(self.q[call]), self.d, k, ef, o[0].data_ptr(), o[1].data_ptr(),
                                            o[2].data_ptr())
        return tok, dq, o

    def check(self, call, o, st, k=K, ef=EF):
        ids, dist, cnt = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in o)
        r_ids, r_bits, r_cnt, r_st, r_node = self.answer_alone(call, k, ef)
        assert r_node is None, (call, r_node)
        assert cnt.tolist() == r_cnt.tolist(), call
        for i in range(len(cnt)):
            m = int(cnt[i])
            assert ids[i, :m].tolist() == r_ids[i, :m].tolist(), (call, i)
            assert bits(dist[i, :m]).tolist() == r_bits[i, :m].tolist(), (call, i)
        if st is not None:
            assert {f: st[f] for f in COUNTERS} == r_st, (call, st, r_st)

    def shared_round(self, idx, calls, k=K, ef=EF, reverse=False):
        """One shared launch: the chip filled from a side stream, `calls` held behind it, all of them waited for
        (in token order, or in reverse) and checked.  The group counters must move by one lone launch for the first
        call, then by one shared launch of len(calls) members: the rules of search_group_plan.hpp for calls of one
        key that arrive while `room` queries are in flight and stay below the cap.  Returns {call: stats}, or the
        CoreError in a call's place where the call alone fails too."""
        base = counters(idx)
        side = self.torch.cuda.Stream()
        bufs = self.buffers([(c, k) for c in calls])
        tok0, keep = self.fill_the_chip(idx, side)
        held = [self.submit(idx, c, o, k, ef) for c, o in zip(calls, bufs)]
        assert counters(idx) == (base[0] + 1, base[1], base[2])  # the first call went out alone, the others are held
        stats = {}
        order = list(range(len(calls)))
        for i in (order[::-1] if reverse else order):
            try:
                stats[i] = idx.wait_stats(held[i][0])
            except ia.CoreError as e:
                stats[i] = e
        assert counters(idx) == (base[0] + 2, base[1] + 1, base[2] + len(calls))
        assert idx.wait_stats(tok0)["queries"] == len(self.extra)
        ok = [s for s in stats.values() if isinstance(s, dict)]
        assert len({s["kernel_ms"] for s in ok}) == 1  # the shared launch's
        out = {}
        for i, c in enumerate(calls):
            node = self.answer_alone(c, k, ef)[4]
            if node is None:
                self.check(c, held[i][2], stats[i], k, ef)
            else:
                assert isinstance(stats[i], ia.CoreError), (c, stats[i])
                assert stats[i].kind == "NodeNotFound" and stats[i].node == node, (c, stats[i].kind, stats[i].node, node)
            out[c] = stats[i]
        del keep
        return out
