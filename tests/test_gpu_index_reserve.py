"""isl_index_reserve on the device: a LeannIndex whose row table has a capacity.  Inserts append into it, removals
compact it in place, and no call on a reserved index allocates a second row block (`capacity["row_allocations"]`).
Every case takes a reserved index and a twin nobody reserved through the same calls and asks for the same bytes,
row bits, stored type, entry seeds and search answers; one insert and one remove case are also checked against the
definitions (the oracle's build over all rows, tests/_remove_ref.py), so that the reserved path does not lean on
the twin's alone.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import islands_amd as ia
from _data import clustered_vectors, random_levels, uniform_vectors
from test_gpu_build_bf16 import reference_bytes, to_bf16_bits, widen
from test_gpu_index_insert import bits
from test_gpu_index_remove import csr_of, remove_and_check
from test_row_compact_plan_cpu import removals

pytestmark = pytest.mark.gpu

N0, CAP, K, EF = 300, 512, 10, 48
RULES = ["reference", "diverse"]
DTYPES = ["f32", "bf16"]

_built = {}


@pytest.fixture(scope="module", autouse=True)
def shared_builds():
    """the starting graphs are built once and shared among the tests; they go when the module is done"""
    yield
    _built.clear()


def cfg_of(metric=ia.DistanceMetric.Cosine):
    return ia.LeannConfig(m=8, m0=16, ef_construction=40, metric=metric)


def rows_of(d, dtype, n=CAP + 40):
    """n rows as the index takes them (f32, or bf16 bit patterns) and their levels"""
    v = uniform_vectors(n, d, 70 + d) if d == 3 else clustered_vectors(n, d, 70 + d)
    return (to_bf16_bits(v) if dtype == "bf16" else v), random_levels(n, 8, 3)


def attach(idx, rows, dtype):
    return idx.set_embeddings_bf16(rows) if dtype == "bf16" else idx.set_embeddings(rows)


def insert(idx, rows, dtype, **kw):
    return idx.insert_bf16(rows, **kw) if dtype == "bf16" else idx.insert(rows, **kw)


def start(d, dtype, rule, n0=N0):
    """an index of the first n0 rows, built on the device once per key and made from its bytes afterwards"""
    rows, lv = rows_of(d, dtype)
    key = (d, dtype, rule, n0)
    if key not in _built:
        build = ia.LeannIndex.build_bf16 if dtype == "bf16" else ia.LeannIndex.build
        _built[key] = build(rows[:n0], cfg_of(), levels=lv[:n0], batch=1, select=rule).to_bytes()
    idx = ia.LeannIndex.from_bytes(_built[key]).upload(0)
    attach(idx, rows[:n0], dtype)
    return idx


def pair(d, dtype, rule, capacity=CAP):
    """(reserved, twin, allocations of each so far)"""
    r, t = start(d, dtype, rule), start(d, dtype, rule)
    assert r.capacity == t.capacity == {"rows": N0, "row_allocations": 1}
    before = r.row_storage()
    r.reserve(capacity)
    assert r.capacity == {"rows": capacity, "row_allocations": 2}
    es = 2 if dtype == "bf16" else 4
    stride = -(-d // (16 // es)) * (16 // es)
    assert r.row_storage() == dict(before, block_bytes=(capacity * stride) * es + 1024)
    assert t.row_storage()["block_bytes"] == N0 * stride * es + 1024
    return r, t


def state(idx, q):
    """everything the issue compares; a search that fails (an emptied index) is recorded by the kind of its error"""
    try:
        ids, dist, cnt = idx.search_batch(q, K, EF)
        # (what lies behind a query's count is not part of its answer)
        answers = ([ids[i, :c].tolist() for i, c in enumerate(cnt)], [bits(dist[i, :c]).tolist() for i, c in enumerate(cnt)],
                   cnt.tolist())
    except ia.CoreError as e:
        answers = e.kind
    rows = idx.read_rows().tobytes() if len(idx) else b""
    return (idx.to_bytes(), len(idx), rows, idx.row_storage()["dtype"], idx.row_storage()["scale_exp"],
            idx.entry_seeds().tolist(), answers)


def queries(d):
    return uniform_vectors(16, d, 9) if d == 3 else clustered_vectors(16, d, 9)


def same(r, t, d):
    q = queries(d)
    a, b = state(r, q), state(t, q)
    for x, y, what in zip(a, b, ("bytes", "len", "row bits", "dtype", "scale_exp", "entry seeds", "answers")):
        assert x == y, what


# ---------------------------------------------------------------- the reservation itself
def test_a_reserved_index_answers_as_its_twin():
    """capacity 4096 over 300 rows: whole-tile reads past the last row land in the zeroed reserve"""
    for dtype in DTYPES:
        r, t = pair(24, dtype, "reference", 4096)
        same(r, t, 24)
        assert r.capacity["rows"] == 4096
        r.reserve(512)  # a reservation never shrinks; nothing is touched
        r.reserve(4096)
        r.reserve(0)
        assert r.capacity == {"rows": 4096, "row_allocations": 2}
        same(r, t, 24)
        with pytest.raises(ia.CoreError) as e:
            r.reserve(8192, d=12)
        assert e.value.kind == "DimensionMismatch" and (e.value.expected, e.value.actual) == (24, 12)
        with pytest.raises(ia.CoreError) as e:
            r.reserve(8192, dtype="fp8" if dtype == "f32" else "f32")
        assert e.value.kind == "Unsupported"
        assert r.capacity == {"rows": 4096, "row_allocations": 2}
        r.reserve(100)  # below len: treated as len
        same(r, t, 24)


# ---------------------------------------------------------------- insert
@pytest.mark.parametrize("count", [1, 50, CAP - N0])
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("d", [3, 24, 100])
@pytest.mark.parametrize("dtype", DTYPES)
def test_insert_appends_in_place(dtype, d, rule, count):
    rows, lv = rows_of(d, dtype)
    r, t = pair(d, dtype, rule)
    new, nlv = rows[N0:N0 + count], lv[N0:N0 + count]
    assert insert(r, new, dtype, levels=nlv, select=rule) == N0
    assert insert(t, new, dtype, levels=nlv, select=rule) == N0
    assert r.capacity == {"rows": CAP, "row_allocations": 2}  # no second block
    assert t.capacity == {"rows": N0 + count, "row_allocations": 2}  # the twin's new table
    assert len(r) == N0 + count
    same(r, t, d)


def test_insert_is_the_oracles_build(orc):
    """the reserved path against the definition: the oracle's build over all rows, reference rule"""
    for dtype in DTYPES:
        rows, lv = rows_of(24, dtype)
        r, _ = pair(24, dtype, "reference")
        insert(r, rows[N0:N0 + 1], dtype, levels=lv[N0:N0 + 1])
        insert(r, rows[N0 + 1:CAP], dtype, levels=lv[N0 + 1:CAP])
        images = widen(rows[:CAP]) if dtype == "bf16" else rows[:CAP]
        want, _ = reference_bytes(orc, images, cfg_of(), lv[:CAP])
        assert r.to_bytes() == want and r.capacity == {"rows": CAP, "row_allocations": 2}
        assert r.read_rows().tobytes() == rows[:CAP].tobytes()


def test_insert_of_device_resident_rows():
    torch = pytest.importorskip("torch")
    for dtype in DTYPES:
        rows, lv = rows_of(24, dtype)
        r, t = pair(24, dtype, "diverse")
        new = rows[N0:N0 + 50]
        dev = torch.from_numpy(new.view(np.int16) if dtype == "bf16" else new).to("cuda:0")
        torch.cuda.synchronize()
        assert insert(r, dev, dtype, levels=lv[N0:N0 + 50], select="diverse") == N0
        del dev  # the index keeps its own copy of the rows
        insert(t, new, dtype, levels=lv[N0:N0 + 50], select="diverse")
        assert r.capacity == {"rows": CAP, "row_allocations": 2}
        same(r, t, 24)


@pytest.mark.parametrize("dtype", DTYPES)
def test_insert_past_the_capacity_uses_the_reservation_up(dtype):
    rows, lv = rows_of(24, dtype)
    r, t = pair(24, dtype, "reference")
    count = CAP - N0 + 1  # 213 rows into 300 of 512
    insert(r, rows[N0:N0 + count], dtype, levels=lv[N0:N0 + count])
    insert(t, rows[N0:N0 + count], dtype, levels=lv[N0:N0 + count])
    assert r.capacity == {"rows": N0 + count, "row_allocations": 3} and len(r) == N0 + count
    same(r, t, 24)
    insert(r, rows[N0 + count:N0 + count + 5], dtype)  # and an index nobody reserved from here on
    assert r.capacity == {"rows": N0 + count + 5, "row_allocations": 4}


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_handle_reserve_then_insert_is_a_build(dtype, rule):
    d = 24
    rows, lv = rows_of(d, dtype)
    idx = ia.LeannIndex(cfg_of())
    assert idx.capacity == {"rows": 0, "row_allocations": 0}
    idx.reserve(CAP, d, dtype)
    assert idx.capacity == {"rows": CAP, "row_allocations": 1} and len(idx) == 0
    with pytest.raises(ia.CoreError) as e:  # the reservation fixed d and dtype of the rows to come
        insert(idx, rows_of(12, dtype)[0][:4], dtype)
    assert e.value.kind == "DimensionMismatch" and (e.value.expected, e.value.actual) == (d, 12)
    other = "f32" if dtype == "bf16" else "bf16"
    with pytest.raises(ia.CoreError) as e:
        insert(idx, rows_of(d, other)[0][:4], other)
    assert e.value.kind == "Unsupported"
    assert insert(idx, rows[:N0], dtype, levels=lv[:N0], select=rule) == 0
    assert idx.capacity == {"rows": CAP, "row_allocations": 1}  # one table, ever
    build = ia.LeannIndex.build_bf16 if dtype == "bf16" else ia.LeannIndex.build
    built = build(rows[:N0], cfg_of(), levels=lv[:N0], batch=1, select=rule)
    assert idx.to_bytes() == built.to_bytes()
    same(idx, built, d)


# ---------------------------------------------------------------- remove
SEEDS = [0, 1, 150, 120, 299, 77]


@pytest.mark.parametrize("stage", [None, "1", "7", "64"])
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(removals()))
def test_remove_compacts_in_place(monkeypatch, name, dtype, rule, stage):
    if stage is None:
        monkeypatch.delenv("ISL_COMPACT_STAGE_ROWS", raising=False)
    else:
        monkeypatch.setenv("ISL_COMPACT_STAGE_ROWS", stage)
    d = 24
    rows, lv = rows_of(d, dtype)
    ids = removals(N0)[name]
    r, t = pair(d, dtype, rule)
    r.set_entry_seeds(SEEDS)
    t.set_entry_seeds(SEEDS)
    assert r.remove(ids, select=rule).tolist() == t.remove(ids, select=rule).tolist()
    assert r.capacity == {"rows": CAP, "row_allocations": 2}  # the same block, the same capacity
    assert len(r) == N0 - len(ids)
    same(r, t, d)
    gone = set(ids)
    assert len(r.entry_seeds()) == len([s for s in SEEDS if s not in gone])
    # the freed room takes rows again
    new, nlv = rows[N0:N0 + 20], lv[N0:N0 + 20]
    assert insert(r, new, dtype, levels=nlv, select=rule) == insert(t, new, dtype, levels=nlv, select=rule)
    assert r.capacity == {"rows": CAP, "row_allocations": 2}
    same(r, t, d)


@pytest.mark.parametrize("stage", ["7", None])
def test_remove_is_the_definition(orc, monkeypatch, stage):
    """the reserved path against the definition: tests/_remove_ref.py over the graph the handle held"""
    if stage is None:
        monkeypatch.delenv("ISL_COMPACT_STAGE_ROWS", raising=False)
    else:
        monkeypatch.setenv("ISL_COMPACT_STAGE_ROWS", stage)
    rows, lv = rows_of(24, "f32")
    r, _ = pair(24, "f32", "reference")
    csr = csr_of(orc, r, lv[:N0])
    ids = np.random.default_rng(5).choice(N0, 90, replace=False).astype(np.uint64)
    remove_and_check(orc, r, csr, rows[:N0], ids, cfg_of())
    assert r.capacity == {"rows": CAP, "row_allocations": 2}
    assert r.read_rows().tobytes() == np.delete(rows[:N0], ids.astype(np.int64), axis=0).tobytes()


# ---------------------------------------------------------------- sequences
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_come_and_go(dtype):
    d = 24
    rows, lv = rows_of(d, dtype, 1200)
    r, t = pair(d, dtype, "diverse")
    rng = np.random.default_rng(11)
    at = N0
    for _ in range(10):
        for count, out in ((40, 25), (1, 1)):
            new, nlv = rows[at:at + count], lv[at:at + count]
            at += count
            assert (insert(r, new, dtype, levels=nlv, select="diverse")
                    == insert(t, new, dtype, levels=nlv, select="diverse"))
            same(r, t, d)
            ids = rng.choice(len(r), out, replace=False)
            assert r.remove(ids, select="diverse").tolist() == t.remove(ids, select="diverse").tolist()
            same(r, t, d)
    assert len(r) == N0 + 10 * 15 and r.capacity == {"rows": CAP, "row_allocations": 2}


# ---------------------------------------------------------------- conversions
def test_conversions_keep_the_capacity():
    d = 24
    rows, lv = rows_of(d, "f32")
    r, t = pair(d, "f32", "reference")
    allocs = 2
    for target in ("bf16", "f32"):
        r.convert_rows(target)
        t.convert_rows(target)
        allocs += 1
        assert r.capacity == {"rows": CAP, "row_allocations": allocs} and t.capacity["rows"] == N0
        same(r, t, d)
    # widen, insert, narrow keeps its reservation
    new = widen(to_bf16_bits(rows[N0:N0 + 10]))
    r.insert(new, levels=lv[N0:N0 + 10])
    t.insert(new, levels=lv[N0:N0 + 10])
    assert r.capacity == {"rows": CAP, "row_allocations": allocs}
    r.convert_rows("fp8")
    t.convert_rows("fp8")
    assert r.capacity == {"rows": CAP, "row_allocations": allocs + 1}
    assert r.row_storage()["block_bytes"] == CAP * 32 + 1024 and t.row_storage()["block_bytes"] == (N0 + 10) * 32 + 1024
    same(r, t, d)
    r.reserve(CAP + 88)  # fp8 rows are reserved like any other
    assert r.capacity == {"rows": CAP + 88, "row_allocations": allocs + 2}
    same(r, t, d)
    # set_embeddings replaces the table: the reservation goes with it
    r.set_embeddings(rows[:N0 + 10])
    t.set_embeddings(rows[:N0 + 10])
    assert r.capacity == {"rows": N0 + 10, "row_allocations": allocs + 3}
    same(r, t, d)


# ---------------------------------------------------------------- refusals that need a device
def busy_case(orc):
    import torch
    from test_gpu_lanes import _case
    from test_gpu_parity import make_index

    v, csr = _case(orc, n=2500, seed=50)
    idx = make_index(csr, v)
    idx.prepare(256, 64, 10, 2)
    q = clustered_vectors(256, v.shape[1], 51)
    out = (torch.zeros((256, 10), dtype=torch.int64, device="cuda"),
           torch.zeros((256, 10), dtype=torch.float32, device="cuda"),
           torch.zeros(256, dtype=torch.int32, device="cuda"))
    dq = torch.from_numpy(q).cuda()
    torch.cuda.synchronize()

    def launch():
        return idx.search_batch_device_async(dq.data_ptr(), 256, v.shape[1], 10, 64, out[0].data_ptr(),
                                             out[1].data_ptr(), out[2].data_ptr())

    return idx, v, q, launch


def test_a_busy_lane_refuses_reserve_and_reserved_remove(orc):
    pytest.importorskip("torch")
    idx, v, q, launch = busy_case(orc)
    want = idx.search_batch(q[:16], K, EF)
    before = idx.to_bytes(), idx.read_rows().tobytes(), idx.capacity

    def unchanged():
        got = idx.search_batch(q[:16], K, EF)
        assert (idx.to_bytes(), idx.read_rows().tobytes(), idx.capacity) == before
        assert got[0].tolist() == want[0].tolist() and bits(got[1]).tolist() == bits(want[1]).tolist()

    tok = launch()
    with pytest.raises(ia.CoreError) as e:
        idx.reserve(4096)
    assert e.value.kind == "SearchError"
    idx.wait(tok)
    unchanged()
    idx.reserve(4096)  # fine once nothing is in flight
    before = idx.to_bytes(), idx.read_rows().tobytes(), idx.capacity
    assert before[2] == {"rows": 4096, "row_allocations": 2}
    tok = launch()
    with pytest.raises(ia.CoreError) as e:
        idx.remove([3, 1000, 2499])
    assert e.value.kind == "SearchError"
    idx.wait(tok)
    unchanged()  # nothing moved


def test_the_core_of_an_hnsw_graph_is_refused():
    g = ia.HnswGraph.build(uniform_vectors(60, 8, 3), m=4, m0=8, ef_construction=16)
    blob = g.to_bytes()
    core = C.c_void_p.from_address(g._h.value)  # isl_hnsw's first member: the layer-0 isl_index
    lib = ia._ffi.lib()
    assert lib.isl_status_name(lib.isl_index_reserve(core, 512, 8, 0)) == b"Unsupported"
    assert "HnswGraph" in lib.isl_last_error_message().decode()
    assert g.to_bytes() == blob and len(g) == 60


def test_a_recompute_index_is_refused(orc):
    from test_gpu_encoder import _recompute_case
    _, enc, tok, lens, emb = _recompute_case(orc, n=64)
    n, d = emb.shape
    ring = ia.CsrGraph(node_offsets=np.arange(n + 1, dtype=np.uint64),
                       neighbors=(np.arange(n, dtype=np.uint64) + 1) % n, levels=np.zeros(n, np.uint64),
                       entry_point=0, num_nodes=n, degree_counts=np.ones(n, np.uint64))
    idx = ia.LeannIndex.from_csr(ring, cfg_of(), dimension=d).upload(0)
    idx.set_recompute_provider(enc, tok, lens)
    blob = idx.to_bytes()
    lib = ia._ffi.lib()
    assert lib.isl_status_name(lib.isl_index_reserve(idx._h, 512, d, 0)) == b"Unsupported"
    assert "recompute" in lib.isl_last_error_message().decode()
    assert idx.to_bytes() == blob and len(idx) == n and idx.capacity["rows"] == 0
