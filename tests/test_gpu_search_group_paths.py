"""Grouped search launches over every launch shape search_enqueue takes (islands_amd/csrc/search_group.hip, and the
union handling of search.hip): bf16 and fp8 rows, entry seeds, pruning, adjacency rows wider than 64 and than 128
ids, ef above 512, members larger than one step of the gather and scatter kernels, k at the edges of the
`replayed` re-derivation, a member that fails, a workspace that serves several launches, a held set cut at the cap.

One rule everywhere: each member of a shared launch equals the same call made alone through
isl_search_batch_device on an ISL_NO_GROUP=1 index -- ids, distance bits, counts and the nine counters of
_group_case.COUNTERS -- and that call equals the CPU oracle over the rows' exact f32 images (Case.answer_alone,
Case.check; no tolerance anywhere).  Case.shared_round also asserts the group counters that prove the calls shared a
launch: (launches, shared launches, shared calls) move by (1, 0, 0) when the first call goes out alone and the
others are held, and by (1, 1, members) once one of them is waited for -- search_group_plan.hpp: a call that finds
`room` queries in flight is held, a held set below the cap goes out whole when a member is waited for.

The conditions on the inputs alone are tests/test_search_group_paths_inputs_cpu.py; those that need a counter of
the call made alone are asserted here."""
import ctypes as C

import numpy as np
import pytest

import islands_amd as ia
from islands_amd import _ffi
import _group_case as gc
from _group_case import EF, K, Case, counters

pytestmark = pytest.mark.gpu

HELD = dict(ISL_GROUP_ROOM=1, ISL_NO_GROUP=0)  # held whatever the process's hardware queues are


def alone_counters(case, calls, k=K, ef=EF):
    return [case.answer_alone(c, k, ef)[3] for c in calls]


def some_replay_and_some_do_not(alone):
    assert any(s["replayed"] > 0 for s in alone), alone
    assert any(s["replayed"] == 0 and s["exact_path"] == 0 for s in alone), alone


# ------------------------------------------------------------------------------------------------ 1. row types
@pytest.fixture(scope="module", params=[(kind, d) for kind in ("f32", "bf16", "fp8") for d in (32, 50)],
                ids=lambda p: f"{p[0]}-{p[1]}")
def typed(request, orc):
    kind, d = request.param
    return kind, Case(orc, gc.row_types(orc, d, kind))


def test_row_types_share_a_launch(typed):
    """f32, bf16 and fp8 rows: six held calls, one launch.  Over bf16 rows the union's queries are split by kind
    across the members' boundaries (launch_classify), and two fast kernels write the one status / counter array."""
    kind, case = typed
    calls = list(range(len(gc.SIZES)))
    if kind == "bf16":
        mixed = gc.bf16_valued(case.q[gc.MIXED])
        assert mixed.any() and not mixed.all()
        assert gc.bf16_valued(case.q[gc.MIXED - 1])[-1] != mixed[0] and mixed[-1] != gc.bf16_valued(case.q[gc.MIXED + 1])[0]
    some_replay_and_some_do_not(alone_counters(case, calls))
    idx = case.index(**HELD)
    idx.prepare(64, EF, K, 8)
    stats = case.shared_round(idx, calls)
    assert all(s["allocations"] == 0 for s in stats.values()), stats


# ------------------------------------------------------------------------------------------------ 2. entry seeds
@pytest.fixture(scope="module")
def seeded(orc):
    return Case(orc, gc.seeded(orc, 32))


@pytest.mark.parametrize("when", ["before_prepare", "after_prepare"])
def test_entry_seeds_in_a_union(seeded, when):
    """64 seeds: the pick runs over the staged queries of the union; every query is entered at ref.pick's seed.
    Seeds that exist when the index is prepared: the group workspace holds the pick's buffer, nothing is allocated.
    Seeds selected afterwards: the launch may allocate it, the answers are the same."""
    case = seeded
    calls = list(range(len(gc.SIZES)))
    assert len(set(int(e) for c in calls for e in case.entries[c])) > 1  # (the queries do start at different seeds)
    idx = case.index(seeds=when == "before_prepare", **HELD)
    idx.prepare(64, EF, K, 8)
    if when == "after_prepare":
        case.select_seeds(idx)
    stats = case.shared_round(idx, calls, reverse=when == "after_prepare")
    if when == "before_prepare":
        assert all(s["allocations"] == 0 for s in stats.values()), stats


# ------------------------------------------------------------------------------------------------ 3. pruning
@pytest.mark.parametrize("strategy", [0, 1], ids=["Global", "Local"])
def test_pruning_in_a_union(orc, strategy):
    case = Case(orc, gc.pruned(orc, 32, strategy))
    idx = case.index(**HELD)
    idx.prepare(64, EF, K, 8)
    case.shared_round(idx, list(range(len(gc.SIZES))))


# ------------------------------------------------------------------------------------------------ 4. wide rows, exact only
def max_degree(csr):
    return int(np.diff(csr.node_offsets.astype(np.int64)).max())


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_rows_wider_than_64_ids(orc, bf16):
    """Degree 100: the fast kernel's WIDE instantiation over the union; over bf16 rows the bf16-query kernel is off,
    whatever the queries' kind."""
    case = Case(orc, gc.wide(orc, 100, bf16))
    assert 64 < max_degree(case.csr) <= 128
    idx = case.index(**HELD)
    idx.prepare(64, EF, K, 8)
    case.shared_round(idx, list(range(len(gc.WIDE_SIZES))))


def test_rows_wider_than_128_ids_exact_kernel_only(orc):
    """Degree 140: no fast kernel.  The enqueue of the union synchronises its stream half-way, every query is on the
    redo list (81 entries: more than the scatter kernel's scan takes in one step), and exact_path still splits by
    member."""
    case = Case(orc, gc.wide(orc, 140))
    assert max_degree(case.csr) > 128
    calls = list(range(len(gc.WIDE_SIZES)))
    assert sum(gc.WIDE_SIZES) >= 70
    assert [s["exact_path"] for s in alone_counters(case, calls)] == gc.WIDE_SIZES
    idx = case.index(**HELD)
    idx.prepare(64, 256, K, 8)
    stats = case.shared_round(idx, calls)
    assert [stats[c]["exact_path"] for c in calls] == gc.WIDE_SIZES


def test_ef_above_512_exact_kernel_only(orc):
    """ef = 600 on the plain graph: the same branch by way of ef."""
    sizes = [1, 30, 17, 33]
    case = Case(orc, gc.plain(orc, 32, sizes=sizes, tied=[False, True, False, True], seed=640))
    calls = list(range(len(sizes)))
    assert sum(sizes) >= 70
    assert [s["exact_path"] for s in alone_counters(case, calls, K, 600)] == sizes
    idx = case.index(**HELD)
    idx.prepare(64, 600, K, 8)
    stats = case.shared_round(idx, calls, K, 600, reverse=True)
    assert [stats[c]["exact_path"] for c in calls] == sizes


# ------------------------------------------------------------------------------------------------ 5. large members
@pytest.mark.parametrize("d", [128, 50])
def test_large_members_take_further_steps_of_gather_and_scatter(orc, d):
    """Members of 300, 520 and 257 queries: more than the 256 waves a member's scatter blocks have.  d = 128: the
    520-query member is 16640 vectors of four floats, more than one step of the gather kernel's vector path; d = 50:
    its place in the union is 8 bytes past a 16-byte boundary, and its 26000 floats take the scalar path in two
    steps.  The last member's queries start one float past a 16-byte boundary and are a multiple of four floats:
    the scalar path for a misaligned source.  Nothing is allocated after prepare(520, ...)."""
    case = Case(orc, gc.big(orc, d))
    sizes = gc.BIG_SIZES
    offset = sum(sizes[:2])
    assert max(sizes) > 256 and (offset * d * 4) % 16 == (0 if d == 128 else 8)
    assert (sizes[2] * d // 4 > 16384) if d == 128 else (sizes[2] * d > 16384)
    assert case.dq[4].data_ptr() % 16 == 4 and (sizes[4] * d) % 4 == 0
    idx = case.index(**HELD)
    idx.prepare(max(sizes), EF, K, 8)
    stats = case.shared_round(idx, list(range(len(sizes))))
    assert all(s["allocations"] == 0 for s in stats.values()), stats


# ------------------------------------------------------------------------------------------------ 6. k at the edges
@pytest.fixture(scope="module", params=[(m, d) for m in (0, 2) for d in (32, 50)],
                ids=lambda p: f"{'Cosine' if p[0] == 0 else 'DotProduct'}-{p[1]}")
def tied(request, orc):
    metric, d = request.param
    return metric, Case(orc, gc.tied_rows(orc, d, metric))


def test_condition_tied_rows_replay_and_reach_the_exact_kernel(tied):
    """Over all (k, ef): a member that is re-ordered in place and one that is neither re-ordered nor sent to the
    heap-exact kernel; under DotProduct the two members with an all-zero query have it answered by that kernel, and
    they alone (under Cosine nothing of this shape can reach it: _group_case.tied_rows)."""
    metric, case = tied
    for k, ef in gc.K_EDGES:
        alone = alone_counters(case, range(len(gc.TIE_SIZES)), k, ef)
        some_replay_and_some_do_not(alone)
        zero = [sum(1 for c, _ in gc.ZERO_AT if c == m) if metric else 0 for m in range(len(gc.TIE_SIZES))]
        assert [s["exact_path"] for s in alone] == zero, (k, ef, alone)


@pytest.mark.parametrize("k,ef", gc.K_EDGES)
def test_replayed_is_rederived_at_the_edges_of_k(tied, k, ef):
    """k = 1 (no pair inside the prefix), k = 4 and 5 (a pair of copies inside it, or cut by it), k = ef (no entry
    past the prefix: the across-the-boundary branch stays off).  Every counter as alone, `replayed` and `exact_path`
    among them."""
    _, case = tied
    idx = case.index(**HELD)
    idx.prepare(64, EF, 8, 8)
    stats = case.shared_round(idx, list(range(len(gc.TIE_SIZES))), k, ef)
    assert all(s["allocations"] == 0 for s in stats.values()), stats


def test_an_evicted_twin_does_not_count_as_replayed_at_k_equal_ef(orc):
    """(k, ef) = (8, 8) where the push log holds the last result's distance twice and the answer once (the other twin
    was pushed and evicted): nothing lies past the prefix, so no member is re-ordered, alone or in the union."""
    case = Case(orc, gc.evicted_twin(orc))
    calls = list(range(len(gc.EVICTED_SIZES)))
    alone = alone_counters(case, calls, 8, 8)
    assert all(s["replayed"] == 0 and s["exact_path"] == 0 and s["pushes"] == 10 * s["queries"] for s in alone), alone
    idx = case.index(**HELD)
    idx.prepare(64, EF, 8, 8)
    stats = case.shared_round(idx, calls, 8, 8)
    assert all(s["replayed"] == 0 for s in stats.values()), stats


# ------------------------------------------------------------------------------------------------ 7. a failing member
def test_a_failing_member_fails_alone(orc):
    """One query of the second member reaches a row that names an id without a vector: that member's wait raises
    NodeNotFound with the node the call alone and the oracle name; the first and third answer as alone; the next
    round on the same index succeeds."""
    case = Case(orc, gc.failing(orc, 32))
    assert [case.answer_alone(c)[4] for c in range(3)] == [None, gc.BAD_ID, None]
    idx = case.index(**HELD)
    idx.prepare(64, EF, K, 8)
    stats = case.shared_round(idx, [0, 1, 2])
    assert isinstance(stats[1], ia.CoreError) and isinstance(stats[0], dict) and isinstance(stats[2], dict)
    again = case.shared_round(idx, [2, 0])
    assert all(isinstance(s, dict) for s in again.values())
    assert counters(idx) == (4, 2, 5)


# ------------------------------------------------------------------------------------------------ 8. reuse
@pytest.mark.parametrize("d", [32, 50])
def test_a_workspace_serves_round_after_round(orc, d):
    """Three rounds of shared launches on one index, with other members in another order each time (the calls near
    the duplicated rows at other places in the union), and a synchronous search_batch from the same thread between
    the second and the third: what a launch's scatter kernel leaves for the next one -- work-queue heads, its own
    scratch words, stale redo and status words -- and a lane that was a member and then serves a call of its own.
    kernel_ms is the same within a round (Case.shared_round); that it is read anew every round is not asserted:
    two launches may take the same time to the last bit, so an inequality across rounds would fail now and then."""
    case = Case(orc, gc.reuse(orc, d))
    every = sorted(set(c for r in gc.REUSE_ROUNDS for c in r))
    some_replay_and_some_do_not(alone_counters(case, every))
    idx = case.index(**HELD)
    idx.prepare(64, EF, K, 8)
    for n, calls in enumerate(gc.REUSE_ROUNDS):
        if n == 2:
            c = 3
            got = idx.search_batch(case.q[c], K, EF)
            case.check(c, got, idx.last_stats())
        stats = case.shared_round(idx, calls, reverse=n == 1)
        assert all(s["allocations"] == 0 for s in stats.values()), stats
    assert counters(idx) == (6, 3, sum(len(r) for r in gc.REUSE_ROUNDS))


# ------------------------------------------------------------------------------------------------ 9. the cap
def test_a_held_set_is_cut_at_the_cap(orc):
    """ISL_GROUP_CAP=100, four held calls of 40 queries.  search_group_plan.hpp: the third arrival brings the held
    set to 120 >= cap, and it is cut in arrival order: calls 0 and 1 go out as one launch at once.  Calls 2 and 3
    (80 < cap) stay held until one of them is asked for -- here by isl_search_stream_wait, which does not wait on
    the host: both launches are in flight, on two workspaces, before the first wait."""
    case = Case(orc, gc.cap_cut(orc, 32))
    torch = case.torch
    idx = case.index(ISL_GROUP_CAP=100, **HELD)
    idx.prepare(40, EF, K, 8)
    side, reader = torch.cuda.Stream(), torch.cuda.Stream()
    bufs = case.buffers([(c, K) for c in range(4)])
    tok0, keep = case.fill_the_chip(idx, side)
    held = [case.submit(idx, c, bufs[c]) for c in range(4)]
    assert counters(idx) == (2, 1, 2)
    assert _ffi.lib().isl_search_stream_wait(idx._h, held[3][0], C.c_void_p(reader.cuda_stream)) == 0
    assert counters(idx) == (3, 2, 4)
    stats = [idx.wait_stats(held[c][0]) for c in (2, 0, 3, 1)]
    stats = dict(zip((2, 0, 3, 1), stats))
    assert counters(idx) == (3, 2, 4)
    assert idx.wait_stats(tok0)["queries"] == 2
    assert stats[0]["kernel_ms"] == stats[1]["kernel_ms"] and stats[2]["kernel_ms"] == stats[3]["kernel_ms"]
    for c in range(4):
        assert stats[c]["allocations"] == 0, stats[c]
        case.check(c, held[c][2], stats[c])
    del keep
