"""Grouped search launches (islands_amd/csrc/search_group.hip): asynchronous device-pointer calls that find the chip
full are held and go out together as one launch.  Every call must still get exactly what it gets alone: ids,
distance bits, counts and all counters of isl_search_stats, equal to the same call made by itself through
isl_search_batch_device and to the CPU oracle.

ISL_GROUP_ROOM=1 makes "the chip is full" hold as soon as one query is in flight, and a first call of two queries
ordered behind a few milliseconds of matrix products on the caller's stream keeps it so while the others arrive."""
import ctypes as C

import numpy as np
import pytest

import islands_amd as ia
from islands_amd import _ffi
from _group_case import EF, K, SIZES, Case, counters, switches
from test_gpu_parity import make_index

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[32, 50])
def case(request, orc):
    return Case(orc, request.param)


def test_condition_some_members_tie_and_some_do_not(case):
    """(b) what makes the comparison of the per-call counters mean something: alone, at least one of the calls has
    queries re-ordered or answered by the heap-exact kernel, and another has none."""
    alone = [case.answer_alone(c)[3] for c in range(len(SIZES))]
    assert any(s["replayed"] > 0 or s["exact_path"] > 0 for s in alone), alone
    assert any(s["replayed"] == 0 and s["exact_path"] == 0 for s in alone), alone


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_held_calls_share_one_launch_and_answer_as_alone(case, order):
    """(a), (d), (f): six held calls, one launch; per call the answers and every counter of the call made alone;
    waited for in token order and in reverse; no allocation after isl_index_prepare."""
    torch = case.torch
    with switches(ISL_GROUP_ROOM=1, ISL_NO_GROUP=0):  # (held whatever the process's hardware queues are)
        idx = make_index(case.csr, case.v)
    idx.prepare(64, EF, K, 8)
    side = torch.cuda.Stream()
    bufs = case.buffers([(c, K) for c in range(len(SIZES))])
    tok0, keep = case.fill_the_chip(idx, side)
    calls = [case.submit(idx, c, bufs[c]) for c in range(len(SIZES))]
    assert counters(idx) == (1, 0, 0)  # the first call went out alone, the six are held
    seq = list(range(len(SIZES)))
    stats = {}
    for c in (seq if order == "forward" else seq[::-1]):
        stats[c] = idx.wait_stats(calls[c][0])
    assert counters(idx) == (2, 1, 6)
    assert idx.wait_stats(tok0)["queries"] == 2
    assert len({stats[c]["kernel_ms"] for c in seq}) == 1  # the shared launch's
    for c in seq:
        assert stats[c]["allocations"] == 0, stats[c]
        case.check(c, calls[c][2], stats[c])
    with pytest.raises(ia.CoreError):  # a token completes once
        idx.wait(calls[0][0])


def test_differing_k_or_ef_never_share(case):
    """(c) calls that differ in k or ef end in different launches and are still right."""
    torch = case.torch
    with switches(ISL_GROUP_ROOM=1, ISL_NO_GROUP=0):  # (held whatever the process's hardware queues are)
        idx = make_index(case.csr, case.v)
    idx.prepare(64, 64, K, 8)
    side = torch.cuda.Stream()
    shapes = [(1, K, EF), (2, K, EF), (3, 3, EF), (4, K, 64), (5, 3, EF)]
    bufs = case.buffers([(c, k) for c, k, _ in shapes])
    tok0, keep = case.fill_the_chip(idx, side)
    calls = [case.submit(idx, c, o, k, ef) for (c, k, ef), o in zip(shapes, bufs)]
    assert counters(idx) == (1, 0, 0)
    stats = [idx.wait_stats(t) for t, _, _ in calls]
    assert counters(idx) == (4, 2, 4)  # {1, 2} and {3, 5} together, 4 alone
    assert stats[0]["kernel_ms"] == stats[1]["kernel_ms"] and stats[2]["kernel_ms"] == stats[4]["kernel_ms"]
    idx.wait(tok0)
    for (c, k, ef), (_, _, o), st in zip(shapes, calls, stats):
        case.check(c, o, st, k, ef)


def test_stream_wait_submits_a_held_call(case):
    """(e) isl_search_stream_wait on a held token submits it; the caller's stream then reads finished outputs
    without the host waiting for the search."""
    torch = case.torch
    with switches(ISL_GROUP_ROOM=1, ISL_NO_GROUP=0):  # (held whatever the process's hardware queues are)
        idx = make_index(case.csr, case.v)
    idx.prepare(64, 64, K, 8)
    side, reader = torch.cuda.Stream(), torch.cuda.Stream()
    bufs = case.buffers([(3, K), (4, K)])
    tok0, keep = case.fill_the_chip(idx, side)
    calls = [case.submit(idx, c, o) for c, o in zip((3, 4), bufs)]
    assert counters(idx) == (1, 0, 0)
    assert _ffi.lib().isl_search_stream_wait(idx._h, calls[1][0], C.c_void_p(reader.cuda_stream)) == 0
    assert counters(idx) == (2, 1, 2)
    with torch.cuda.stream(reader):
        copies = [tuple(x.clone() for x in o) for _, _, o in calls]
    reader.synchronize()
    for c, o in zip((3, 4), copies):
        case.check(c, o, None)
    for c, (t, _, o) in zip((3, 4), calls):
        case.check(c, o, idx.wait_stats(t))
    idx.wait(tok0)


def test_no_group_switch_is_one_launch_per_call(case):
    """(g) ISL_NO_GROUP=1: no call is held or shares a launch."""
    torch = case.torch
    with switches(ISL_NO_GROUP=1, ISL_GROUP_ROOM=1):
        idx = make_index(case.csr, case.v)
    idx.prepare(64, 64, K, 8)
    side = torch.cuda.Stream()
    bufs = case.buffers([(c, K) for c in range(len(SIZES))])
    tok0, keep = case.fill_the_chip(idx, side)
    calls = [case.submit(idx, c, bufs[c]) for c in range(len(SIZES))]
    stats = [idx.wait_stats(t) for t, _, _ in calls]
    idx.wait(tok0)
    assert counters(idx) == (0, 0, 0)
    for c, ((_, _, o), st) in enumerate(zip(calls, stats)):
        case.check(c, o, st)


def test_wrong_dimension_is_refused_before_it_joins(case):
    """(h) a call of the wrong dimension gets its error at once and joins nothing; the held calls complete."""
    torch = case.torch
    with switches(ISL_GROUP_ROOM=1, ISL_NO_GROUP=0):  # (held whatever the process's hardware queues are)
        idx = make_index(case.csr, case.v)
    idx.prepare(64, 64, K, 8)
    side = torch.cuda.Stream()
    bufs = case.buffers([(1, K), (2, K), (5, K)])
    bad, o = case.dev(np.zeros((4, case.d + 1), np.float32)), case.outputs(4, K)
    torch.cuda.synchronize()
    tok0, keep = case.fill_the_chip(idx, side)
    calls = [case.submit(idx, c, b) for c, b in zip((1, 2), bufs)]
    with pytest.raises(ia.CoreError) as e:
        idx.search_batch_device_async(bad.data_ptr(), 4, case.d + 1, K, EF, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())
    assert e.value.kind == "DimensionMismatch"
    calls.append(case.submit(idx, 5, bufs[2]))
    stats = [idx.wait_stats(t) for t, _, _ in calls]
    assert counters(idx) == (2, 1, 3)
    idx.wait(tok0)
    for c, (_, _, o), st in zip((1, 2, 5), calls, stats):
        case.check(c, o, st)
