"""The group path's marker on the caller's stream (islands_amd/csrc/search_group.hip, group_arrive): a call is ordered
after its caller's stream by an event recorded there only where that stream has work pending; an idle stream gets no
marker.  Whatever the call finds, it must read its queries after the work that was on the caller's stream when it
was made, and answer exactly as the same call made alone.

The fixture shapes, the chip-filling first call and the per-call references are those of test_gpu_search_group.py."""
import ctypes as C

import numpy as np
import pytest

from islands_amd import _ffi
from test_gpu_parity import make_index
from test_gpu_search_group import EF, K, SIZES, Case, counters, switches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(orc):
    return Case(orc, 32)


def markers(idx):
    a, b = C.c_uint64(), C.c_uint64()
    assert _ffi.lib().isl_index_group_markers(idx._h, C.byref(a), C.byref(b)) == 0
    return int(a.value), int(b.value)


def held_index(case, **env):
    with switches(ISL_GROUP_ROOM=1, ISL_NO_GROUP=0, **env):  # (held whatever the process's hardware queues are)
        idx = make_index(case.csr, case.v)
    idx.prepare(64, EF, K, 8)
    return idx


def stale_queries(case, call):
    """A query buffer for `call` that holds ANOTHER call's queries; made before a test's sequence starts."""
    other = case.q[5][:len(case.q[call])]
    assert other.shape == case.q[call].shape and not np.array_equal(other, case.q[call])
    return case.dev(other)


def write_late(case, dq, call, stream):
    """The call's own queries reach `dq` behind some 50 ms of matrix products on `stream`: a search that does not
    wait for the stream answers the wrong questions."""
    with case.torch.cuda.stream(stream):
        x = case.busy
        for _ in range(64):
            x = (x @ case.busy) * 1e-2
        dq.copy_(case.dq[call], non_blocking=True)
    return x


@pytest.mark.parametrize("mark", [0, 1])
def test_idle_caller_stream_gets_no_marker(case, mark):
    """Six held calls from a stream with nothing pending: no marker (every one with ISL_GROUP_MARK=1), one shared
    launch, the answers and counters of the calls made alone.  The chip-filling call has work in front: marked."""
    torch = case.torch
    idx = held_index(case, ISL_GROUP_MARK=mark)
    side = torch.cuda.Stream()
    bufs = case.buffers([(c, K) for c in range(len(SIZES))])
    tok0, keep = case.fill_the_chip(idx, side)
    calls = [case.submit(idx, c, bufs[c]) for c in range(len(SIZES))]
    assert markers(idx) == (7, 7 if mark else 1)
    stats = [idx.wait_stats(t) for t, _, _ in calls]
    assert counters(idx) == (2, 1, 6)
    idx.wait(tok0)
    for c, ((_, _, o), st) in enumerate(zip(calls, stats)):
        assert st["allocations"] == 0, st
        case.check(c, o, st)


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_pending_work_on_the_caller_stream_is_waited_for(case, order):
    """Calls whose queries are written by work still pending on their caller's stream: marked, and answered from
    the queries that work wrote, all three in one shared launch."""
    torch = case.torch
    idx = held_index(case)
    side, mine = torch.cuda.Stream(), torch.cuda.Stream()
    picked = [3, 4, 2]
    dqs = [stale_queries(case, c) for c in picked]
    bufs = case.buffers([(c, K) for c in picked])
    tok0, keep = case.fill_the_chip(idx, side)
    toks, alive = [], []
    for c, o, dq in zip(picked, bufs, dqs):
        alive.append(write_late(case, dq, c, mine))
        toks.append(idx.search_batch_device_async(dq.data_ptr(), len(case.q[c]), case.d, K, EF, o[0].data_ptr(),
                                                  o[1].data_ptr(), o[2].data_ptr(), stream=mine.cuda_stream))
    assert markers(idx) == (4, 4)
    assert counters(idx) == (1, 0, 0)
    seq = list(range(len(picked)))
    stats = {}
    for i in (seq if order == "forward" else seq[::-1]):
        stats[i] = idx.wait_stats(toks[i])
    idx.wait(tok0)
    for i, c in enumerate(picked):
        case.check(c, bufs[i], stats[i])


def test_one_call_alone_behind_pending_work(case):
    """A single held call (its launch runs on its own lane) behind pending work on its caller's stream."""
    torch = case.torch
    idx = held_index(case)
    side, mine = torch.cuda.Stream(), torch.cuda.Stream()
    dq = stale_queries(case, 1)
    (o,) = case.buffers([(1, K)])
    tok0, keep = case.fill_the_chip(idx, side)
    x = write_late(case, dq, 1, mine)
    tok = idx.search_batch_device_async(dq.data_ptr(), len(case.q[1]), case.d, K, EF, o[0].data_ptr(), o[1].data_ptr(),
                                        o[2].data_ptr(), stream=mine.cuda_stream)
    assert markers(idx) == (2, 2)
    st = idx.wait_stats(tok)
    assert counters(idx) == (2, 0, 0)
    idx.wait(tok0)
    case.check(1, o, st)


def test_default_stream_follows_a_blocking_stream(case):
    """The legacy default stream is ordered after every blocking stream of the device.  A call made on it while a
    blocking stream still has the work that writes its queries is marked and waits for that work."""
    torch = case.torch
    hip = C.CDLL("libamdhip64.so")
    raw = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(raw)) == 0  # (no flags: a blocking stream)
    blocking = torch.cuda.ExternalStream(raw.value)
    try:
        idx = held_index(case)
        side = torch.cuda.Stream()
        dq = stale_queries(case, 3)
        (o,) = case.buffers([(3, K)])
        tok0, keep = case.fill_the_chip(idx, side)
        x = write_late(case, dq, 3, blocking)
        tok = idx.search_batch_device_async(dq.data_ptr(), len(case.q[3]), case.d, K, EF, o[0].data_ptr(),
                                            o[1].data_ptr(), o[2].data_ptr())  # stream 0
        assert markers(idx) == (2, 2)
        st = idx.wait_stats(tok)
        idx.wait(tok0)
        case.check(3, o, st)
    finally:
        torch.cuda.synchronize()
        assert hip.hipStreamDestroy(raw) == 0
