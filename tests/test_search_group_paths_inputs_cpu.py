"""The inputs of tests/test_gpu_search_group_paths.py, without a device: the conditions under which those tests
mean something, computed from the scenarios of tests/_group_case.py with the CPU oracle alone.  The conditions are
fixed; the scenarios' seeds are chosen so that they hold."""
import numpy as np
import pytest

import _group_case as gc

DIMS = [32, 50]


@pytest.mark.parametrize("d", DIMS)
def test_bf16_union_has_a_mixed_member_between_members_of_another_kind(orc, d):
    """Scenario 1 over bf16 rows: one call holds bf16-valued queries and others, and in the union of calls 0..5 the
    kind of query changes at both of its boundaries."""
    sc = gc.row_types(orc, d, "bf16")
    kinds = [gc.bf16_valued(q) for q in sc.q]
    mixed = kinds[gc.MIXED]
    assert mixed.any() and not mixed.all()
    assert kinds[gc.MIXED - 1][-1] != mixed[0] and mixed[-1] != kinds[gc.MIXED + 1][0]
    assert kinds[1].all() and kinds[3].all() and not kinds[0].any() and not kinds[4].any()
    # the rounded queries are still what they were rounded from, to bf16's eight bits
    plain_q, _ = gc.member_queries(sc.v, gc.SIZES, gc.TIED, 100 + d)
    for c in (1, 2, 3):
        assert np.abs(sc.q[c] - plain_q[c]).max() <= np.abs(plain_q[c]).max() * 2.0 ** -8


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("metric", [0, 2], ids=["Cosine", "DotProduct"])
@pytest.mark.parametrize("k", [1, 5])
def test_tied_rows_put_equal_distances_across_the_boundary_of_k(orc, d, metric, k):
    """Scenario 6: for k = 1 and k = 5 some query's k + 1 nearest (ef = 32) have equal distance bits at positions
    k - 1 and k -- the tie the returned prefix does not show.  The all-zero queries of the DotProduct variant are
    not counted: all of their distances are -0.0, and they are the heap-exact kernel's."""
    sc = gc.tied_rows(orc, d, metric)
    ef = dict(gc.K_EDGES)[k]
    across = 0
    zeros = 0
    for q in sc.q:
        for x in q:
            r = gc.oracle_search(orc, sc, x, k + 1, ef)
            assert r.status == 0
            b = gc.bits(r.dist)
            if not x.any():
                zeros += 1
                assert (b == 0x80000000).all()
            else:
                across += int(b.size == k + 1 and b[k - 1] == b[k])
    assert across > 0 and zeros == (len(gc.ZERO_AT) if metric else 0)


def test_evicted_twin_ties_with_the_last_result_of_k_equal_ef(orc):
    """Scenario 6, (k, ef) = (8, 8): every query's eight results have eight different distances, with a twin (node
    8 or 9) last; a ninth place (ef = 9) would hold the other twin at the same distance."""
    sc = gc.evicted_twin(orc)
    for q in sc.q + [sc.extra]:
        for x in q:
            r8, r9 = gc.oracle_search(orc, sc, x, 8, 8), gc.oracle_search(orc, sc, x, 9, 9)
            assert r8.status == 0 and r8.counters["pushes"] == 10
            assert len(set(gc.bits(r8.dist).tolist())) == 8 and int(r8.ids[7]) in (8, 9)
            assert sorted(r9.ids[7:].tolist()) == [8, 9] and gc.bits(r9.dist)[7] == gc.bits(r9.dist)[8]


@pytest.mark.parametrize("d", DIMS)
def test_only_the_second_member_reaches_the_row_that_names_a_missing_id(orc, d):
    """Scenario 7: the oracle fails a query of call 1 with NodeNotFound(BAD_ID), the one asked at the node whose row
    names it among them, and no query of calls 0 and 2 nor of the call that fills the chip."""
    sc = gc.failing(orc, d)
    row = sc.csr.neighbors[int(sc.csr.node_offsets[sc.bad_row_of]):int(sc.csr.node_offsets[sc.bad_row_of + 1])]
    assert gc.BAD_ID >= len(sc.v) and gc.BAD_ID in row.tolist() and (sc.csr.neighbors == gc.BAD_ID).sum() == 1
    status = [[gc.oracle_search(orc, sc, x, gc.K, gc.EF) for x in q] for q in sc.q + [sc.extra]]
    assert all(r.status == 0 for c in (0, 2, 3) for r in status[c])
    failed = [i for i, r in enumerate(status[1]) if r.status != 0]
    assert gc.FAIL_AT[1] in failed
    assert all(status[1][i].status == gc.NODE_NOT_FOUND and status[1][i].payload == gc.BAD_ID for i in failed)
    # deep inside a cluster: the node is among the nearest of its own query in the graph without the bad id
    good = gc.plain(orc, d)
    r = gc.oracle_search(orc, good, sc.q[gc.FAIL_AT[0]][gc.FAIL_AT[1]], gc.K, gc.EF)
    assert sc.bad_row_of in r.ids.tolist()
