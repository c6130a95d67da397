"""The reference of the distinct-session tests (distinct_session_ref.py) on its own: no GPU.

The reference against literal Python sets on a hand-written stream that holds the two counter-examples of the cell
argument; the non-vacuity counters a .. f of the random streams the GPU tests use; and a pure-Python model of the cell
bitmap, which equals the reference with both of its rules and differs from it with either switched off."""
import numpy as np
import pytest

import distinct_session_ref as R
from flink_amd import _abi as A


def _i64(x):
    return np.asarray(x, np.int64)


def _batch(recs, wm):
    a = _i64(recs).reshape(len(recs), 3)
    return (a[:, 0].copy(), a[:, 1].copy(), [a[:, 2].copy()], None, wm)


def _step(wm):
    e = np.zeros(0, np.int64)
    return (e, e, [e], None, wm)


AGGS = [("COUNT", 0), ("COUNT_DISTINCT", 0), ("SUM_DISTINCT_I64", 0)]


def _fired(ref, b):
    r = ref.rows[b]
    return sorted(zip(r["key"].tolist(), r["win_start"].tolist(), r["win_end"].tolist(), r["agg0"].tolist(),
                      r["agg1"].tolist(), r["agg2"].tolist()))


def test_reference_against_literal_sets():
    """gap 10. Key 1: 25 opens [25, 35); at watermark 20 the record 10 (value 7) is dropped while 12 (value 8), in the
    same cell, is accepted as [12, 22). Key 2: [0, 10) = {3, 4} fires at watermark 9, then 5 (value 6) opens [5, 15) in
    the same cell 0. Key 3: 48 is late on its own at watermark 60 but is saved by [55, 65) -> [48, 65), whose start
    lies below the record 50 of the session [50, 60) that fired at 59."""
    kw = dict(R.SESSION_KW, gap_ms=10)
    batches = [
        _batch([(2, 0, 3), (2, 0, 4), (2, 0, 3)], 9),                       # fires key 2 [0, 10)
        _batch([(1, 25, 3), (2, 5, 6)], 20),                                # fires key 2 [5, 15)
        _batch([(1, 10, 7), (1, 12, 8), (3, 50, 1)], 59),                   # 10 dropped; fires key 1 twice, key 3 [50, 60)
        _batch([(3, 55, 2)], 60),
        _batch([(3, 48, 2), (3, 30, 9)], A.LONG_MAX),                       # 48 saved, 30 dropped
    ]
    ref = R.SessionReference(kw, AGGS, batches)
    assert [x.tolist() for x in ref.late] == [[], [], [0], [], [1]]
    assert _fired(ref, 0) == [(2, 0, 10, 3, len({3, 4}), sum({3, 4}))]
    assert _fired(ref, 1) == [(2, 5, 15, 1, len({6}), sum({6}))]             # not {3, 4, 6}: cell 0 was cleared
    assert _fired(ref, 2) == [(1, 12, 22, 1, len({8}), sum({8})),           # not {7, 8}: 10 was dropped
                              (1, 25, 35, 1, len({3}), sum({3})), (3, 50, 60, 1, len({1}), sum({1}))]
    assert _fired(ref, 3) == []
    assert _fired(ref, 4) == [(3, 48, 65, 2, len({2}), sum({2}))]           # not {1, 2}: 50 belongs to the fired session
    assert ref.counters["d"] >= 2 and ref.counters["e"] >= 1 and ref.counters["f"] >= 1
    assert R.model_matches(ref, batches)
    assert not R.model_matches(ref, batches, drop_filter=False)
    assert not R.model_matches(ref, batches, clear=False)


def test_live_tuples_are_those_of_the_sessions_in_flight():
    kw = dict(R.SESSION_KW, gap_ms=10)
    ref = R.SessionReference(kw, AGGS, [_batch([(1, 0, 3), (1, 5, 3), (1, 12, 4), (2, -50, 3), (2, 130, 5)], 20)])
    assert ref.live_tuples() == {(1, 3, 0, 0), (1, 4, 1, 0), (2, 5, 13, 0)}   # key 2's [-50, -40) has fired


@pytest.mark.parametrize("name", R.RANDOM)
def test_random_streams_are_not_vacuous(name):
    """A condition on the inputs: every stream has rows that need the union (a), steps firing two sessions of a key in
    one block (c), records in cells of fired sessions (d), dropped records that must set no bit (e) and saved records
    (f); the stream of gap 3 has sessions across three blocks with a value in the first and the last (b)."""
    kw, aggs, batches, ref = R.random_case(name)
    c = ref.counters
    assert all(c[x] >= 1 for x in "acdef"), c
    if name == "g3_blocks":
        assert c["b"] >= 1, c
    assert ref.n_late > 0 and sum(len(r["key"]) > 0 for r in ref.rows) >= len(batches) - 1
    assert 2000 <= sum(len(b[0]) for b in batches) <= 5000 and 6 <= len(batches) - 1 <= 10
    if name == "g50_nulls":
        assert ref.stats["null"] > 0


def test_the_counters_hold_over_the_streams_together():
    total = dict.fromkeys("abcdef", 0)
    for name in R.RANDOM:
        for x, v in R.random_case(name)[3].counters.items():
            total[x] += v
    assert all(v >= 1 for v in total.values()), total


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_cell_model_equals_the_reference(name):
    kw, aggs, batches, ref = R.random_case(name)
    assert R.model_matches(ref, batches)


@pytest.mark.parametrize("name", R.RANDOM)
def test_cell_model_needs_both_rules(name):
    kw, aggs, batches, ref = R.random_case(name)
    assert not R.model_matches(ref, batches, drop_filter=False)
    assert not R.model_matches(ref, batches, clear=False)


def test_python_gains_the_flag():
    c = A.make_config(window_kind="SESSION", semantics="TABLE", gap_ms=10, aggs=[("COUNT_DISTINCT", 0)],
                      distinct_session=True)
    assert A.CFG_DISTINCT_SESSION == 0x40 and c.flags == 0x40
    assert A.make_config().flags == 0
