"""COUNT(DISTINCT) over HOP / CUMULATE windows without a GPU: the WindowAggregateITCase columns against their literal
values, the brute-force reference against the first-occurrence reference on a TUMBLE stream, the binding's view of
FWA_CFG_DISTINCT_RANGE, and the non-vacuity of the GPU test's random streams."""
import importlib.util
import json
import os

import numpy as np
import pytest

from distinct_ref import FirstOccurrence
from distinct_range_ref import BruteForce, count_aggs, random_case
from flink_amd import _abi as A
from helpers import GOLDEN

HOP_COLUMN = [2, 3, 1, 2, 2, 1, 1, 1, 1, 0, 0]
CUMULATE_COLUMN = [2, 3, 3, 2, 2, 1, 1, 1, 1, 1, 1, 0, 0, 0]


def _gen():
    spec = importlib.util.spec_from_file_location("gen_sql_distinct_hop_cumulate_kats",
                                                  os.path.join(GOLDEN, "gen_sql_distinct_hop_cumulate_kats.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_itcase_distinct_columns_are_the_literal_ones():
    g = _gen()
    assert g.distinct_column("SLIDE", g.HOP) == HOP_COLUMN
    assert g.distinct_column("CUMULATE", g.CUMULATE) == CUMULATE_COLUMN


def test_json_is_the_generators_output():
    g = _gen()
    with open(os.path.join(GOLDEN, "sql_distinct_hop_cumulate_kats.json")) as f:
        doc = json.load(f)
    assert doc == json.loads(json.dumps(g.document()))
    hop, cum = doc["operators"]
    assert [r[-1] for r in hop["expected"]] == HOP_COLUMN and [r[-1] for r in cum["expected"]] == CUMULATE_COLUMN
    assert (hop["window_kind"], hop["size_ms"], hop["slide_ms"]) == ("SLIDE", 10000, 5000)
    assert (cum["window_kind"], cum["size_ms"], cum["slide_ms"]) == ("CUMULATE", 15000, 5000)
    for case in (hop, cum):
        assert case["late_dropped"] == 0 and case["aggs"][-1] == ["COUNT_DISTINCT", 3]
        assert ["e", 1, [555, 5.0, None, "Hi"], 1602288004000] in case["events"]       # the late, accepted `Hi`


def test_binding_and_header_declare_the_flag():
    assert A.CFG_DISTINCT_RANGE == 0x20
    cfg = A.make_config(window_kind="SLIDE", semantics="TABLE", size_ms=4000, slide_ms=1000,
                        aggs=[("COUNT", 0), ("COUNT_DISTINCT", 0)], distinct_range=True)
    assert cfg.flags & 0x20
    assert not A.make_config(window_kind="SLIDE", semantics="TABLE", size_ms=4000, slide_ms=1000).flags & 0x20
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "flink_amd.h")) as f:
        h = f.read()
    assert "#define FWA_CFG_DISTINCT_RANGE 0x20" in h
    assert "FWA_AGG_KIND_COUNT = 34" in h and "#define FWA_ABI_VERSION 5" in h          # no new kind, no ABI bump


def test_count_aggs_rewrite():
    aggs = [("COUNT", 0), ("COUNT_DISTINCT", 1), ("SUM_I64", 0), ("COUNT_DISTINCT", 1), ("COUNT_DISTINCT", 0)]
    assert count_aggs(aggs) == ([("COUNT", 0), ("COUNT", 0), ("SUM_I64", 0), ("COUNT", 0), ("COUNT", 0)], [1, 0])


def test_brute_force_agrees_with_first_occurrence_on_a_tumble_stream():
    """The two references tied together: per (key, window) the brute-force count equals the sum of the first-occurrence
    marks, under an offset and a zone that changes its offset mid-stream."""
    rng = np.random.default_rng(4)
    n, size, off = 5000, 1000, 300
    tz = [(-(1 << 40), 3_600_000), (4_000, 7_200_000)]
    keys = rng.integers(-3, 4, n).astype(np.int64)
    ts = rng.integers(-5_000, 12_000, n).astype(np.int64)
    vals = rng.integers(-4, 5, n).astype(np.int64)
    nulls = (rng.random(n) < 0.2).astype(np.uint8)
    f, bf = FirstOccurrence(size, off, tz), BruteForce([0], tz, size, off)
    marks = []
    for s in (slice(0, 1700), slice(1700, n)):
        marks.append(f.mark(keys[s], ts[s], vals[s], nulls[s]))
        bf.add(keys[s], ts[s], [vals[s]], [nulls[s]])
    marks, win = np.concatenate(marks), f.windows(ts)
    summed = {}
    for i in range(n):
        kw = (int(keys[i]), int(win[i]))
        summed[kw] = summed.get(kw, 0) + int(marks[i])
    for (k, w), total in summed.items():
        assert bf.distinct(k, off + w * size, off + (w + 1) * size, 0) == total
        assert bf.pairs(k, off + w * size, off + (w + 1) * size, 0) == total       # one slice: no cross-slice repeats
        assert bf.count_star(k, off + w * size, off + (w + 1) * size) == int(((keys == k) & (win == w)).sum())


def test_brute_force_leaves_out_late_records_and_nulls():
    bf = BruteForce([0], None, 1000, 0)
    bf.add(np.array([1, 1, 1, 1]), np.array([100, 1100, 1200, 2100]), [np.array([7, 7, 8, 9])],
           [np.array([0, 0, 1, 0], np.uint8)], late=[3])
    assert bf.count_star(1, 0, 4000) == 3 and bf.distinct(1, 0, 4000, 0) == 1 and bf.pairs(1, 0, 4000, 0) == 2
    assert bf.live_tuples(lambda q: q < 1) == {(1, 7, 1, 0)}


@pytest.mark.parametrize("name", ["hop", "cumulate", "hop_shift"])
def test_random_streams_exercise_the_cross_slice_union(name):
    """The GPU test's random streams through the oracle and the brute force alone (which also asserts COUNT(*) of
    every row): late records are dropped, steps fire rows, and in at least a quarter of the rows the distinct count is
    smaller than the number of different (value, slice) pairs, so a per-slice sum would be wrong there."""
    _kw, _batches, ref = random_case(name)
    assert ref.n_late > 0 and ref.n_rows > 1000
    assert 4 * ref.n_union >= ref.n_rows, (ref.n_union, ref.n_rows)
