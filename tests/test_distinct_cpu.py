"""COUNT(DISTINCT) without a GPU: the first-occurrence reference against a brute-force set of tuples, the
WindowAggregateITCase column against its literal values, and the binding's view of the new kind."""
import importlib.util
import json
import os

import numpy as np

from distinct_ref import FirstOccurrence, reference_aggs, tz_local
from flink_amd import _abi as A
from helpers import GOLDEN


def _gen():
    spec = importlib.util.spec_from_file_location("gen_sql_distinct_kats", os.path.join(GOLDEN, "gen_sql_distinct_kats.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_first_occurrence_sums_to_brute_force_distinct_counts():
    rng = np.random.default_rng(3)
    n, size, off = 5000, 1000, 300
    tz = [(-(1 << 40), 3_600_000), (4_000, 7_200_000)]                # a zone that changes offset mid-stream
    keys = rng.integers(-3, 4, n).astype(np.int64)
    ts = rng.integers(-5_000, 12_000, n).astype(np.int64)
    vals = rng.integers(-4, 5, n).astype(np.int64)
    nulls = (rng.random(n) < 0.2).astype(np.uint8)
    f = FirstOccurrence(size, off, tz)
    marks = np.concatenate([f.mark(keys[s], ts[s], vals[s], nulls[s]) for s in (slice(0, 1700), slice(1700, n))])
    assert set(np.unique(marks)) <= {0, 1} and not marks[nulls != 0].any()
    local = tz_local(ts, tz)
    assert (local[ts < 4_000] == ts[ts < 4_000] + 3_600_000).all() and (local[ts >= 4_000] == ts[ts >= 4_000] + 7_200_000).all()
    win = np.floor((local - off) / size).astype(np.int64)
    brute, summed = {}, {}
    for i in range(n):
        kw = (int(keys[i]), int(win[i]))
        brute.setdefault(kw, set())
        summed[kw] = summed.get(kw, 0) + int(marks[i])
        if not nulls[i]:
            brute[kw].add(int(vals[i]))
    assert {k: len(v) for k, v in brute.items()} == summed


def test_first_occurrence_compares_bits():
    f = FirstOccurrence(1000)
    v = np.array([0.0, -0.0, 0.0, np.nan, np.nan])
    assert f.mark(np.zeros(5, np.int64), np.zeros(5, np.int64), v).tolist() == [1, 1, 0, 1, 0]


def test_reference_aggs_rewrite():
    aggs = [("COUNT", 0), ("COUNT_DISTINCT", 1), ("SUM_I64", 0), ("COUNT_DISTINCT", 1), ("COUNT_DISTINCT", 0)]
    out, cols = reference_aggs(aggs, 2)
    assert out == [("COUNT", 0), ("SUM_I64", 2), ("SUM_I64", 0), ("SUM_I64", 2), ("SUM_I64", 3)] and cols == {1: 2, 0: 3}


def test_itcase_distinct_column_is_the_literal_one():
    g = _gen()
    assert g.distinct_column() == [2, 1, 2, 1, 1, 0]
    with open(os.path.join(GOLDEN, "sql_distinct_kats.json")) as f:
        case = json.load(f)["operators"][0]
    assert [r[-1] for r in case["expected"]] == [2, 1, 2, 1, 1, 0]
    assert case["expected"] == [r + [d] for r, d in zip(g.parse(g.TUMBLE), g.distinct_column())]
    assert case["events"] == g.events() and case["late_dropped"] == 1
    assert case["aggs"][-1] == ["COUNT_DISTINCT", 3]


def test_binding_knows_the_kind():
    assert A.AGG_KINDS["COUNT_DISTINCT"] == 33 and A.AGG_RESULT_DTYPE["COUNT_DISTINCT"] == "i8"
    assert A.AGG_INPUT_DTYPE["COUNT_DISTINCT"] == "i8"
    cfg = A.make_config(window_kind="TUMBLE", semantics="TABLE", size_ms=1000, aggs=[("COUNT", 0), ("COUNT_DISTINCT", 0)])
    assert A.agg_names(cfg) == ["COUNT", "COUNT_DISTINCT"]
    from flink_amd.engine import OPTIONS
    assert (OPTIONS["distinct_slots"], OPTIONS["distinct_live"], OPTIONS["distinct_rebuilds"]) == (18, 19, 20)


def test_header_declares_the_kind_and_options():
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "flink_amd.h")) as f:
        h = f.read()
    assert "FWA_COUNT_DISTINCT = 33" in h and "FWA_AGG_KIND_COUNT = 34" in h and "#define FWA_ABI_VERSION 5" in h
    for line in ("FWA_OPT_DISTINCT_SLOTS = 18", "FWA_OPT_DISTINCT_LIVE = 19", "FWA_OPT_DISTINCT_REBUILDS = 20"):
        assert line in h
