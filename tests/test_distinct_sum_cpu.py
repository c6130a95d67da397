"""SUM / AVG(DISTINCT col) without a GPU: the reference (distinct_sum_ref.py) against a literal set per (key, window) on
small random streams of both window families, the binding's names and kind values, the header's modifier bit beside the
unchanged enum and ABI version, and the non-vacuity of the random cases the GPU test uses."""
import os

import numpy as np
import pytest

import distinct_sum_ref as R
from flink_amd import _abi as A
from helpers import GOLDEN


def _small_stream(seed, n=1500, pushes=3, f64=False):
    """Sorted timestamps over 8 s, 4 keys (0 among them), values from a small set (0 among them), 25% NULL, each push
    followed by a watermark 500 ms under its newest timestamp; the last sixth of the records arrives 6 s late."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 4, n).astype(np.int64)
    ts = np.sort(rng.integers(0, 8000, n)).astype(np.int64)
    ts[-n // 6:] -= 6000
    pool = np.array([0, 1, -7, 2, 1 << 62, -(1 << 62), (1 << 63) - 1, 5], np.int64)
    vals = pool[rng.integers(0, len(pool), n)]
    if f64:
        vals = (rng.integers(-8, 8, n) / 1024.0).astype(np.float64)                # multiples of 2^-10: exact sums
    plain = rng.integers(-50, 50, n).astype(np.int64)
    nul = (rng.random(n) < 0.25).astype(np.uint8)
    nul[(keys == 3) & (ts < 2000)] = 1                                             # NULL-only windows of key 3
    per, out, mx = n // pushes, [], -(1 << 63)
    for b in range(pushes):
        sl = slice(b * per, (b + 1) * per)
        mx = max(mx, int(ts[sl].max()))
        out.append((keys[sl], ts[sl], [plain[sl], vals[sl]], [None, nul[sl]], mx - 500))
    out.append((keys[:0], ts[:0], [plain[:0], vals[:0]], None, A.LONG_MAX))
    return out


def _literal(batches, late, rows, aggs):
    """{(key, start, end): [per distinct aggregate: (value, is NULL)]} and {...: COUNT(*)} from literal Python sets: for
    every row a watermark fired, over the records accepted up to that watermark (late: the dropped indices per batch)
    with start <= ts < end."""
    recs, out, star = [], {}, {}
    for (keys, ts, cols, nulls, _wm), lo, fired in zip(batches, late, rows):
        drop = set(int(i) for i in lo)
        bits = np.ascontiguousarray(cols[1]).view(np.int64)
        recs += [(int(keys[i]), int(ts[i]), int(bits[i]), bool(nulls[1][i])) for i in range(len(keys)) if i not in drop]
        for i in range(len(fired["key"])):
            kw = (int(fired["key"][i]), int(fired["win_start"][i]), int(fired["win_end"][i]))
            mine = [r for r in recs if r[0] == kw[0] and kw[1] <= r[1] < kw[2]]
            star[kw] = len(mine)
            s = {r[2] for r in mine if not r[3]}
            out[kw] = [R.distinct_result(name, np.array(sorted(s), np.int64)) for name, _c in aggs if R.is_distinct(name)]
    return out, star


def _rows_as_dict(rows, aggs):
    out = {}
    for b in rows:
        for i in range(len(b["key"])):
            kw = (int(b["key"][i]), int(b["win_start"][i]), int(b["win_end"][i]))
            assert kw not in out
            out[kw] = []
            for j, (name, _c) in enumerate(aggs):
                if R.is_distinct(name):
                    z = bool(b["null%d" % j][i]) if "null%d" % j in b else False
                    out[kw].append((b["agg%d" % j][i].item(), z))
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for kw in a:
        for (x, zx), (y, zy) in zip(a[kw], b[kw]):
            assert zx == zy, (kw, a[kw], b[kw])
            assert zx or x == y or (x != x and y != y), (kw, a[kw], b[kw])


@pytest.mark.parametrize("f64", [False, True], ids=["i64", "f64"])
def test_tumble_reference_vs_literal_sets(f64):
    t = "F64" if f64 else "I64"
    aggs = [("COUNT", 0), ("COUNT_DISTINCT", 1), ("SUM_DISTINCT_" + t, 1), ("AVG_DISTINCT_" + t, 1)]
    batches = _small_stream(3, f64=f64)
    ref = R.TumbleReference(dict(R.TUMBLE_KW), aggs, 2, batches)
    assert ref.n_late > 0
    lit, star = _literal(batches, ref.late, ref.rows, aggs)
    got = _rows_as_dict(ref.rows, aggs)
    _same(got, lit)
    assert any(z for v in got.values() for _x, z in v)                     # a NULL-only (key, window) exists


@pytest.mark.parametrize("kind", ["hop", "cumulate"])
def test_range_reference_vs_literal_sets(kind):
    aggs = [("COUNT", 0), ("SUM_DISTINCT_I64", 1), ("AVG_DISTINCT_I64", 1), ("COUNT_DISTINCT", 1)]
    batches = _small_stream(5)
    kw = dict(R.HOP_KW if kind == "hop" else R.CUMULATE_KW)
    ref = R.RangeReference(kw, aggs, batches)
    assert ref.n_late > 0

    lit, star = _literal(batches, ref.late, ref.rows, aggs)
    got = _rows_as_dict(ref.rows, aggs)
    _same(got, lit)
    for b in ref.rows:                                                      # COUNT(*) by the literal count as well
        for i in range(len(b["key"])):
            assert star[(int(b["key"][i]), int(b["win_start"][i]), int(b["win_end"][i]))] == int(b["agg0"][i])


def test_distinct_result_arithmetic():
    i = lambda *x: np.array(x, np.int64)
    f = lambda *x: np.array(x, np.float64).view(np.int64)
    assert R.distinct_result("SUM_DISTINCT_I64", i(5, 5, 7, 5)) == (12, False)
    assert R.distinct_result("AVG_DISTINCT_I64", i(5, 5, 7, 5)) == (6, False)
    assert R.distinct_result("SUM_DISTINCT_I64", i()) == (0, True)
    assert R.distinct_result("SUM_DISTINCT_I64", i(A.LONG_MAX, 1)) == (A.LONG_MIN, False)
    assert R.distinct_result("AVG_DISTINCT_I64", i(-7, 2)) == (-2, False)  # -5 / 2 truncates toward zero
    assert R.distinct_result("SUM_DISTINCT_I64", i(0)) == (0, False)
    assert R.distinct_result("COUNT_DISTINCT", f(-0.0, 0.0)) == (2, False)
    assert R.distinct_result("SUM_DISTINCT_F64", f(-0.0, 0.0))[0] == 0.0
    assert np.isnan(R.distinct_result("SUM_DISTINCT_F64", f(np.inf, -np.inf))[0])
    assert R.distinct_result("SUM_DISTINCT_F64", f(np.inf, 1.0))[0] == np.inf
    assert np.isnan(R.distinct_result("AVG_DISTINCT_F64", f(np.nan, np.nan, 2.0))[0])
    assert R.distinct_result("AVG_DISTINCT_F64", f(0.25, 0.5, 0.5)) == (0.375, False)


def test_binding_names_and_kind_values():
    assert A.AGG_DISTINCT == 0x100
    want = {"SUM_DISTINCT_I64": 0x101, "SUM_DISTINCT_F64": 0x103, "AVG_DISTINCT_I64": 0x10A, "AVG_DISTINCT_F64": 0x10C}
    for name, kind in want.items():
        assert A.AGG_KINDS[name] == kind == 0x100 | A.AGG_KINDS[A.DISTINCT_SUM_KINDS[name]]
        assert A.AGG_NAMES[kind] == name
        assert A.AGG_RESULT_DTYPE[name] == A.AGG_INPUT_DTYPE[name] == ("f8" if name.endswith("F64") else "i8")
    aggs = [("COUNT", 0)] + [(n, 1) for n in want] + [("COUNT_DISTINCT", 1)]
    cfg = A.make_config(window_kind="TUMBLE", semantics="TABLE", size_ms=1000, aggs=aggs)
    assert A.agg_names(cfg) == [a[0] for a in aggs]                       # the names round-trip through the struct
    assert A.AGG_KINDS["COUNT_DISTINCT"] == 33 and len(A.AGG_NAMES) == len(A.AGG_KINDS)


def test_header_declares_the_modifier_bit():
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "flink_amd.h")) as f:
        h = f.read()
    assert "#define FWA_AGG_DISTINCT 0x100" in h
    assert "FWA_AGG_KIND_COUNT = 34" in h and "#define FWA_ABI_VERSION 5" in h        # no new kind, no ABI bump


@pytest.mark.parametrize("name", ["tumble", "hop", "cumulate"])
def test_random_cases_are_not_vacuous(name):
    """The random cases of tests/test_distinct_sum_gpu.py, on the reference alone: a row whose distinct sum differs from
    the plain sum of its column (a value repeated), a row with a NULL result, late drops; for the range cases a row in
    which a value repeats across slices of its window."""
    kw, batches, ref = R.random_case(name)
    assert ref.n_late > 0 and ref.n_rows > 0
    if name == "tumble":
        differ = sum(int(((r["agg3"] != r["agg5"]) & (r["null3"] == 0)).sum()) for r in ref.rows)
        null = sum(int((r["null3"] != 0).sum() + (r["null4"] != 0).sum()) for r in ref.rows)
    else:
        differ, null = ref.stats["differ"], ref.stats["null"]
        assert ref.stats["union"] > 0
    assert differ > 0 and null > 0, (differ, null)
