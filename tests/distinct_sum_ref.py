"""Reference for SUM(DISTINCT col) / AVG(DISTINCT col) (FWA_AGG_DISTINCT) over Table windows, shared by the distinct-sum
tests. It is built from the references that exist and never calls the engine.

TUMBLE: the oracle over a nullable copy of every distinct column whose NULL flags are "input NULL, or not the first
occurrence of its (key, window, value)" (distinct_ref.FirstOccurrence). COUNT_DISTINCT becomes COUNT_COL over that
column, SUM / AVG_DISTINCT_* become SUM / AVG_* over it: the oracle's own SQL NULL semantics then give sums, averages,
NULL results, late drops and late indices (within a window acceptance only ever turns off, so a first occurrence is
accepted whenever any occurrence is).

HOP / CUMULATE: every other column from the oracle with COUNT(*) in place of each distinct aggregate, the distinct
columns from distinct_range_ref.BruteForce extended with distinct_sum() over the unique non-NULL value bits of the
window. BIGINT sums wrap; DOUBLE sums are exact rationals (fractions.Fraction, as float_ref does), so a stream whose sums
are exactly representable has error bound 0 and compares bit for bit, the sign of a zero sum aside. The oracle's
COUNT(*) is recomputed by brute force and asserted before a distinct column is trusted.
"""
from fractions import Fraction

import numpy as np

from distinct_ref import FirstOccurrence
from distinct_range_ref import BruteForce, slice_ms_of
from flink_amd import _abi as A

SUM_KINDS = A.DISTINCT_SUM_KINDS                           # name -> the plain aggregate of the same arithmetic


def is_sum(name):
    return name in SUM_KINDS


def is_distinct(name):
    return name == "COUNT_DISTINCT" or name in SUM_KINDS


def value_dtype(name):
    return "f8" if name.endswith("F64") else "i8"


def wrap64(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >= 1 << 63 else x


def java_div(a, b):
    """Java long division: truncation toward zero (b > 0)."""
    q = abs(a) // b
    return -q if a < 0 else q


def distinct_result(name, bits):
    """(value, is NULL) of the aggregate `name` over the unique non-NULL value bits `bits` (int64) of one window."""
    u = np.unique(np.asarray(bits, np.int64))
    n = len(u)
    if name == "COUNT_DISTINCT":
        return n, False
    if n == 0:
        return 0, True
    if value_dtype(name) == "i8":
        s = wrap64(sum(int(x) for x in u))
        return (s if name.startswith("SUM") else java_div(s, n)), False
    f = u.view(np.float64)
    if np.isnan(f).any() or (np.isposinf(f).any() and np.isneginf(f).any()):
        return float("nan"), False
    if np.isinf(f).any():
        s = np.float64(f[np.isinf(f)][0])
    else:
        exact = sum((Fraction(float(x)) for x in f), Fraction(0))
        s = np.float64(float(exact))
        assert Fraction(float(s)) == exact, "the stream's DOUBLE sums must be exactly representable"
    return (s if name.startswith("SUM") else s / np.float64(n)), False


def _order(r):
    return np.lexsort((r["win_end"], r["win_start"], r["key"]))


def assert_sum_rows_equal(got, exp, names, ctx=""):
    """Multiset equality of two fired-row dicts: integer columns bit for bit, DOUBLE columns bit for bit with -0.0 read
    as +0.0 and any NaN equal to any NaN; NULL flags equal, and a real array on `got` for every SUM / AVG(DISTINCT)."""
    n = len(exp["key"])
    assert len(got["key"]) == n, "%s row count %d != %d" % (ctx, len(got["key"]), n)
    for j, name in enumerate(names):
        if is_sum(name):
            assert "null%d" % j in got, "%s agg %d %s: agg_null must be a real array" % (ctx, j, name)
        if name == "COUNT_DISTINCT":
            assert "null%d" % j not in got, "%s COUNT(DISTINCT) is never NULL" % ctx
    if n == 0:
        return
    og, oe = _order(got), _order(exp)
    for f in ("key", "win_start", "win_end"):
        assert np.array_equal(got[f][og], exp[f][oe]), "%s column %s differs" % (ctx, f)
    for j, name in enumerate(names):
        x, y = np.asarray(got["agg%d" % j])[og], np.asarray(exp["agg%d" % j])[oe]
        zg, ze = got.get("null%d" % j), exp.get("null%d" % j)
        zg = np.zeros(n, bool) if zg is None else np.asarray(zg)[og] != 0
        ze = np.zeros(n, bool) if ze is None else np.asarray(ze)[oe] != 0
        assert np.array_equal(zg, ze), "%s agg %d %s NULL flags differ: %s vs %s" % (ctx, j, name, zg, ze)
        x, y = x[~ze], y[~ze]
        if x.dtype.kind == "f":
            x, y = x.astype(np.float64) + 0.0, y.astype(np.float64) + 0.0           # -0.0 -> +0.0
            nan = np.isnan(y)
            assert np.array_equal(np.isnan(x), nan), "%s agg %d %s NaNs differ" % (ctx, j, name)
            x, y = x[~nan].view(np.int64), y[~nan].view(np.int64)
        bad = np.nonzero(x != y)[0]
        assert len(bad) == 0, "%s agg %d %s differs at %d rows, first %s vs %s" % (ctx, j, name, len(bad), x[bad[0]],
                                                                                 y[bad[0]])


# ---- TUMBLE ----

def tumble_aggs(aggs, ncols):
    """aggs with every distinct aggregate over c mapped to its plain form over an appended nullable column; returns
    (aggs', {c: column'})."""
    cols, out = {}, []
    for spec in aggs:
        name, c = spec[0], spec[1]
        if is_distinct(name):
            cols.setdefault(c, ncols + len(cols))
            out.append(("COUNT_COL" if name == "COUNT_DISTINCT" else SUM_KINDS[name], cols[c]))
        else:
            out.append(tuple(spec))
    return out, cols


class TumbleReference:
    """Per batch [(keys, ts, cols, nulls or None, watermark)]: the expected rows of its watermark and the late indices
    of its push. `names` are the caller's aggregate names."""

    def __init__(self, cfg_kw, aggs, ncols, batches):
        from oracle.oracle import Oracle
        raggs, dcols = tumble_aggs(aggs, ncols)
        kw = {k: v for k, v in cfg_kw.items() if k not in ("record_lists", "output_on_device")}
        nullable = tuple(kw.pop("nullable_cols", ())) + tuple(dcols.values())
        o = Oracle(A.make_config(aggs=raggs, nullable_cols=nullable, late_indices=True, **kw))
        first = {c: FirstOccurrence(kw["size_ms"], kw.get("offset_ms", 0), kw.get("tz")) for c in dcols}
        self.names = [s[0] for s in aggs]
        self.rows, self.late = [], []
        for keys, ts, cols, nulls, wm in batches:
            lo = np.zeros(0, np.int32)
            if len(keys):
                extra, extra_nulls = [], []
                for c in dcols:
                    z = None if nulls is None or nulls[c] is None else nulls[c]
                    mark = first[c].mark(keys, ts, cols[c], z)
                    extra.append(cols[c])
                    extra_nulls.append((mark == 0).astype(np.uint8))       # NULL input, or a repeat of its value
                base_nulls = [None] * len(cols) if nulls is None else list(nulls)
                n = o.push(keys, ts, list(cols) + extra, nulls=base_nulls + extra_nulls)
                lo = np.array(o.late_records(), copy=True)
                assert n == len(lo)
            self.rows.append(o.advance_watermark(wm))
            self.late.append(lo)
        o.close()
        self.n_late = sum(len(x) for x in self.late)
        self.n_rows = sum(len(r["key"]) for r in self.rows)


# ---- HOP / CUMULATE ----

class SumBruteForce(BruteForce):
    def window_bits(self, key, start, end, c):
        idx = self._in(key, start, end)
        return self.bits[c][idx][~self.nul[c][idx]]

    def distinct_sum(self, key, start, end, c, dtype):
        """(sum, is NULL) of the unique non-NULL value bits of column c in the window, as dtype 'i8' or 'f8'."""
        return distinct_result("SUM_DISTINCT_I64" if dtype == "i8" else "SUM_DISTINCT_F64",
                               self.window_bits(key, start, end, c))

    def plain_sum_i64(self, key, start, end, c):
        return wrap64(sum(int(x) for x in self.window_bits(key, start, end, c)))


def range_aggs(aggs):
    """aggs with every distinct aggregate replaced by COUNT(*), and the distinct source columns in first-use order."""
    out, dcols = [], []
    for spec in aggs:
        if is_distinct(spec[0]):
            out.append(("COUNT", 0))
            if spec[1] not in dcols:
                dcols.append(spec[1])
        else:
            out.append(tuple(spec))
    return out, dcols


def range_expected_rows(ro, aggs, bf, stats=None):
    """The oracle's rows `ro` (COUNT(*) where the distinct aggregates are) with the distinct columns from brute force.
    stats counts the non-vacuity conditions: rows, rows whose distinct sum differs from the plain sum (`differ`), rows
    in which a value repeats across slices (`union`), rows with a NULL result (`null`)."""
    exp = dict(ro)
    n = len(ro["key"])
    jd = [j for j, s in enumerate(aggs) if is_distinct(s[0])]
    for j in jd:
        exp["agg%d" % j] = np.zeros(n, A.AGG_RESULT_DTYPE[aggs[j][0]])
        if is_sum(aggs[j][0]):
            exp["null%d" % j] = np.zeros(n, np.uint8)
    for i in range(n):
        k, s, e = int(ro["key"][i]), int(ro["win_start"][i]), int(ro["win_end"][i])
        star = bf.count_star(k, s, e)
        assert star == int(ro["agg%d" % jd[0]][i]), ("brute-force COUNT(*) differs from the oracle", k, s, e, star)
        union = differ = null = False
        for j in jd:
            name, c = aggs[j][0], aggs[j][1]
            bits = bf.window_bits(k, s, e, c)
            v, z = distinct_result(name, bits)
            exp["agg%d" % j][i] = v
            if is_sum(name):
                exp["null%d" % j][i] = z
                null |= z
                if name == "SUM_DISTINCT_I64":
                    differ |= (not z) and v != bf.plain_sum_i64(k, s, e, c)
                union |= len(np.unique(bits)) < bf.pairs(k, s, e, c)
        if stats is not None:
            stats["rows"] += 1
            stats["union"] += union
            stats["differ"] += differ
            stats["null"] += null
    return exp


class RangeReference:
    def __init__(self, cfg_kw, aggs, batches):
        from oracle.oracle import Oracle
        raggs, dcols = range_aggs(aggs)
        kw = {k: v for k, v in cfg_kw.items() if k != "output_on_device"}
        nullable = tuple(kw.pop("nullable_cols", ()))
        o = Oracle(A.make_config(aggs=raggs, nullable_cols=nullable, late_indices=True, **kw))
        self.names = [s[0] for s in aggs]
        self.brute = SumBruteForce(dcols, kw.get("tz"), slice_ms_of(kw), kw.get("offset_ms", 0))
        self.stats = {"rows": 0, "union": 0, "differ": 0, "null": 0}
        self.rows, self.late = [], []
        for keys, ts, cols, nulls, wm in batches:
            lo = np.zeros(0, np.int32)
            if len(keys):
                n = o.push(keys, ts, cols, nulls=nulls)
                lo = np.array(o.late_records(), copy=True)
                assert n == len(lo)
                self.brute.add(keys, ts, cols, nulls, lo)
            self.rows.append(range_expected_rows(o.advance_watermark(wm), aggs, self.brute, self.stats))
            self.late.append(lo)
        o.close()
        self.n_late = sum(len(x) for x in self.late)
        self.n_rows = self.stats["rows"]


def range_cfg(cfg_kw, aggs, **more):
    kw = dict(cfg_kw, **more)
    nullable = tuple(kw.pop("nullable_cols", ()))
    return A.make_config(aggs=list(aggs), nullable_cols=nullable, late_indices=True, distinct_range=True, **kw)


def tumble_cfg(cfg_kw, aggs, **more):
    kw = dict(cfg_kw, **more)
    nullable = tuple(kw.pop("nullable_cols", ()))
    return A.make_config(aggs=list(aggs), nullable_cols=nullable, late_indices=True, **kw)


def check_engine(g, ref, batches, first=0, last=None, device=False, sync=True, async_wm=False):
    """Push batches[first:last] through the handle `g`: rows after every watermark and late indices after every
    synchronous push must equal the reference's. async_wm: the rows come from advance_watermark_async / fired_output.
    Returns the rows compared."""
    rows = 0
    for b in range(first, len(batches) if last is None else last):
        keys, ts, cols, nulls, wm = batches[b]
        if len(keys):
            if device:
                import torch
                dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
                keep = (dev(keys), dev(ts), [dev(c) for c in cols], None if nulls is None else [dev(z) for z in nulls])
                dg = g.push(keep[0], keep[1], keep[2], nulls=keep[3], sync=sync)
            else:
                dg = g.push(keys, ts, cols, nulls=nulls)
            if sync:
                assert np.array_equal(g.late_records(), ref.late[b]), "late indices differ (batch %d)" % b
                assert dg == len(ref.late[b])
        if async_wm:
            g.advance_watermark_async(wm)
            rg = g.fired_output()
        else:
            rg = g.advance_watermark(wm)
        assert_sum_rows_equal(rg, ref.rows[b], ref.names, ctx="batch %d wm=%d" % (b, wm))
        rows += len(rg["key"])
    return rows


# ---- the random cases of tests/test_distinct_sum_gpu.py (their reference alone: tests/test_distinct_sum_cpu.py) ----

TUMBLE_KW = dict(window_kind="TUMBLE", semantics="TABLE", size_ms=1000)
HOP_KW = dict(window_kind="SLIDE", semantics="TABLE", size_ms=4000, slide_ms=1000)
CUMULATE_KW = dict(window_kind="CUMULATE", semantics="TABLE", size_ms=4000, slide_ms=1000)
# columns: 0 BIGINT (plain), 1 BIGINT of 8 values, 2 BIGINT of 8 values << 40 (distinct_range_ref.random_batches)
RANDOM_AGGS = [("COUNT", 0), ("SUM_I64", 0), ("COUNT_DISTINCT", 1), ("SUM_DISTINCT_I64", 1), ("AVG_DISTINCT_I64", 2),
               ("SUM_I64", 1)]

_REFS = {}


def random_case(name):
    """(configuration, batches, reference) of a named random case, computed once per process. The streams are those of
    distinct_range_ref.random_batches at a quarter of their length (2^14 records, 8 pushes): every row still holds
    repeats, NULL-only windows appear at the stream's edges."""
    if name not in _REFS:
        from distinct_range_ref import random_batches
        batches = random_batches(n=1 << 14, null_p=0.3, nkeys=400)
        if name == "tumble":
            kw = dict(TUMBLE_KW, key_capacity=1024, nullable_cols=(1, 2))
            ref = TumbleReference(kw, RANDOM_AGGS, 3, batches)
        else:
            kw = dict(HOP_KW if name == "hop" else CUMULATE_KW, key_capacity=1024, nullable_cols=(1, 2))
            ref = RangeReference(kw, RANDOM_AGGS, batches)
        _REFS[name] = (kw, batches, ref)
    return _REFS[name]
