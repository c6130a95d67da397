"""Reference for COUNT(DISTINCT col) over Table HOP / CUMULATE windows (FWA_CFG_DISTINCT_RANGE), shared by the
distinct-range tests and by tests/golden/gen_sql_distinct_hop_cumulate_kats.py.

Every column but the distinct ones comes from the existing oracle, run on the same stream with ("COUNT", 0) in place of
every COUNT_DISTINCT: the rows per watermark, the late drops and late_records() per push. The distinct columns come
from brute force: BruteForce keeps the accepted records (those not in the oracle's late indices) as (key, local ts,
value bits, NULL?) and, for a fired row (key, start, end), counts the different non-NULL value bits among the records
pushed so far with start <= local ts < end. It recomputes COUNT(*) of the row the same way, and the caller asserts that
it equals the oracle's: that proves the window membership (a shift time zone included) before the distinct column is
trusted.
"""
import numpy as np


def tz_local(ts, tz):
    """Local wall-clock millis of epoch instants under a shift time zone [(utc_instant_ms, offset_ms), ...]."""
    ts = np.asarray(ts, np.int64)
    if not tz:
        return ts
    inst = np.array([p[0] for p in tz], np.int64)
    offs = np.array([p[1] for p in tz], np.int64)
    idx = np.clip(np.searchsorted(inst, ts, side="right") - 1, 0, None)
    return ts + offs[idx]


class BruteForce:
    """The accepted records so far, and counts over [start, end) of one key."""

    def __init__(self, dcols, tz=None, slice_ms=None, offset_ms=0):
        self.dcols, self.tz = list(dcols), tz
        self.slice_ms, self.off = slice_ms, offset_ms
        self.keys = np.zeros(0, np.int64)
        self.lts = np.zeros(0, np.int64)
        self.bits = {c: np.zeros(0, np.int64) for c in self.dcols}
        self.nul = {c: np.zeros(0, bool) for c in self.dcols}
        self._by_key = None

    def add(self, keys, ts, cols, nulls=None, late=()):
        """One push: cols[c] / nulls[c] are the batch's value column c and its NULL flags; late: dropped indices."""
        keep = np.ones(len(keys), bool)
        keep[np.asarray(late, np.int64)] = False
        self.keys = np.concatenate([self.keys, np.asarray(keys, np.int64)[keep]])
        self.lts = np.concatenate([self.lts, tz_local(ts, self.tz)[keep]])
        for c in self.dcols:
            self.bits[c] = np.concatenate([self.bits[c], np.ascontiguousarray(cols[c]).view(np.int64)[keep]])
            z = None if nulls is None else nulls[c]
            z = np.zeros(len(keys), bool) if z is None else np.asarray(z) != 0
            self.nul[c] = np.concatenate([self.nul[c], z[keep]])
        self._by_key = None

    def _index(self, key):
        if self._by_key is None:
            order = np.argsort(self.keys, kind="stable")
            ks, first = np.unique(self.keys[order], return_index=True)
            bounds = list(first) + [len(order)]
            self._by_key = {int(k): order[bounds[i]:bounds[i + 1]] for i, k in enumerate(ks)}
        return self._by_key.get(int(key), np.zeros(0, np.int64))

    def _in(self, key, start, end):
        idx = self._index(key)
        t = self.lts[idx]
        return idx[(t >= start) & (t < end)]

    def count_star(self, key, start, end):
        return len(self._in(key, start, end))

    def distinct(self, key, start, end, c):
        idx = self._in(key, start, end)
        return len(np.unique(self.bits[c][idx][~self.nul[c][idx]]))

    def pairs(self, key, start, end, c):
        """Different (value, slice) pairs of the window: more than distinct() iff a value repeats across slices."""
        idx = self._in(key, start, end)
        idx = idx[~self.nul[c][idx]]
        q = (self.lts[idx] - self.off) // self.slice_ms
        return len(set(zip(self.bits[c][idx].tolist(), q.tolist())))

    def live_tuples(self, fired):
        """(key, value, slice, column) tuples of the slices q with not fired(q) (snapshot section size)."""
        q = (self.lts - self.off) // self.slice_ms
        live = ~np.array([fired(int(x)) for x in q], bool) if len(q) else np.zeros(0, bool)
        out = set()
        for d, c in enumerate(self.dcols):
            m = live & ~self.nul[c]
            out |= set(zip(self.keys[m].tolist(), self.bits[c][m].tolist(), q[m].tolist(), [d] * int(m.sum())))
        return out


def count_aggs(aggs):
    """aggs with every COUNT_DISTINCT(c) replaced by COUNT(*), and the distinct source columns in first-use order."""
    out, dcols = [], []
    for spec in aggs:
        if spec[0] == "COUNT_DISTINCT":
            out.append(("COUNT", 0))
            if spec[1] not in dcols:
                dcols.append(spec[1])
        else:
            out.append(tuple(spec))
    return out, dcols


def expected_rows(ro, aggs, bf, stats=None):
    """The oracle's rows `ro` (COUNT(*) where the distinct aggregates are) with the distinct columns from brute force.
    The first COUNT(*)-valued column is recomputed by brute force and asserted. stats: {"rows", "union"} counters of
    the non-vacuity condition (rows whose distinct count is smaller than their (value, slice) pairs)."""
    exp = dict(ro)
    n = len(ro["key"])
    jd = [j for j, s in enumerate(aggs) if s[0] == "COUNT_DISTINCT"]
    for j in jd:
        exp["agg%d" % j] = np.zeros(n, np.int64)
    for i in range(n):
        k, s, e = int(ro["key"][i]), int(ro["win_start"][i]), int(ro["win_end"][i])
        star = bf.count_star(k, s, e)
        assert star == int(ro["agg%d" % jd[0]][i]), ("brute-force COUNT(*) differs from the oracle", k, s, e, star)
        for j in jd:
            exp["agg%d" % j][i] = bf.distinct(k, s, e, aggs[j][1])
        if stats is not None and bf.slice_ms:
            stats["rows"] += 1
            stats["union"] += exp["agg%d" % jd[0]][i] < bf.pairs(k, s, e, aggs[jd[0]][1])
    return exp


def slice_ms_of(kw):
    from math import gcd
    return gcd(int(kw["size_ms"]), int(kw["slide_ms"]))


class Reference:
    """What the oracle and the brute force give for a stream: per batch the expected rows of its watermark and the
    late indices of its push; `union` / `rows` count the rows of the non-vacuity condition; `most` is the largest
    number of windows one step fired; `brute` keeps the accepted records."""

    def __init__(self, cfg_kw, aggs, batches):
        from flink_amd import _abi as A
        from oracle.oracle import Oracle
        raggs, dcols = count_aggs(aggs)
        kw = {k: v for k, v in cfg_kw.items() if k != "output_on_device"}
        nullable = tuple(kw.pop("nullable_cols", ()))
        rcfg = A.make_config(aggs=raggs, nullable_cols=nullable, late_indices=True, **kw)
        self.names = A.agg_names(rcfg)
        self.aggs = list(aggs)
        o = Oracle(rcfg)
        self.brute = BruteForce(dcols, kw.get("tz"), slice_ms_of(kw), kw.get("offset_ms", 0))
        stats = {"rows": 0, "union": 0}
        self.rows, self.late, self.most = [], [], 0
        for keys, ts, cols, nulls, wm in batches:
            lo = np.zeros(0, np.int32)
            if len(keys):
                n = o.push(keys, ts, cols, nulls=nulls)
                lo = np.array(o.late_records(), copy=True)
                assert n == len(lo)
                self.brute.add(keys, ts, cols, nulls, lo)
            ro = o.advance_watermark(wm)
            self.rows.append(expected_rows(ro, aggs, self.brute, stats))
            self.late.append(lo)
            self.most = max(self.most, len({(int(s), int(e)) for s, e in zip(ro["win_start"], ro["win_end"])}))
        o.close()
        self.n_rows, self.n_union = stats["rows"], stats["union"]
        self.n_late = sum(len(x) for x in self.late)


def check_engine(g, ref, batches, first=0, last=None, device=False):
    """Push batches[first:last] through the handle `g`; rows after every watermark and late indices after every push
    must equal the reference's. Returns the rows compared."""
    from helpers import assert_rows_equal
    rows = 0
    for b in range(first, len(batches) if last is None else last):
        keys, ts, cols, nulls, wm = batches[b]
        if len(keys):
            if device:
                import torch
                dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
                dg = g.push(dev(keys), dev(ts), [dev(c) for c in cols],
                            nulls=None if nulls is None else [dev(z) for z in nulls])
            else:
                dg = g.push(keys, ts, cols, nulls=nulls)
            assert np.array_equal(g.late_records(), ref.late[b]), "late indices differ (batch %d)" % b
            assert dg == len(ref.late[b])
        rg = g.advance_watermark(wm)
        assert_rows_equal(rg, ref.rows[b], ref.names, ctx="batch %d wm=%d" % (b, wm))
        for j, spec in enumerate(ref.aggs):
            if spec[0] == "COUNT_DISTINCT":
                assert "null%d" % j not in rg, "COUNT(DISTINCT) is never NULL"
        rows += len(rg["key"])
    return rows


def run_range_vs_reference(eng_mod, cfg_kw, aggs, batches, device=False, options=None):
    """One handle with `aggs` under FWA_CFG_DISTINCT_RANGE against the reference of the same stream. Returns the
    Reference and the option reader's values."""
    ref = Reference(cfg_kw, aggs, batches)
    g = eng_mod.WindowAggregator(make_cfg(cfg_kw, aggs), options=options)
    check_engine(g, ref, batches, device=device)
    opts = {n: g.get_option(n) for n in ("distinct_slots", "distinct_live", "distinct_rebuilds")}
    assert g.stats().late_dropped == ref.n_late
    g.close()
    return ref, opts


def make_cfg(cfg_kw, aggs, **more):
    from flink_amd import _abi as A
    kw = dict(cfg_kw, **more)
    nullable = tuple(kw.pop("nullable_cols", ()))
    return A.make_config(aggs=list(aggs), nullable_cols=nullable, late_indices=True, distinct_range=True, **kw)


# ---- the random streams of tests/test_distinct_range_gpu.py (their reference alone: tests/test_distinct_range_cpu.py) ----

RANDOM_AGGS = [("COUNT", 0), ("SUM_I64", 0), ("COUNT_DISTINCT", 1), ("COUNT_DISTINCT", 2)]
HOP_KW = dict(window_kind="SLIDE", semantics="TABLE", size_ms=4000, slide_ms=1000)
CUMULATE_KW = dict(window_kind="CUMULATE", semantics="TABLE", size_ms=4000, slide_ms=1000)
SHIFT_T0 = 1615593600000


def random_batches(seed=21, t0=0, pushes=8, n=1 << 16, nkeys=200, nvals=8, span=40_000, disorder=6000, delay=1000,
                   null_p=0.1):
    """2^16 records of 200 keys, two distinct columns of 8 values each (10% NULL), timestamps sorted over 40 slices of
    1 s then moved back by up to 6 s, in 8 pushes each followed by a watermark 1 s under the newest timestamp (so a
    HOP 4 s / 1 s handle drops the oldest quarter of the displaced records and a CUMULATE one more), then end of input."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, nkeys, n).astype(np.int64)
    ts = t0 + np.sort(rng.integers(0, span, n)).astype(np.int64) - rng.integers(0, disorder + 1, n)
    cols = [rng.integers(-1000, 1000, n).astype(np.int64), rng.integers(0, nvals, n).astype(np.int64),
            rng.integers(-nvals // 2, nvals // 2, n).astype(np.int64) << 40]
    nulls = [None, (rng.random(n) < null_p).astype(np.uint8), (rng.random(n) < null_p).astype(np.uint8)]
    per, mx, out = n // pushes, -(1 << 63), []
    for b in range(pushes):
        sl = slice(b * per, (b + 1) * per)
        mx = max(mx, int(ts[sl].max()))
        out.append((keys[sl], ts[sl], [c[sl] for c in cols], [None if z is None else z[sl] for z in nulls], mx - delay))
    out.append((keys[:0], ts[:0], [c[:0] for c in cols], None, (1 << 63) - 1))
    return out


_REFS = {}


def random_case(name):
    """(configuration, batches, Reference) of a named random case, computed once per process."""
    if name not in _REFS:
        if name == "hop":
            kw, t0 = dict(HOP_KW, key_capacity=1024, nullable_cols=(1, 2)), 0
        elif name == "cumulate":
            kw, t0 = dict(CUMULATE_KW, key_capacity=1024, nullable_cols=(1, 2)), 0
        else:                                             # "hop_shift": a shift time zone
            from helpers import load_tz_kats
            tz = {c["zone"]: c["tz"] for c in load_tz_kats()["timer"]}["Asia/Shanghai"]
            kw, t0 = dict(HOP_KW, key_capacity=1024, nullable_cols=(1, 2), tz=tz), SHIFT_T0
        batches = random_batches(t0=t0)
        _REFS[name] = (kw, batches, Reference(kw, RANDOM_AGGS, batches))
    return _REFS[name]


