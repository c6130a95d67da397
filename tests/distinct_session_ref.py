"""Reference for COUNT / SUM / AVG(DISTINCT col) over Table SESSION windows (FWA_CFG_DISTINCT_SESSION), shared by the
distinct-session tests. It never calls the engine.

Every column but the distinct ones comes from the existing oracle, run on the same stream with ("COUNT", 0) in place of
every distinct aggregate: the rows per watermark, the late drops and late_records() per push. The distinct columns come
from distinct_range_ref.BruteForce / distinct_sum_ref.range_expected_rows: for a fired row (key, start, end) they take
the accepted records of the key with start <= local ts < end that no earlier fired row has taken (SessionBrute). The
last condition is needed: a record that is late on its own but is saved by a session in flight moves that session's
start back, possibly below the records of a session of the key that has already fired (gap 500: [21224, 21724) fires
at watermark 21914; then 21532 is accepted and 21100 is saved by it, and [21100, 22032) spans the fired 21224). Records
of other sessions in flight are more than a gap away and never fall into [start, end). range_expected_rows recomputes
every row's COUNT(*) this way and asserts that it equals the oracle's before a distinct column is trusted.

The reference also counts what makes a stream a test of the cell bitmap (cell = floor(local ts / gap), block = cell >> 6):
  a  rows whose distinct count is below their number of (value, cell) pairs (the union is taken, not a sum of cells)
  b  rows whose cell range spans at least 3 blocks with one value present in the first and in the last block
  c  steps that fire at least 2 sessions of one key inside one block
  d  accepted records whose cell holds a record of a session of the same key that fired earlier (clear at the fire)
  e  dropped records whose (key, value) occurs in no accepted record of their cell, where an accepted record of the key
     arrives in that cell later (no bits for dropped records)
  f  records accepted only because an in-flight session saved them (their own window had already passed the watermark)

CellModel is a pure-Python model of what the engine keeps: a set of cells per (key, column, value), marked behind the
ingest for accepted records only and cleared at the fire. Either rule can be switched off to show that it is needed.
"""
import numpy as np

from distinct_range_ref import tz_local
from distinct_sum_ref import (SumBruteForce, assert_sum_rows_equal, distinct_result, is_distinct, is_sum,
                              range_aggs, range_expected_rows)
from flink_amd import _abi as A

LONG_MIN = -(1 << 63)


def session_cfg(cfg_kw, aggs, late_indices=True, **more):
    kw = dict(cfg_kw, **more)
    nullable = tuple(kw.pop("nullable_cols", ()))
    return A.make_config(aggs=list(aggs), nullable_cols=nullable, late_indices=late_indices, distinct_session=True, **kw)


def cells_of_row(start, end, gap):
    """The cell range of the session [start, end): its records lie in [start, end - gap]."""
    return start // gap, (end - gap) // gap


class SessionBrute(SumBruteForce):
    """The accepted records so far; a window [start, end) of a key holds those no fired row has taken yet."""

    def __init__(self, *a):
        super().__init__(*a)
        self.fired = np.zeros(0, bool)                    # per accepted record: its session has fired

    def add(self, keys, ts, cols, nulls=None, late=()):
        super().add(keys, ts, cols, nulls, late)
        self.fired = np.concatenate([self.fired, np.zeros(len(self.keys) - len(self.fired), bool)])

    def _in(self, key, start, end):
        idx = super()._in(key, start, end)
        return idx[~self.fired[idx]]


class SessionReference:
    """Per batch [(keys, ts, cols, nulls or None, watermark)]: the expected rows of its watermark and the late indices of
    its push; `counters` holds a .. f; live_tuples() the (key, value, cell, column) tuples of the sessions in flight."""

    def __init__(self, cfg_kw, aggs, batches):
        from oracle.oracle import Oracle
        raggs, dcols = range_aggs(aggs)
        kw = {k: v for k, v in cfg_kw.items() if k != "output_on_device"}
        nullable = tuple(kw.pop("nullable_cols", ()))
        o = Oracle(A.make_config(aggs=raggs, nullable_cols=nullable, late_indices=True, **kw))
        self.aggs = [tuple(s) for s in aggs]
        self.names = [s[0] for s in aggs]
        self.dcols = dcols
        self.gap = gap = int(kw["gap_ms"])
        self.tz = kw.get("tz")
        self.brute = SessionBrute(dcols, self.tz, gap, 0)
        self.stats = {"rows": 0, "union": 0, "differ": 0, "null": 0}
        self.counters = dict.fromkeys("abcdef", 0)
        self.rows, self.late = [], []
        fired_cells = set()                               # (key, cell) of the records of fired sessions
        dropped = []                                      # (push, index, key, cell, {column: value bits or None})
        accepted = []                                     # (push, index, key, cell)
        wm_prev = LONG_MIN
        for b, (keys, ts, cols, nulls, wm) in enumerate(batches):
            lo = np.zeros(0, np.int32)
            if len(keys):
                n = o.push(keys, ts, cols, nulls=nulls)
                lo = np.array(o.late_records(), copy=True)
                assert n == len(lo)
                self.brute.add(keys, ts, cols, nulls, lo)
                lts = tz_local(ts, self.tz)
                lwm = LONG_MIN if wm_prev == LONG_MIN else int(tz_local([wm_prev], self.tz)[0])
                late = set(int(i) for i in lo)
                for i in range(len(keys)):
                    k, c = int(keys[i]), int(lts[i]) // gap
                    if i in late:
                        vals = {}
                        for col in dcols:
                            z = nulls is not None and nulls[col] is not None and nulls[col][i]
                            vals[col] = None if z else int(np.ascontiguousarray(cols[col]).view(np.int64)[i])
                        dropped.append((b, i, k, c, vals))
                        continue
                    accepted.append((b, i, k, c))
                    self.counters["d"] += (k, c) in fired_cells
                    self.counters["f"] += lwm != LONG_MIN and int(lts[i]) + gap - 1 <= lwm
            ro = o.advance_watermark(wm)
            wm_prev = max(wm_prev, wm)
            self.rows.append(range_expected_rows(ro, self.aggs, self.brute, self.stats))
            self.late.append(lo)
            self._count_rows(ro, fired_cells)
        o.close()
        self._count_dropped(dropped, accepted)
        self.n_late = sum(len(x) for x in self.late)
        self.n_rows = self.stats["rows"]

    def _count_rows(self, ro, fired_cells):
        gap, bf = self.gap, self.brute
        blocks = {}
        for i in range(len(ro["key"])):
            k, s, e = int(ro["key"][i]), int(ro["win_start"][i]), int(ro["win_end"][i])
            c_lo, c_hi = cells_of_row(s, e, gap)
            idx = bf._in(k, s, e)
            assert len(idx), "a fired row without records"
            cells = bf.lts[idx] // gap
            assert cells.min() == c_lo and cells.max() == c_hi, "the session's cells are not [start / g, (end - g) / g]"
            bf.fired[idx] = True
            fired_cells.update((k, int(c)) for c in cells)
            union = span = False
            for col in self.dcols:
                ok = ~bf.nul[col][idx]
                bits, cc = bf.bits[col][idx][ok], cells[ok]
                union |= len(np.unique(bits)) < len(set(zip(bits.tolist(), cc.tolist())))
                if (c_hi >> 6) - (c_lo >> 6) >= 2:
                    first = set(bits[(cc >> 6) == (c_lo >> 6)].tolist())
                    span |= bool(first & set(bits[(cc >> 6) == (c_hi >> 6)].tolist()))
            self.counters["a"] += union
            self.counters["b"] += span
            for B in range(c_lo >> 6, (c_hi >> 6) + 1):
                blocks[(k, B)] = blocks.get((k, B), 0) + 1
        self.counters["c"] += any(v >= 2 for v in blocks.values())

    def _count_dropped(self, dropped, accepted):
        bf, gap = self.brute, self.gap
        have = set()                                      # (key, cell, column, value) of the accepted records
        cells = bf.lts // gap
        for col in self.dcols:
            ok = ~bf.nul[col]
            have |= set(zip(bf.keys[ok].tolist(), cells[ok].tolist(), [col] * int(ok.sum()), bf.bits[col][ok].tolist()))
        last = {}                                         # (key, cell) -> the last (push, index) accepted there
        for b, i, k, c in accepted:
            last[(k, c)] = max(last.get((k, c), (-1, -1)), (b, i))
        for b, i, k, c, vals in dropped:
            if last.get((k, c), (-1, -1)) > (b, i):
                self.counters["e"] += any(v is not None and (k, c, col, v) not in have for col, v in vals.items())

    def live_tuples(self):
        """(key, value bits, cell, column ordinal) of the non-NULL values of the sessions in flight."""
        bf, out = self.brute, set()
        cells = bf.lts // self.gap
        for d, col in enumerate(self.dcols):
            m = ~bf.fired & ~bf.nul[col]
            out |= set(zip(bf.keys[m].tolist(), bf.bits[col][m].tolist(), cells[m].tolist(), [d] * int(m.sum())))
        return out


class CellModel:
    """What the engine keeps, in Python: per (key, column, value bits) the set of cells it occurred in. drop_filter: the
    dropped records of a push set no bits (the marking pass runs behind the ingest). clear: a fired session's cells are
    removed at its fire."""

    def __init__(self, ref, drop_filter=True, clear=True):
        self.ref, self.drop_filter, self.clear = ref, drop_filter, clear
        self.cells = {}

    def mark(self, keys, ts, cols, nulls, late):
        lts = tz_local(ts, self.ref.tz)
        late = set(int(i) for i in late) if self.drop_filter else set()
        for i in range(len(keys)):
            if i in late:
                continue
            for col in self.ref.dcols:
                if nulls is not None and nulls[col] is not None and nulls[col][i]:
                    continue
                v = int(np.ascontiguousarray(cols[col]).view(np.int64)[i])
                self.cells.setdefault((int(keys[i]), col, v), set()).add(int(lts[i]) // self.ref.gap)

    def fire(self, ro):
        """The reference's rows `ro` with the distinct columns taken from the cell sets, then the clear."""
        ref = self.ref
        out = {f: ro[f] for f in ("key", "win_start", "win_end")}
        n = len(ro["key"])
        ranges = [cells_of_row(int(ro["win_start"][i]), int(ro["win_end"][i]), ref.gap) for i in range(n)]
        for j, (name, col) in enumerate(ref.aggs):
            if not is_distinct(name):
                out["agg%d" % j] = ro["agg%d" % j]
                if "null%d" % j in ro:
                    out["null%d" % j] = ro["null%d" % j]
                continue
            out["agg%d" % j] = np.zeros(n, A.AGG_RESULT_DTYPE[name])
            if is_sum(name):
                out["null%d" % j] = np.zeros(n, np.uint8)
            for i in range(n):
                k, (c_lo, c_hi) = int(ro["key"][i]), ranges[i]
                bits = [v for (kk, cc, v), cs in self.cells.items()
                        if kk == k and cc == col and any(c_lo <= c <= c_hi for c in cs)]
                val, z = distinct_result(name, np.array(bits, np.int64))
                out["agg%d" % j][i] = val
                if is_sum(name):
                    out["null%d" % j][i] = z
        if self.clear:
            for i in range(n):
                k, (c_lo, c_hi) = int(ro["key"][i]), ranges[i]
                for (kk, _, _), cs in self.cells.items():
                    if kk == k:
                        cs.difference_update([c for c in cs if c_lo <= c <= c_hi])
        return out


def model_matches(ref, batches, **rules):
    """True iff the cell model under `rules` gives the reference's rows at every watermark."""
    m = CellModel(ref, **rules)
    for b, (keys, ts, cols, nulls, wm) in enumerate(batches):
        if len(keys):
            m.mark(keys, ts, cols, nulls, ref.late[b])
        try:
            assert_sum_rows_equal(m.fire(ref.rows[b]), ref.rows[b], ref.names)
        except AssertionError:
            return False
    return True


def check_engine(g, ref, batches, first=0, last=None, device=False, late=True, flags=0):
    """Push batches[first:last] through the handle `g`: rows after every watermark, the late drops of every push and
    (late: the handle was configured with late_indices) its late indices must equal the reference's. Returns the rows."""
    rows = 0
    for b in range(first, len(batches) if last is None else last):
        keys, ts, cols, nulls, wm = batches[b]
        if len(keys):
            if device:
                import torch
                dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
                keep = (dev(keys), dev(ts), [dev(c) for c in cols], None if nulls is None else [dev(z) for z in nulls])
                dg = g.push(keep[0], keep[1], keep[2], nulls=keep[3])
            else:
                dg = g.push(keys, ts, cols, nulls=nulls)
            assert dg == len(ref.late[b]), "late drops differ (batch %d): %d vs %d" % (b, dg, len(ref.late[b]))
            if late:
                assert np.array_equal(g.late_records(), ref.late[b]), "late indices differ (batch %d)" % b
        rg = g.advance_watermark(wm)
        assert_sum_rows_equal(rg, ref.rows[b], ref.names, ctx="batch %d wm=%d" % (b, wm))
        rows += len(rg["key"])
    return rows


# ---- the random streams of tests/test_distinct_session_gpu.py (their reference alone: test_distinct_session_cpu.py) ----

# columns: 0 BIGINT (plain), 1 BIGINT of 8 values, 2 DOUBLE of 8 exactly summable values, 3 DOUBLE (plain)
AGGS_COUNT = [("COUNT", 0), ("COUNT_DISTINCT", 1)]
AGGS_ALL = [("COUNT_DISTINCT", 1), ("SUM_DISTINCT_I64", 1), ("AVG_DISTINCT_I64", 1), ("SUM_DISTINCT_F64", 2),
            ("AVG_DISTINCT_F64", 2), ("SUM_I64", 0), ("MAX_F64", 3)]
AGGS_NULLS = [("COUNT", 0), ("COUNT_DISTINCT", 1), ("SUM_DISTINCT_I64", 1), ("COUNT_DISTINCT", 2), ("SUM_DISTINCT_F64", 2)]
SHIFT_T0 = 1615593600000


def random_batches(seed, gap, t0=0, pushes=8, n=3000, nkeys=50, nvals=8, null_p=0.0, dense=0, disorder=3.0):
    """n records of nkeys keys over 60 gaps per key's share (so a key's sessions keep splitting and merging), sorted and
    then moved back by up to 3 gaps, in `pushes` pushes each followed by a watermark one gap under the newest timestamp
    (the oldest displaced records are dropped unless an in-flight session saves them), then end of input. dense: that
    many keys also get a run of 225 records 2 ms apart (sessions of 450 ms: three blocks and more at gap 3). disorder:
    the displacement in gaps; under 1 nothing is late, so every push is order-free and can take a cell path. Column 1
    (and 2) NULL with probability null_p; key nkeys - 1 has NULLs only."""
    rng = np.random.default_rng(seed)
    span = 60 * gap * max(1, n // (60 * nkeys))
    keys = rng.integers(0, nkeys, n).astype(np.int64)
    ts = np.sort(rng.integers(0, span, n)).astype(np.int64) - rng.integers(0, int(disorder * gap) + 1, n)
    if dense:
        dk = np.repeat(np.arange(dense, dtype=np.int64), 225)
        dt = np.tile(np.arange(0, 450, 2, dtype=np.int64), dense) + np.repeat(rng.integers(0, span // 4, dense), 225)
        keys, ts = np.concatenate([keys, dk]), np.concatenate([ts, dt])
        order = np.argsort(ts + rng.integers(0, int(disorder * gap) + 1, len(ts)), kind="stable")
        keys, ts = keys[order], ts[order]
        n = len(keys)
    ts = ts + t0
    cols = [rng.integers(-1000, 1000, n).astype(np.int64), rng.integers(0, nvals, n).astype(np.int64) * 1000003 - 7,
            (rng.integers(-nvals // 2, nvals // 2, n) * 0.25).astype(np.float64), rng.normal(size=n)]
    nulls = [None, None, None, None]
    if null_p:
        nulls[1] = ((rng.random(n) < null_p) | (keys == nkeys - 1)).astype(np.uint8)
        nulls[2] = (rng.random(n) < null_p).astype(np.uint8)
    per, mx, out = (n + pushes - 1) // pushes, LONG_MIN, []
    for b in range(pushes):
        sl = slice(b * per, min((b + 1) * per, n))
        mx = max(mx, int(ts[sl].max()))
        out.append((keys[sl], ts[sl], [c[sl] for c in cols], None if not null_p else [None if z is None else z[sl] for z in nulls],
                    mx - gap))
    out.append((keys[:0], ts[:0], [c[:0] for c in cols], None, (1 << 63) - 1))
    return out


SESSION_KW = dict(window_kind="SESSION", semantics="TABLE", key_capacity=1024)
# name -> (gap, aggregates, generator arguments); the seeds are fixed so that the counters hold (asserted on the CPU)
CASES = {
    "g50_count": (50, AGGS_COUNT, dict(seed=20)),
    "g500_all": (500, AGGS_ALL, dict(seed=12)),
    "g50_nulls": (50, AGGS_NULLS, dict(seed=23, null_p=0.3)),
    "g3_blocks": (3, AGGS_COUNT, dict(seed=14, dense=3)),
    # nothing late: the pushes are order-free (the cell paths take them)
    "g50_ordered": (50, AGGS_ALL, dict(seed=17, disorder=0.4)),
    "g3_ordered": (3, AGGS_COUNT, dict(seed=18, dense=3, disorder=0.4)),
    # a shift time zone, the stream crossing a transition: +1 h (Asia/Shanghai 1991-04-14), -1 h (Los Angeles 2021-11-07)
    "g500_shanghai": (500, AGGS_ALL, dict(seed=15, t0=671565600000 - 15000, zone="Asia/Shanghai")),
    "g500_los_angeles": (500, AGGS_COUNT, dict(seed=16, t0=1636275600000 - 15000, zone="America/Los_Angeles")),
}
RANDOM = ("g50_count", "g500_all", "g50_nulls", "g3_blocks")   # the streams whose counters a .. f are asserted
_REFS = {}


def random_case(name):
    """(configuration, aggregates, batches, SessionReference) of a named random case, computed once per process."""
    if name not in _REFS:
        gap, aggs, gen = CASES[name]
        gen = dict(gen)
        kw = dict(SESSION_KW, gap_ms=gap)
        zone = gen.pop("zone", None)
        if zone:
            from helpers import load_tz_kats
            kw["tz"] = {c["zone"]: c["tz"] for c in load_tz_kats()["timer"]}[zone]
        if gen.get("null_p"):
            kw["nullable_cols"] = (1, 2)
        batches = random_batches(gap=gap, **gen)
        _REFS[name] = (kw, aggs, batches, SessionReference(kw, aggs, batches))
    return _REFS[name]
