"""Exact per-row reference for SUM / AVG / MIN / MAX over FLOAT and DOUBLE on non-reduce handles, its two streams and
its row comparator (tests/test_float_ref_cpu.py, tests/test_float_edges_gpu.py).

The existing oracle, run with ("COUNT", 0) alone, supplies the rows per watermark (key, window, COUNT) and the late
indices per push. Every float column of a row comes from the row's multiset of inputs: the accepted records (not in
the oracle's late indices) with the row's key and win_start <= ts < win_end that were pushed at or before the row's
watermark; its size is asserted against the oracle's COUNT for every row. Allowed lateness is 0 throughout.

Expected values, per aggregate:
  SUM / AVG  n the row's count, S the exact sum (scaled Python ints), A the exact sum of magnitudes, u = 2^-53,
             B = gamma * A with gamma = (n-1)u / (1 - (n-1)u): the error bound of n-1 double additions in any order or
             tree (adding the +0.0 identity is exact; double addition has no underflow error). SUM_F64 must lie in
             [S-B, S+B]. For AVG_F64, SUM_F32 and AVG_F32 the double ends L = nextafter(S-B, -inf) and
             H = nextafter(S+B, +inf) go through the engine's own final operations, each monotone: dv / (double)cnt
             and one (float) rounding. Nothing is measured or chosen: these bounds are the whole margin. A stream of
             exact sums (Reference(exact=True): small integers and multiples of 2^-10) has B = 0 and compares bit for
             bit, the sign of a zero sum aside. Any NaN, or +Inf with -Inf, gives NaN (any sign, any payload); +Inf
             alone +Inf; -Inf alone -Inf.
  MIN / MAX  two assertions. The engine's rule, bit for bit: the extreme under the order of the bits of the values
             widened to double (-0.0 below 0.0, a NaN with a clear sign bit above +Inf, one with a set sign bit below
             -Inf); of a NaN result only "is NaN" and the sign bit are compared (widening quiets signalling NaNs).
             Admissibility: the result is one the reference's lessThan fold (first || v < x) gives for some arrival
             order -- NaN only if the multiset holds one, else the true extreme of the non-NaN values, a zero of
             either sign when that extreme is zero and both signs occur.
"""
import fractions

import numpy as np

from flink_amd import _abi as A

Fr = fractions.Fraction
U = Fr(1, 1 << 53)
SCALE = 1074                                   # every finite double is an integer multiple of 2^-1074
SLICE = 1000
SLICES = 12
LONG_MAX = A.LONG_MAX
SUM_KINDS = ("SUM_F64", "AVG_F64", "SUM_F32", "AVG_F32")

# value columns of both streams: 0 DOUBLE, 1 FLOAT, 2 DOUBLE, 3 FLOAT
COL_DTYPES = (np.float64, np.float32, np.float64, np.float32)

KINDS = {
    "tumble": dict(window_kind="TUMBLE", semantics="TABLE", size_ms=SLICE),
    "hop": dict(window_kind="SLIDE", semantics="TABLE", size_ms=4 * SLICE, slide_ms=SLICE),
    "cumulate": dict(window_kind="CUMULATE", semantics="TABLE", size_ms=4 * SLICE, slide_ms=SLICE),
    "session150": dict(window_kind="SESSION", semantics="DATASTREAM", gap_ms=150),
    "session1000": dict(window_kind="SESSION", semantics="DATASTREAM", gap_ms=1000),
}
TABLE_KINDS = ("tumble", "hop", "cumulate")


def ord_bits(w):
    """The engine's order-preserving key of double bits (load_ord with jcmp = 0)."""
    b = np.ascontiguousarray(w, np.float64).view(np.uint64)
    return np.where((b >> np.uint64(63)) != 0, ~b, b | np.uint64(1 << 63))


def scaled(x):
    """A finite double as an integer multiple of 2^-1074."""
    num, den = float(x).as_integer_ratio()
    return num << (SCALE - (den.bit_length() - 1))


class Column:
    """One value column of a stream, widened to double, with what the expectations need per record."""

    def __init__(self, values):
        self.w = np.ascontiguousarray(values).astype(np.float64)
        self.nan = np.isnan(self.w)
        self.pinf = self.w == np.inf
        self.ninf = self.w == -np.inf
        fin = np.isfinite(self.w)
        self.sc = [scaled(x) if f else 0 for x, f in zip(self.w.tolist(), fin.tolist())]
        self.ordk = ord_bits(self.w)


class Reference:
    """Rows, late indices and row multisets of one stream under one window configuration.

    batches: [(keys, ts, cols, wm)]; wm None: no watermark step after the push. rows[b]: the oracle's rows of batch
    b's watermark sorted by (key, start, end), with `count`; members[b][i]: the global record indices of row i in
    arrival order; late[b]: the late indices of push b."""

    def __init__(self, cfg_kw, batches, exact=False):
        from oracle.oracle import Oracle
        self.exact = exact
        self.batches = batches
        self.keys = np.concatenate([b[0] for b in batches]).astype(np.int64)
        self.ts = np.concatenate([b[1] for b in batches]).astype(np.int64)
        self.cols = [np.concatenate([b[2][c] for b in batches]) for c in range(len(COL_DTYPES))]
        self._col, self._sum, self._exp = {}, {}, {}
        o = Oracle(A.make_config(aggs=[("COUNT", 0)], late_indices=True, **cfg_kw))
        groups = {}
        self.rows, self.members, self.late = [], [], []
        base = 0
        for keys, ts, cols, wm in batches:
            lo = np.zeros(0, np.int32)
            if len(keys):
                n = o.push(keys, ts, cols)
                lo = np.array(o.late_records(), copy=True)
                assert n == len(lo)
                keep = np.ones(len(keys), bool)
                keep[lo] = False
                for i in np.flatnonzero(keep).tolist():
                    groups.setdefault((int(keys[i]), int(ts[i]) // SLICE), []).append(base + i)
                base += len(keys)
            self.late.append(lo)
            if wm is None:
                self.rows.append(None)
                self.members.append(None)
                continue
            ro = o.advance_watermark(wm)
            order = np.lexsort((ro["win_end"], ro["win_start"], ro["key"]))
            rows = {"key": ro["key"][order], "win_start": ro["win_start"][order], "win_end": ro["win_end"][order],
                    "count": ro["agg0"][order]}
            mem = []
            for k, s, e, c in zip(rows["key"].tolist(), rows["win_start"].tolist(), rows["win_end"].tolist(),
                                  rows["count"].tolist()):
                idx = []
                for q in range(s // SLICE, (e - 1) // SLICE + 1):
                    idx += groups.get((k, q), ())
                idx = np.array(sorted(idx), np.int64)
                t = self.ts[idx]
                idx = idx[(t >= s) & (t < e)]
                assert len(idx) == c, ("the row's multiset differs from the oracle's COUNT", k, s, e, len(idx), c)
                mem.append(idx)
            self.rows.append(rows)
            self.members.append(mem)
        o.close()
        self.n_late = sum(len(x) for x in self.late)
        self.n_rows = sum(len(r["key"]) for r in self.rows if r is not None)

    def column(self, c):
        if c not in self._col:
            self._col[c] = Column(self.cols[c])
        return self._col[c]

    def each_row(self):
        """(batch, row index, member indices) of every row."""
        for b, mem in enumerate(self.members):
            for i, idx in enumerate(mem or ()):
                yield b, i, idx

    # ---- sums ----
    def sum_base(self, c):
        """Per batch, per row: ("nan" | "pinf" | "ninf",) or ("fin", S, A, S-B, S+B, L, H) over column c."""
        if c in self._sum:
            return self._sum[c]
        col = self.column(c)
        out = [None if mem is None else [] for mem in self.members]
        for b, i, idx in self.each_row():
            n = len(idx)
            if col.nan[idx].any() or (col.pinf[idx].any() and col.ninf[idx].any()):
                out[b].append(("nan",))
            elif col.pinf[idx].any():
                out[b].append(("pinf",))
            elif col.ninf[idx].any():
                out[b].append(("ninf",))
            else:
                terms = [col.sc[j] for j in idx.tolist()]
                S = Fr(sum(terms), 1 << SCALE)
                Aq = Fr(sum(abs(x) for x in terms), 1 << SCALE)
                if self.exact:
                    lo = hi = S
                    L = H = float(S)
                    assert Fr(L) == S, "the stream's sums are meant to be exact"
                else:
                    g = (n - 1) * U
                    B = g / (1 - g) * Aq
                    lo, hi = S - B, S + B
                    L = float(np.nextafter(float(lo), -np.inf))
                    H = float(np.nextafter(float(hi), np.inf))
                out[b].append(("fin", S, Aq, lo, hi, L, H))
        self._sum[c] = out
        return out

    def expect(self, name, c):
        """Per batch, per row: the expectation of aggregate `name` over column c (see check_value)."""
        if (name, c) in self._exp:
            return self._exp[(name, c)]
        out = [None if mem is None else [] for mem in self.members]
        if name in SUM_KINDS:
            base = self.sum_base(c)
            f32, avg = name.endswith("F32"), name.startswith("AVG")
            for b, i, idx in self.each_row():
                e = base[b][i]
                if e[0] != "fin":
                    out[b].append(e)
                    continue
                _, S, Aq, lo, hi, L, H = e
                if name == "SUM_F64":
                    out[b].append(("frac", lo, hi))
                    continue
                x, y = np.float64(L), np.float64(H)
                if avg:
                    x, y = x / np.float64(len(idx)), y / np.float64(len(idx))
                if f32:
                    with np.errstate(over="ignore"):
                        x, y = np.float32(x), np.float32(y)
                out[b].append(("range", x, y, L, H))
        else:
            col = self.column(c)
            is_min = name.startswith("MIN")
            dt = np.float32 if name.endswith("F32") else np.float64
            for b, i, idx in self.each_row():
                k = col.ordk[idx]
                ext = col.w[idx[int(np.argmin(k) if is_min else np.argmax(k))]]
                vals = col.w[idx]
                nn = vals[~np.isnan(vals)]
                te = None if len(nn) == 0 else (nn.min() if is_min else nn.max())
                signs = set(np.signbit(nn[nn == 0]).tolist()) if te == 0 else set()
                out[b].append(("ext", dt(ext), len(nn) < len(vals), te, signs, nn))
        self._exp[(name, c)] = out
        return out


def bits_of(x):
    x = np.asarray(x)
    return int(x.view(np.uint32 if x.dtype.itemsize == 4 else np.uint64))


def admissible(e, got):
    """MIN / MAX: `got` is a result the reference's lessThan fold gives for some arrival order of the multiset."""
    _, _, has_nan, te, signs, _ = e
    if np.isnan(got):
        return has_nan
    if te is None or got != te:
        return False
    return te != 0 or bool(np.signbit(got)) in signs


def check_value(name, e, got, mode="engine"):
    """None if `got` meets expectation e of aggregate `name`, else what is wrong. mode "engine": every check; "oracle":
    the checks an order-dependent fold in arrival order must meet (sums of the double kinds; MIN / MAX bit for bit
    only where the multiset has neither a NaN nor both zeros, admissible everywhere); "oracle_merged": the oracle on
    session windows, where a window merged from several folds their accumulators -- with a NaN among the values the
    result may then be the extreme of a part of them (a NaN accumulator loses every comparison of the merge), which
    no single fold gives. The engine is never checked in that mode."""
    if e[0] == "nan":
        return None if np.isnan(got) else "expected NaN"
    if e[0] in ("pinf", "ninf"):
        want = np.inf if e[0] == "pinf" else -np.inf
        return None if got == want else "expected %s" % want
    if e[0] == "frac":
        if not np.isfinite(got) or not (e[1] <= Fr(float(got)) <= e[2]):
            return "outside [S-B, S+B] = [%r, %r]" % (float(e[1]), float(e[2]))
        return None
    if e[0] == "range":
        _, x, y, L, H = e
        if not (x <= got <= y):                       # (a NaN fails both comparisons)
            return "outside [%r, %r]" % (x, y)
        if got == 0 and ((L > 0 and np.signbit(got)) or (H < 0 and not np.signbit(got))):
            return "a zero of the wrong sign for a sum in [%r, %r]" % (L, H)
        return None
    _, want, has_nan, te, signs, nn = e
    if mode == "oracle_merged" and has_nan and not np.isnan(got) and (nn == got).any():
        return None      # a session merged from sessions folds their accumulators: the extreme of a part of the values
    if not admissible(e, got):
        return "not a result of the reference's fold in any arrival order (true extreme %r, NaN present: %s)" % (te, has_nan)
    if mode != "engine" and (has_nan or len(signs) == 2):
        return None
    if np.isnan(want):
        ok = np.isnan(got) and bool(np.signbit(got)) == bool(np.signbit(want))
    else:
        ok = bits_of(got) == bits_of(want)
    return None if ok else "the bit order gives %r (bits %#x)" % (want, bits_of(want))


def compare_rows(got, ref, b, aggs, ctx="", mode="engine", only=None):
    """Fired rows `got` of batch b's watermark against the reference: the same (key, window) set, COUNT bit-exact,
    every float aggregate of every row by check_value. Returns the number of rows."""
    want = ref.rows[b]
    n = len(want["key"])
    order = np.lexsort((got["win_end"], got["win_start"], got["key"]))
    for f in ("key", "win_start", "win_end"):
        x = np.asarray(got[f])[order]
        assert len(x) == n and np.array_equal(x, want[f]), "%s batch %d: column %s differs (%d rows, expected %d)" % (
            ctx, b, f, len(x), n)
    for j, (name, c) in enumerate(aggs):
        if only is not None and name not in only:
            continue
        assert "null%d" % j not in got
        x = np.asarray(got["agg%d" % j])[order]
        if name == "COUNT":
            assert np.array_equal(x, want["count"]), "%s batch %d: COUNT differs" % (ctx, b)
            continue
        assert x.dtype == np.dtype(A.AGG_RESULT_DTYPE[name])
        exp = ref.expect(name, c)[b]
        for i in range(n):
            why = check_value(name, exp[i], x[i], mode)
            assert why is None, "%s batch %d key %d window [%d, %d) %s(col %d) over %d values: got %r (bits %#x): %s" % (
                ctx, b, want["key"][i], want["win_start"][i], want["win_end"][i], name, c, want["count"][i], x[i],
                bits_of(x[i]), why)
    return n


def run_engine(g, ref, aggs, first=0, last=None, device=False, ctx="", after_push=None):
    """Push batches[first:last] of the reference's stream through the handle g: late indices after every push and
    every row after every watermark must meet the reference. Returns the rows compared."""
    rows = 0
    batches = ref.batches
    for b in range(first, len(batches) if last is None else last):
        keys, ts, cols, wm = batches[b]
        if len(keys):
            if device:
                import torch
                dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
                dg = g.push(dev(keys), dev(ts), [dev(c) for c in cols])
            else:
                dg = g.push(keys, ts, cols)
            assert np.array_equal(g.late_records(), ref.late[b]), "%s late indices differ (batch %d)" % (ctx, b)
            assert dg == len(ref.late[b])
            if after_push is not None:
                after_push(g)
        if wm is not None:
            rows += compare_rows(g.advance_watermark(wm), ref, b, aggs, ctx)
    return rows


# ---- the two streams ----

SEED_KEY = 1 << 20


def _arrange(rng, keys, ts, cols, pushes, jitter, delay, seed):
    """Arrival order = event time displaced by up to `jitter` ms (with a seed push: one record in fifty by 3 to 6 s
    more); `pushes` pushes, each followed by a watermark `delay` under the newest timestamp so far, then end of input.
    seed: a first push of one record per slice (value 1) with no watermark step, so that every slice exists when the
    next push is partitioned."""
    n = len(keys)
    shift = rng.integers(0, jitter + 1, n)
    if seed:
        shift = shift + np.where(rng.random(n) < 0.02, rng.integers(3000, 6001, n), 0)
    order = np.argsort(ts + shift, kind="stable")
    keys, ts, cols = keys[order], ts[order], [c[order] for c in cols]
    out = []
    if seed:
        st = np.arange(SLICES, dtype=np.int64) * SLICE + 1
        out.append((np.full(SLICES, SEED_KEY, np.int64), st, [np.ones(SLICES, dt) for dt in COL_DTYPES], None))
    per, mx = -(-n // pushes), -(1 << 63)
    for b in range(pushes):
        sl = slice(b * per, min(n, (b + 1) * per))
        mx = max(mx, int(ts[sl].max()))
        out.append((keys[sl], ts[sl], [c[sl] for c in cols], mx - delay))
    out.append((keys[:0], ts[:0], [c[:0] for c in cols], LONG_MAX))
    return out, (keys, ts, cols)


JITTER = 1500
FINITE_KEYS = 300
FINITE_CLASSES = ("cancel_in_slice", "cancel_across_slices", "subnormal", "near_flt_max", "generic")


def finite_records(seed=5, n=11_000):
    """About 2^14 records of 300 keys over 12 slices of 1 s; class = key % 5:
      0 cancelling pairs in one (key, slice): +x and -x of magnitude 1e6..1e12 next to loners of 1e-12..1e-3;
      1 the same pairs one to three slices apart (inside one HOP / CUMULATE window, in different TUMBLE windows);
      2 double and float subnormals only;
      3 FLOAT values of 1e38..3.4e38, four in five positive: the float-order sum overflows, the double sum does not
        (or passes FLT_MAX and rounds to Inf);
      4 magnitudes 1e-12..1e12, a few of them zeros of either sign."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, FINITE_KEYS, n).astype(np.int64)
    ts = rng.integers(0, SLICES * SLICE, n).astype(np.int64)
    cls = keys % 5
    loner = rng.random(n) < 0.3
    paired = (cls <= 1) & ~loner
    pts = np.where(cls == 0, ts // SLICE * SLICE + rng.integers(0, SLICE, n), ts + SLICE * rng.integers(1, 4, n))
    pts = np.where(pts >= SLICES * SLICE, ts, pts)                     # (no slice behind the last: the pair stays here)
    cols = []
    for dt in COL_DTYPES:
        sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
        v = sign * 10.0 ** rng.uniform(-12, 12, n)
        v = np.where(paired, sign * 10.0 ** rng.uniform(6, 12, n), v)
        v = np.where((cls <= 1) & loner, sign * 10.0 ** rng.uniform(-12, -3, n), v)
        zero = (cls == 4) & (rng.random(n) < 0.05)
        v = np.where(zero, np.where(rng.random(n) < 0.5, -0.0, 0.0), v)
        v = v.astype(dt)
        sub = cls == 2
        if dt is np.float64:
            tiny = rng.integers(1, 1 << 40, n).astype(np.uint64).view(np.float64)
        else:
            tiny = rng.integers(1, 1 << 20, n).astype(np.uint32).view(np.float32)
            big = (rng.uniform(1e38, 3.4e38, n) * np.where(rng.random(n) < 0.8, 1.0, -1.0)).astype(np.float32)
            v = np.where(cls == 3, big, v)
        v = np.where(sub, tiny * sign.astype(dt), v).astype(dt)
        cols.append(v)
    pk, pt = keys[paired], pts[paired]
    keys = np.concatenate([keys, pk])
    ts = np.concatenate([ts, pt])
    cols = [np.concatenate([v, -v[paired]]) for v in cols]
    return rng, keys, ts, cols


SPECIAL_CLASSES = ("nan_first", "nan_middle", "nan_last", "all_nan", "nan_sign_set", "nan_payload", "pos_inf",
                   "neg_inf", "both_inf", "only_neg_zero", "zeros_pos_first", "zeros_neg_first", "clean",
                   "nan_in_slice_5", "neg_inf_in_slice_3", "nan_sign_set_in_slice_1")
SPECIAL_KEYS_PER_CLASS = 24
CONFINED = {"nan_in_slice_5": 5, "neg_inf_in_slice_3": 3, "nan_sign_set_in_slice_1": 1}
_NAN = {np.float64: (0x7ff8000000000000, 0xfff8000000000000, 0x7ff8000000000123),
        np.float32: (0x7fc00000, 0xffc00000, 0x7fc00123)}


def special_records(seed=6):
    """16 key classes (key % 16, 24 keys each), 3 or 4 records per (key, slice) over 12 slices. Finite values are
    multiples of 2^-10 below 2^10 in magnitude, so every finite sum is exact in any order. The class plants its special
    value by arrival rank inside each (key, slice): see SPECIAL_CLASSES; the last three classes only in one slice."""
    rng = np.random.default_rng(seed)
    nk = len(SPECIAL_CLASSES) * SPECIAL_KEYS_PER_CLASS
    per = rng.integers(3, 5, nk * SLICES)
    gid = np.repeat(np.arange(nk * SLICES), per)
    keys = (gid // SLICES).astype(np.int64)
    ts = (gid % SLICES) * SLICE + rng.integers(0, SLICE, len(gid)).astype(np.int64)
    return rng, keys, ts


def _plant(keys, ts, rng):
    """Value columns of the special stream for records already in arrival order."""
    n = len(keys)
    gid = keys * SLICES + ts // SLICE
    o = np.argsort(gid, kind="stable")
    sg = gid[o]
    start = np.r_[True, sg[1:] != sg[:-1]]
    first = np.maximum.accumulate(np.where(start, np.arange(n), 0))
    rank = np.empty(n, np.int64)
    rank[o] = np.arange(n) - first
    size = np.bincount(gid)[gid]
    cls = keys % len(SPECIAL_CLASSES)
    q = ts // SLICE
    last = rank == size - 1
    is_ = lambda name: cls == SPECIAL_CLASSES.index(name)              # noqa: E731
    cols = []
    for dt in COL_DTYPES:
        ut = np.uint64 if dt is np.float64 else np.uint32
        nan, nnan, pnan = (np.array([x], ut).view(dt)[0] for x in _NAN[dt])
        v = (rng.integers(-(1 << 20), 1 << 20, n) / 1024.0).astype(dt)
        v[is_("nan_first") & (rank == 0)] = nan
        v[is_("nan_middle") & (rank == 1)] = nan
        v[is_("nan_last") & last] = nan
        v[is_("all_nan")] = nan
        v[is_("nan_sign_set") & (rank == 1)] = nnan
        v[is_("nan_payload") & (rank == 0)] = pnan
        v[is_("pos_inf") & (rank == 1)] = np.inf
        v[is_("neg_inf") & (rank == 1)] = -np.inf
        v[is_("both_inf") & (rank == 0)] = np.inf
        v[is_("both_inf") & last] = -np.inf
        v[is_("only_neg_zero")] = -0.0
        v[is_("zeros_pos_first")] = np.where(rank % 2 == 0, 0.0, -0.0).astype(dt)[is_("zeros_pos_first")]
        v[is_("zeros_neg_first")] = np.where(rank % 2 == 0, -0.0, 0.0).astype(dt)[is_("zeros_neg_first")]
        v[is_("nan_in_slice_5") & (q == 5) & (rank == 1)] = nan
        v[is_("neg_inf_in_slice_3") & (q == 3) & (rank == 0)] = -np.inf
        v[is_("nan_sign_set_in_slice_1") & (q == 1) & last] = nnan
        cols.append(v)
    return cols


def holds_special(name, w):
    """Whether a row's multiset w (double, arrival order) shows the special value of class `name`."""
    nan = np.isnan(w)
    if name == "nan_first":
        return bool(nan[0])
    if name == "nan_last":
        return bool(nan[-1])
    if name == "nan_middle":
        return bool(nan[1:-1].any()) and not nan[0] and not nan[-1]
    if name == "all_nan":
        return bool(nan.all())
    if name in ("nan_sign_set", "nan_sign_set_in_slice_1"):
        return bool((nan & np.signbit(w)).any())
    if name == "nan_payload":
        return bool((nan & ((w.view(np.uint64) & np.uint64((1 << 51) - 1)) != 0)).any())
    if name == "nan_in_slice_5":
        return bool(nan.any())
    if name == "pos_inf":
        return bool((w == np.inf).any()) and not (w == -np.inf).any()
    if name in ("neg_inf", "neg_inf_in_slice_3"):
        return bool((w == -np.inf).any()) and not (w == np.inf).any()
    if name == "both_inf":
        return bool((w == np.inf).any() and (w == -np.inf).any())
    zero = w == 0
    if name == "only_neg_zero":
        return bool((zero & np.signbit(w)).all())
    if name in ("zeros_pos_first", "zeros_neg_first"):
        return bool(zero.all()) and len(set(np.signbit(w).tolist())) == 2 and \
            bool(np.signbit(w[0])) == (name == "zeros_neg_first")
    return bool(np.isfinite(w).all())                                   # "clean"


def stream_batches(stream, kind):
    """The batches of a stream for a window kind. Table kinds: a seed push, then 4 pushes with watermarks 0.2 s under
    the newest timestamp (displacement up to 1.5 s, a few records up to 7.5 s: every kind drops records as late, HOP and
    CUMULATE also accept records behind windows that fired). Sessions: no seed, watermarks under every displaced
    record (no late record: the cell paths take only order-free pushes)."""
    table = kind in TABLE_KINDS
    if stream == "finite":
        rng, keys, ts, cols = finite_records()
        return _arrange(rng, keys, ts, cols, 4, JITTER, 200 if table else JITTER + 1, table)[0]
    rng, keys, ts = special_records()
    dummy = [np.zeros(len(keys), dt) for dt in COL_DTYPES]
    out, (k, t, _) = _arrange(rng, keys, ts, dummy, 4, JITTER, 200 if table else JITTER + 1, table)
    cols = _plant(k, t, rng)
    res, at = [], 0
    for bk, bt, bc, wm in out:
        if wm is None or len(bk) == 0:
            res.append((bk, bt, bc, wm))
            continue
        sl = slice(at, at + len(bk))
        at += len(bk)
        res.append((bk, bt, [c[sl] for c in cols], wm))
    return res


_REFS = {}


def case(stream, kind):
    """(configuration keywords, Reference) of a stream ("finite" / "special") under a window kind of KINDS, computed
    once per process."""
    if (stream, kind) not in _REFS:
        # (a key table of 2^13 slots: at least two combiner partitions for every aggregate list, so that a push of one
        # partition3 tile does not overfill a sub-bucket and send its tail to the replay)
        kw = dict(KINDS[kind], key_capacity=4096)
        _REFS[(stream, kind)] = (kw, Reference(kw, stream_batches(stream, kind), exact=stream == "special"))
    return _REFS[(stream, kind)]


def straggler_case(n=16 * 4096 - 1, nkeys=3000, seed=9):
    """One TUMBLE push of n records over 6 slices in event-time order whose last third returns to the first slice,
    behind a seed push; exact values with a NaN, an infinity or a -0.0 in one record of a hundred."""
    if "straggler" not in _REFS:
        rng = np.random.default_rng(seed)
        keys = rng.integers(0, nkeys, n).astype(np.int64)
        ts = np.sort(rng.integers(0, 6 * SLICE, n)).astype(np.int64)
        tail = n // 3
        ts[-tail:] = rng.integers(0, SLICE, tail)
        cols = []
        for dt in COL_DTYPES:
            v = (rng.integers(-(1 << 20), 1 << 20, n) / 1024.0).astype(dt)
            r = rng.random(n)
            ut = np.uint64 if dt is np.float64 else np.uint32
            v[r < 0.002] = np.array([_NAN[dt][0]], ut).view(dt)[0]
            v[(r >= 0.002) & (r < 0.004)] = np.array([_NAN[dt][1]], ut).view(dt)[0]
            v[(r >= 0.004) & (r < 0.006)] = np.inf
            v[(r >= 0.006) & (r < 0.008)] = -np.inf
            v[(r >= 0.008) & (r < 0.012)] = -0.0
            cols.append(v)
        st = np.arange(6, dtype=np.int64) * SLICE + 1
        batches = [(np.full(6, SEED_KEY, np.int64), st, [np.ones(6, dt) for dt in COL_DTYPES], None),
                   (keys, ts, cols, LONG_MAX)]
        kw = dict(KINDS["tumble"], key_capacity=4096)
        _REFS["straggler"] = (kw, Reference(kw, batches, exact=True))
    return _REFS["straggler"]
