"""Reference for COUNT(DISTINCT col) over TUMBLE windows, shared by the distinct tests.

COUNT(DISTINCT c) of a (key, window) equals SUM(BIGINT) over the column "this record is the first occurrence of its
(key, window, value) in arrival order" (0 for NULL values). Within a window acceptance only ever turns off (the
watermark only grows), so the first occurrence is accepted whenever any occurrence is: the existing oracle, run with
SUM_I64 over that column in place of the distinct aggregate, gives the rows, the late drops and the late indices.
"""
import numpy as np

from flink_amd import _abi as A
from helpers import assert_rows_equal


def tz_local(ts, tz):
    """Local wall-clock millis of epoch instants under a shift time zone [(utc_instant_ms, offset_ms), ...]."""
    ts = np.asarray(ts, np.int64)
    if not tz:
        return ts
    inst = np.array([p[0] for p in tz], np.int64)
    offs = np.array([p[1] for p in tz], np.int64)
    idx = np.clip(np.searchsorted(inst, ts, side="right") - 1, 0, None)
    return ts + offs[idx]


class FirstOccurrence:
    """The 0/1 first-occurrence column per (key, window, value), carried across pushes."""

    def __init__(self, size_ms, offset_ms=0, tz=None):
        self.size, self.off, self.tz = int(size_ms), int(offset_ms), tz
        self.seen = set()

    def windows(self, ts):
        return (tz_local(ts, self.tz) - self.off) // self.size      # floor division

    def mark(self, keys, ts, vals, nulls=None):
        keys = np.asarray(keys, np.int64)
        bits = np.ascontiguousarray(vals).view(np.int64)
        w = self.windows(ts)
        out = np.zeros(len(keys), np.int64)
        for i in range(len(keys)):
            if nulls is not None and nulls[i]:
                continue
            t = (int(keys[i]), int(w[i]), int(bits[i]))
            if t not in self.seen:
                self.seen.add(t)
                out[i] = 1
        return out


def reference_aggs(aggs, ncols):
    """aggs with every COUNT_DISTINCT(c) replaced by SUM_I64 over an appended column; returns (aggs', {c: column'})."""
    cols, out = {}, []
    for spec in aggs:
        if spec[0] == "COUNT_DISTINCT":
            cols.setdefault(spec[1], ncols + len(cols))
            out.append(("SUM_I64", cols[spec[1]]))
        else:
            out.append(tuple(spec))
    return out, cols


def run_vs_reference(eng_mod, cfg_kw, aggs, ncols, batches, device=False, sync=True, options=None, late_indices=False):
    """Push `batches` [(keys, ts, cols, nulls or None, watermark)] through an engine handle with `aggs` and through
    the oracle over the first-occurrence columns; rows after every watermark, late drops and (late_indices) the dropped
    records' indices must be equal. Returns (rows, late drops, the engine handle's stats, its option reader's values)."""
    from oracle.oracle import Oracle
    raggs, dcols = reference_aggs(aggs, ncols)
    kw = dict(cfg_kw)
    nullable = tuple(kw.pop("nullable_cols", ()))
    cfg = A.make_config(aggs=aggs, nullable_cols=nullable, late_indices=late_indices, **kw)
    rcfg = A.make_config(aggs=raggs, nullable_cols=nullable, late_indices=late_indices,
                         **{k: v for k, v in kw.items() if k != "record_lists"})
    names = A.agg_names(rcfg)
    g, o = eng_mod.WindowAggregator(cfg, options=options), Oracle(rcfg)
    first = {c: FirstOccurrence(kw["size_ms"], kw.get("offset_ms", 0), kw.get("tz")) for c in dcols}
    rows = dg = do = 0
    for keys, ts, cols, nulls, wm in batches:
        if len(keys):
            marks = [first[c].mark(keys, ts, cols[c], None if nulls is None or nulls[c] is None else nulls[c])
                     for c in dcols]
            rnulls = None if nulls is None else list(nulls) + [None] * len(marks)
            do += o.push(keys, ts, list(cols) + marks, nulls=rnulls)
            if device:
                import torch
                dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
                r = g.push(dev(keys), dev(ts), [dev(c) for c in cols], sync=sync,
                           nulls=None if nulls is None else [dev(z) for z in nulls])
            else:
                r = g.push(keys, ts, cols, nulls=nulls)
            if late_indices:
                assert np.array_equal(g.late_records(), o.late_records()), "late indices differ"
            if sync:
                dg += r
        rg, ro = g.advance_watermark(wm), o.advance_watermark(wm)
        assert_rows_equal(rg, ro, names, ctx="wm=%d" % wm)
        for j, nm in enumerate(A.agg_names(cfg)):
            if nm == "COUNT_DISTINCT":
                assert "null%d" % j not in rg, "COUNT(DISTINCT) is never NULL"
        rows += len(ro["key"])
    st = g.stats()
    if not sync:
        dg = st.late_dropped
    assert dg == do, ("late drops", dg, do)
    opts = {n: g.get_option(n) for n in ("distinct_slots", "distinct_live", "distinct_rebuilds")}
    g.close()
    o.close()
    return rows, do, st, opts
