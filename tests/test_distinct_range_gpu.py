"""COUNT(DISTINCT col) over Table HOP / CUMULATE windows on the GPU (FWA_CFG_DISTINCT_RANGE, flink_amd/csrc/distinct.inc).

The set keeps one entry per (key, value, column, block of 64 slices) with a bitmap of the slices, and every firing step
counts the values with a bit inside each fired window's slice range. Small hand-built shapes sit on the places that can
go wrong (a window across a block boundary, negative slice numbers, many windows in one step, windows of three blocks,
late-but-accepted and dropped records, zero keys / values and NULLs); random streams, rebuilds, snapshots, the facade and
the WindowAggregateITCase rows follow. Every case is compared, after every watermark, with the oracle's rows whose
distinct columns come from brute force (distinct_range_ref.py)."""
import json
import os

import numpy as np
import pytest

from distinct_range_ref import (CUMULATE_KW, HOP_KW, RANDOM_AGGS, Reference, check_engine, make_cfg, random_batches,
                                random_case, run_range_vs_reference)
from flink_amd import _abi as A
from helpers import GOLDEN, assert_rows_equal

pytestmark = pytest.mark.gpu

DA = [("COUNT", 0), ("COUNT_DISTINCT", 0)]


@pytest.fixture(scope="module")
def eng_mod():
    from flink_amd import engine
    engine.lib()
    return engine


def _i64(x):
    return np.asarray(x, np.int64)


def _batch(recs, wm, ncols=1):
    """recs: [(key, ts, v0, ...)] -> one batch of int64 columns followed by the watermark."""
    a = _i64(recs).reshape(len(recs), 2 + ncols)
    return (a[:, 0].copy(), a[:, 1].copy(), [a[:, 2 + c].copy() for c in range(ncols)], None, wm)


def _steps(wms):
    e = np.zeros(0, np.int64)
    return [(e, e, [e], None, wm) for wm in wms]


def _col(ref, b, j=1):
    """{(key, start, end): value of aggregate j} of the reference rows of batch b."""
    r = ref.rows[b]
    return {(int(k), int(s), int(e)): int(v) for k, s, e, v in zip(r["key"], r["win_start"], r["win_end"], r["agg%d" % j])}


# ---- a window across a block boundary: the smallest shape that can go wrong ----

def _boundary_records(sign):
    """HOP 4 s / 1 s, one key: value 5 in slices 62 and 65, value 9 only in slice 63 (the block boundary is q = 64);
    sign = -1 mirrors it to slices -63 and -66 (value 5) and -64 (value 9), across q = -64."""
    if sign > 0:
        return [(7, 62_100, 5), (7, 62_900, 5), (7, 63_500, 9), (7, 65_200, 5)]
    return [(7, -62_100, 5), (7, -62_900, 5), (7, -63_500, 9), (7, -65_200, 5)]


@pytest.mark.parametrize("sign", [1, -1], ids=["q64", "q_minus64"])
def test_block_boundary_one_window_per_step(eng_mod, sign):
    lo = 60_000 if sign > 0 else -70_000
    batches = [_batch(_boundary_records(sign), lo - 1)] + _steps(range(lo + 999, lo + 12_000, 1000))
    ref, _ = run_range_vs_reference(eng_mod, HOP_KW, DA, batches)
    assert ref.most == 1                                  # every window fired alone (the launch_fire path)
    got = {}
    for b in range(len(batches)):
        got.update(_col(ref, b))
    if sign > 0:      # windows [59, 63) .. [65, 69) s: slices 62 | 62 63 | 62 63 (64) | 62 63 (64) 65 | 63 (64) 65 | (64) 65 | 65
        assert [got[(7, s, s + 4000)] for s in range(59_000, 66_000, 1000)] == [1, 2, 2, 2, 2, 1, 1]
    else:
        assert sorted(got.values()) == [1, 1, 1, 2, 2, 2, 2]


@pytest.mark.parametrize("sign", [1, -1], ids=["q64", "q_minus64"])
def test_many_windows_in_one_step(eng_mod, sign):
    """The same stream, one watermark jump over all seven windows: the sliding fire with carried sums."""
    lo = 60_000 if sign > 0 else -70_000
    batches = [_batch(_boundary_records(sign), lo - 1)] + _steps([lo + 12_000])
    ref, _ = run_range_vs_reference(eng_mod, HOP_KW, DA, batches)
    assert ref.most >= 2 and sorted(_col(ref, 1).values()) == [1, 1, 1, 2, 2, 2, 2]


def test_wide_windows_span_three_blocks(eng_mod):
    """HOP 130 ms / 1 ms: a window is 130 slices, so it meets three blocks and the earlier-block probes run twice.
    Value 1 sits in blocks 0, 1 and 2 (slices 10, 70, 135), value 2 in blocks 0 and 2, value 3 only in block 1."""
    kw = dict(window_kind="SLIDE", semantics="TABLE", size_ms=130, slide_ms=1)
    recs = [(3, 10, 1), (3, 70, 1), (3, 135, 1), (3, 20, 2), (3, 130, 2), (3, 100, 3), (4, 63, 8), (4, 64, 8), (4, 192, 8)]
    batches = [_batch(recs, -1000)] + _steps([-50, 9, 10, 63, 64, 100, 139, 140, 141, 149, 200, 264, 265, 400])
    ref, _ = run_range_vs_reference(eng_mod, kw, DA, batches)
    allrows = {}
    for b in range(len(batches)):
        allrows.update(_col(ref, b))
    assert allrows[(3, 6, 136)] == 3 and allrows[(3, 10, 140)] == 3 and allrows[(3, 21, 151)] == 3
    assert allrows[(3, 101, 231)] == 2 and allrows[(3, 131, 261)] == 1 and allrows[(4, 63, 193)] == 1
    assert ref.most >= 2


def test_windows_shorter_than_64_ms_are_accepted(eng_mod):
    """The 64 ms limit of the TUMBLE form does not apply: the tag keeps the block number."""
    kw = dict(window_kind="SLIDE", semantics="TABLE", size_ms=8, slide_ms=2)
    recs = [(1, t, t % 3) for t in range(0, 300, 1)]
    run_range_vs_reference(eng_mod, kw, DA, [_batch(recs[:150], 100), _batch(recs[150:], 260)] + _steps([A.LONG_MAX]))


# ---- CUMULATE ----

def test_cumulate_late_slices_accepted_and_dropped_records(eng_mod):
    """CUMULATE 4 s / 1 s, cycle [0, 4 s). Value 12 is first seen in the cycle's last slice; (500, 13) arrives when its own
    slice [0, 1 s) has fired and is accepted into the later windows of the cycle; (600, 14) arrives when the cycle has
    fired and is dropped (its index is reported, its value counts nowhere)."""
    batches = [_batch([(1, 100, 11), (1, 1100, 11), (2, 200, 11)], 999),
               _batch([(1, 500, 13), (1, 3500, 12), (1, 3600, 11)], 1999),
               _batch([(1, 2500, 13)], 3999),
               _batch([(1, 600, 14), (1, 4100, 14)], A.LONG_MAX)]
    ref, _ = run_range_vs_reference(eng_mod, CUMULATE_KW, DA, batches)
    assert _col(ref, 0) == {(1, 0, 1000): 1, (2, 0, 1000): 1}
    assert _col(ref, 1) == {(1, 0, 2000): 2, (2, 0, 2000): 1}
    assert _col(ref, 2) == {(1, 0, 3000): 2, (1, 0, 4000): 3, (2, 0, 3000): 1, (2, 0, 4000): 1}
    assert ref.late[1].tolist() == [] and ref.late[3].tolist() == [0]
    assert set(_col(ref, 3).values()) == {1}


# ---- zero keys, zero values, NULLs, several distinct aggregates ----

def test_zero_keys_zero_values_and_nulls(eng_mod):
    aggs = [("COUNT", 0), ("COUNT_DISTINCT", 1), ("SUM_I64", 0), ("COUNT_DISTINCT", 2), ("MAX_F64", 3),
            ("COUNT_DISTINCT", 1)]
    kw = dict(HOP_KW, nullable_cols=(1, 2))
    #       key   ts   c0  c1  c2  n1 n2
    recs = [(0,  100,   1,  0,  0,  0, 0), (0,  200,  2,  1,  0,  0, 0), (0, 1300,  3,  0,  1,  0, 0),
            (0, 1400,   4,  5,  5,  1, 0), (5,  100,  5,  0,  7,  1, 1), (5, 2100,  6,  0,  7,  1, 1),
            (-1, 300,   7,  0,  0,  0, 1), (-1, 5300, 8,  1,  0,  1, 0), (0, 5200,  9,  0,  0,  0, 0)]
    a = _i64(recs)
    f = np.linspace(-2.0, 2.0, len(recs))
    cols = [a[:, 2].copy(), a[:, 3].copy(), a[:, 4].copy(), f]
    nulls = [None, a[:, 5].astype(np.uint8), a[:, 6].astype(np.uint8), None]
    e = np.zeros(0, np.int64)
    batches = [(a[:, 0].copy(), a[:, 1].copy(), cols, nulls, -5000)]
    batches += [(e, e, [e, e, e, np.zeros(0)], None, wm) for wm in (999, 1999, 4999, A.LONG_MAX)]
    ref, _ = run_range_vs_reference(eng_mod, kw, aggs, batches)
    first = _col(ref, 1, 1)                               # windows ending at 1 s: slice 0 only
    assert first[(0, -3000, 1000)] == 2 and first[(5, -3000, 1000)] == 0 and first[(-1, -3000, 1000)] == 1
    assert _col(ref, 1, 5) == first and _col(ref, 1, 3)[(-1, -3000, 1000)] == 0
    assert _col(ref, 2, 1)[(0, -2000, 2000)] == 2 and _col(ref, 2, 3)[(0, -2000, 2000)] == 3   # value 5 of c1 is NULL


# ---- random streams ----

@pytest.mark.parametrize("name,device,out_dev", [("hop", False, 0), ("hop", True, 1), ("cumulate", False, 1),
                                                 ("cumulate", True, 0), ("hop_shift", False, 0)])
def test_random_streams_vs_reference(eng_mod, name, device, out_dev):
    kw, batches, ref = random_case(name)
    assert ref.n_late > 0 and 4 * ref.n_union >= ref.n_rows > 1000     # the cross-slice union is exercised
    g = eng_mod.WindowAggregator(make_cfg(kw, RANDOM_AGGS, output_on_device=out_dev))
    assert check_engine(g, ref, batches, device=device) == ref.n_rows
    assert g.stats().late_dropped == ref.n_late
    assert g.get_option("distinct_count_steps") > 0 and g.get_option("distinct_count_us") > 0
    g.close()


# ---- rebuilds keep the bitmaps; fired blocks are reclaimed ----

def test_rebuilds_keep_the_bitmaps(eng_mod):
    kw, batches, ref = random_case("hop")
    g = eng_mod.WindowAggregator(make_cfg(kw, RANDOM_AGGS), options={"distinct_slots": 64})
    check_engine(g, ref, batches)
    assert g.get_option("distinct_rebuilds") > 0 and g.get_option("distinct_slots") > 64
    g.close()


def test_fired_blocks_are_reclaimed(eng_mod):
    """40 pushes of 2000 new values, 16 slices apart, each fired before the next: an entry lives as long as its block
    of 64 slices, so a rebuild finds at most the pushes of the block the watermark is in and of the one pushed next --
    5 pushes -- and sizes the table for 2 x (5 n + n) entries: 32768 slots for n = 2000, however long the stream."""
    n = 2000
    g = eng_mod.WindowAggregator(make_cfg(HOP_KW, DA))
    slots = []
    for p in range(40):
        g.push(np.full(n, 1, np.int64), np.full(n, 16_000 * p + 10, np.int64), [np.arange(n, dtype=np.int64) + p * n])
        r = g.advance_watermark(16_000 * p - 1)           # fires the four windows of push p - 1
        got = {int(s): int(c) for s, c in zip(r["win_start"], r["agg1"])}
        assert got == ({16_000 * (p - 1) - 1000 * i: n for i in range(4)} if p else {})
        slots.append(g.get_option("distinct_slots"))
    assert g.get_option("distinct_rebuilds") > 0
    assert g.get_option("distinct_live") <= 5 * n
    assert max(slots) <= 32768 and len(set(slots[12:])) == 1, slots
    r = g.advance_watermark(A.LONG_MAX)
    assert sorted(r["agg1"].tolist()) == [n] * 4
    g.close()


# ---- snapshot mid-stream, restored into one handle and into two ----

def test_snapshot_restore_with_rescale(eng_mod):
    from flink_amd import snapshot as S
    kw = dict(HOP_KW, key_capacity=256, nullable_cols=(1, 2))
    batches = random_batches(seed=33, n=1 << 14, nkeys=60, pushes=8)
    ref = Reference(kw, RANDOM_AGGS, batches)
    cut = 4
    mid = Reference(kw, RANDOM_AGGS, batches[:cut])
    wm = batches[cut - 1][4]
    g = eng_mod.WindowAggregator(make_cfg(kw, RANDOM_AGGS))
    check_engine(g, ref, batches, last=cut)
    blob = g.snapshot()
    check_engine(g, ref, batches, first=cut)             # the snapshot's rebuild left the uninterrupted handle intact
    g.close()
    d = S.parse(blob)["distinct"]
    live = mid.brute.live_tuples(lambda q: q * 1000 + 4000 - 1 <= wm)
    assert d["n"] == len(live) > 0 and d["agg_mask"] == 0b1100
    got = set(zip(d["key"].tolist(), d["value"].tolist(), (d["slice_start"] // 1000).tolist(), d["column"].tolist()))
    assert got == live

    h = eng_mod.WindowAggregator(make_cfg(kw, RANDOM_AGGS))
    h.restore(blob)
    check_engine(h, ref, batches, first=cut)
    h.close()

    keys_all = np.concatenate([b[0] for b in batches])
    kg_of = dict(zip(keys_all.tolist(), eng_mod.key_groups(keys_all, 128, 1, A.KEY_JAVA_LONG)[0].tolist()))
    hs = []
    for lo, hi in ((0, 63), (64, 127)):
        x = eng_mod.WindowAggregator(make_cfg(kw, RANDOM_AGGS, kg_start=lo, kg_end=hi))
        x.restore(blob)
        hs.append((lo, hi, x))
    for b in range(cut, len(batches)):
        keys, ts, cols, nulls, bwm = batches[b]
        kgs = np.array([kg_of[k] for k in keys.tolist()], np.int64)
        outs, late = [], 0
        for lo, hi, x in hs:
            m = (kgs >= lo) & (kgs <= hi)
            if m.any():
                late += x.push(keys[m], ts[m], [c[m] for c in cols], nulls=[None if z is None else z[m] for z in nulls])
            outs.append(x.advance_watermark(bwm))
        assert late == len(ref.late[b])
        assert_rows_equal({f: np.concatenate([r[f] for r in outs]) for f in outs[0]}, ref.rows[b], ref.names)
    for _lo, _hi, x in hs:
        x.close()


# ---- the Table facade sets the flag itself ----

@pytest.mark.parametrize("kind", ["hopping", "cumulative"])
def test_slicing_window_processor_needs_no_flag(eng_mod, kind):
    from flink_amd.assigners import SliceAssigners
    from flink_amd.operators import SlicingWindowProcessor
    p = SlicingWindowProcessor(getattr(SliceAssigners, kind)(2000, 1000), [("COUNT", 0), ("COUNT_DISTINCT", 0)]).open()
    assert p.cfg.flags & A.CFG_DISTINCT_RANGE
    for key, v, ts in ((1, 7, 100), (1, 7, 1200), (1, 8, 1300), (2, 7, 400)):
        assert p.process_element(key, (v,), ts) is False
    rows = sorted(p.advance_progress(1999))
    if kind == "hopping":                                 # windows [-1, 1) s and [0, 2) s
        assert rows == [(1, 1, 1, -1000, 1000), (1, 3, 2, 0, 2000), (2, 1, 1, -1000, 1000), (2, 1, 1, 0, 2000)]
    else:                                                 # windows [0, 1) s and [0, 2) s
        assert rows == [(1, 1, 1, 0, 1000), (1, 3, 2, 0, 2000), (2, 1, 1, 0, 1000), (2, 1, 1, 0, 2000)]
    p.close()


# ---- the reference's own numbers: WindowAggregateITCase HOP and CUMULATE with COUNT(DISTINCT string) ----

@pytest.mark.parametrize("which", [0, 1], ids=["hop", "cumulate"])
def test_itcase_rows_with_all_five_aggregates(eng_mod, which):
    from flink_amd.keydict import KeyDictionary
    with open(os.path.join(GOLDEN, "sql_distinct_hop_cumulate_kats.json")) as f:
        case = json.load(f)["operators"][which]
    cfg = A.make_config(window_kind=case["window_kind"], semantics="TABLE", size_ms=case["size_ms"],
                        slide_ms=case["slide_ms"], offset_ms=case["offset_ms"], aggs=[tuple(a) for a in case["aggs"]],
                        nullable_cols=case["nullable_cols"], distinct_range=True)
    g = eng_mod.WindowAggregator(cfg)
    d = KeyDictionary(["STRING"], capacity=64)
    types = case["col_types"]
    got, dropped = [], 0
    for ev in case["events"]:
        if ev[0] == "e":
            vals = ev[2]
            s = vals[3]
            sid = d.encode([[s or ""]], [np.array([s is None], np.uint8)]).cpu().numpy()   # NULL: only its flag is read
            cols = [np.array([0 if vals[c] is None else vals[c]], types[c]) for c in range(3)] + [sid]
            nulls = [np.array([vals[c] is None], np.uint8) for c in range(4)]
            dropped += g.push(_i64([ev[1]]), _i64([ev[3]]), cols, nulls=nulls)
            continue
        rows = g.advance_watermark(ev[1])
        assert "null0" not in rows and "null4" not in rows
        for i in range(len(rows["key"])):
            r = [int(rows["key"][i]), int(rows["win_start"][i]), int(rows["win_end"][i])]
            for j in range(5):
                nul = rows.get("null%d" % j)
                v = rows["agg%d" % j][i]
                r.append(None if nul is not None and nul[i] else (v.item() if hasattr(v, "item") else v))
            got.append(r)
    key = lambda r: tuple((x is None, x) for x in r)
    assert sorted(got, key=key) == sorted(case["expected"], key=key), got
    assert dropped == case["late_dropped"] == 0
    g.close()
    d.close()


# ---- refusals that remain under the flag ----

def _refused(eng_mod, **kw):
    with pytest.raises(eng_mod.EngineError) as ei:
        eng_mod.WindowAggregator(A.make_config(**kw))
    assert ei.value.code == -7 and "DISTINCT" in str(ei.value), str(ei.value)
    return str(ei.value)


def test_refused_configurations_under_the_flag(eng_mod):
    fl = dict(distinct_range=True)
    _refused(eng_mod, window_kind="SESSION", semantics="TABLE", gap_ms=500, aggs=DA, **fl)
    _refused(eng_mod, window_kind="SLIDE", semantics="DATASTREAM", size_ms=4000, slide_ms=1000, aggs=DA, **fl)
    _refused(eng_mod, window_kind="SLIDE", semantics="DATASTREAM", size_ms=4000, slide_ms=1000,
             aggs=[("COUNT_DISTINCT", 0)], reduce=True, **fl)
    _refused(eng_mod, aggs=DA, key_kind=A.KEY_PREHASHED, **HOP_KW, **fl)
    _refused(eng_mod, aggs=DA, key_kind=A.KEY_PREHASHED, **CUMULATE_KW, **fl)
    assert "FWA_CFG_DISTINCT_RANGE" in _refused(eng_mod, aggs=DA, **HOP_KW)         # without the flag: as before
    g = eng_mod.WindowAggregator(A.make_config(window_kind="TUMBLE", semantics="TABLE", size_ms=1000, aggs=DA, **fl))
    g.push(_i64([1, 1]), _i64([5, 6]), [_i64([3, 3])])     # on a TUMBLE handle the flag changes nothing
    r = g.advance_watermark(A.LONG_MAX)
    assert r["agg1"].tolist() == [1]
    with pytest.raises(eng_mod.EngineError):
        g.get_option("distinct_count_steps")               # (range-mode counters: not this handle's)
    g.close()


def test_refused_entry_points_under_the_flag(eng_mod):
    import ctypes as C
    L = eng_mod.lib()
    g = eng_mod.WindowAggregator(make_cfg(HOP_KW, DA, output_on_device=1))
    k = np.zeros(1, np.int64)
    g.push(k, k, [k])

    def refused(call):
        with pytest.raises(eng_mod.EngineError) as ei:
            call()
        assert ei.value.code == -7 and "DISTINCT" in str(ei.value), str(ei.value)

    refused(lambda: g.drain_partials(10))
    refused(lambda: g.push_partials(k, k, k, [k, k]))
    refused(lambda: g.drain_route(10, 2))
    refused(lambda: g.fire_partials(np.zeros((1, 4), np.int64), [2, 3], 10))
    refused(lambda: g.snapshot_heap())
    body = C.create_string_buffer(8)
    ptrs, sizes, wms = (C.c_void_p * 1)(C.cast(body, C.c_void_p).value), (C.c_int64 * 1)(0), (C.c_int64 * 1)(0)
    assert L.fwa_restore_heap(g.h, ptrs, sizes, wms, 1) == -7 and b"DISTINCT" in L.fwa_last_error(g.h)
    g.close()
