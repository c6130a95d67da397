"""COUNT / SUM / AVG(DISTINCT col) over Table SESSION windows on the GPU (FWA_CFG_DISTINCT_SESSION, distinct.inc).

The set keeps one entry per (key, value, column, block of 64 cells), a cell being floor(local ts / gap); the marking pass
runs behind the ingest and skips the records it dropped, and every firing step counts the fired rows from the set and
then clears their bits. Every case is compared, after every watermark, with the oracle's rows whose distinct columns
come from brute force (distinct_session_ref.py); late drops and late indices are compared after every push."""
import ctypes as C

import numpy as np
import pytest

import distinct_session_ref as R
from distinct_sum_ref import assert_sum_rows_equal
from flink_amd import _abi as A

pytestmark = pytest.mark.gpu

DA = [("COUNT", 0), ("COUNT_DISTINCT", 0)]
LONG_MIN = -(1 << 63)


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


def _step(wm, ncols=1):
    e = np.zeros(0, np.int64)
    return (e, e, [e] * ncols, None, wm)


def _run(eng_mod, kw, aggs, batches, ref=None, options=None, device=False, late=True, firing=True):
    """One handle under the flag against the reference of the same stream; returns (reference, options read, paths)."""
    ref = ref or R.SessionReference(kw, aggs, batches)
    g = eng_mod.WindowAggregator(R.session_cfg(kw, aggs, late_indices=late), options=options)
    paths = []
    for b in range(len(batches)):
        R.check_engine(g, ref, batches, first=b, last=b + 1, device=device, late=late)
        if len(batches[b][0]):
            paths.append(g.get_option("session_path"))
    opts = {n: g.get_option(n) for n in ("distinct_slots", "distinct_live", "distinct_rebuilds", "distinct_count_steps",
                                         "distinct_index_us", "distinct_count_us")}
    assert g.stats().late_dropped == ref.n_late
    if firing:
        assert opts["distinct_count_steps"] > 0
    if not late:
        with pytest.raises(eng_mod.EngineError) as ei:     # the caller did not ask for the indices
            g.late_records()
        assert ei.value.code == -8
    flags = g.get_config().flags                          # the caller's, not the internal configuration's
    assert bool(flags & A.CFG_LATE_INDICES) == late and flags & A.CFG_DISTINCT_SESSION
    g.close()
    return ref, opts, paths


def _rows(ref, b, j=1):
    r = ref.rows[b]
    return sorted((int(k), int(s), int(e), int(v)) for k, s, e, v in zip(r["key"], r["win_start"], r["win_end"], r["agg%d" % j]))


# ---- the two counter-examples of the cell argument, rows written out by hand ----

def test_dropped_record_sets_no_bit(eng_mod):
    """g = 10, watermark 20: 10 is dropped, 12 is accepted as [12, 22) in the same cell; the dropped value 7 must not
    count. Then a watermark that jumps far enough to fire several sessions of the key in one step."""
    kw = dict(R.SESSION_KW, gap_ms=10)
    batches = [_batch([(1, 25, 3)], 20), _batch([(1, 10, 7), (1, 12, 8)], 21),
               _batch([(1, 50, 3), (1, 70, 3), (1, 75, 4), (1, 100, 5), (2, 100, 5)], 22), _step(A.LONG_MAX)]
    ref, _, _ = _run(eng_mod, kw, DA, batches)
    assert [len(x) for x in ref.late] == [0, 1, 0, 0] and ref.late[1].tolist() == [0]
    assert _rows(ref, 1) == [(1, 12, 22, 1)]              # 8 alone: not 7
    assert _rows(ref, 3) == [(1, 25, 35, 1), (1, 50, 60, 1), (1, 70, 85, 2), (1, 100, 110, 1), (2, 100, 110, 1)]
    assert _rows(ref, 3, j=0) == [(1, 25, 35, 1), (1, 50, 60, 1), (1, 70, 85, 2), (1, 100, 110, 1), (2, 100, 110, 1)]


def test_fired_session_bits_are_cleared(eng_mod):
    """g = 10: [0, 10) with values 3 and 4 fires at watermark 9; then 5 is accepted as the new session [5, 15) in the
    same cell 0 with value 6: its count is 1, not 3."""
    kw = dict(R.SESSION_KW, gap_ms=10)
    batches = [_batch([(1, 0, 3), (1, 0, 4)], 9), _batch([(1, 5, 6)], 13), _step(14), _step(A.LONG_MAX)]
    ref, _, _ = _run(eng_mod, kw, DA, batches)
    assert _rows(ref, 0) == [(1, 0, 10, 2)] and _rows(ref, 1) == [] and _rows(ref, 2) == [(1, 5, 15, 1)]


def test_saved_record_moves_the_start_below_a_fired_session(eng_mod):
    """g = 500: [21224, 21724) fires at 21914; 21532 is accepted and 21100, late on its own, is saved by it: the session
    [21100, 22032) spans the fired record's cell, whose bit the fire has cleared."""
    kw = dict(R.SESSION_KW, gap_ms=500)
    batches = [_batch([(36, 21224, 1)], 21914), _batch([(36, 21532, 2), (36, 21100, 3)], A.LONG_MAX)]
    ref, _, _ = _run(eng_mod, kw, DA, batches)
    assert _rows(ref, 0) == [(36, 21224, 21724, 1)] and _rows(ref, 1) == [(36, 21100, 22032, 2)]


# ---- edge values ----

def test_edge_keys_values_and_negative_timestamps(eng_mod):
    """Key 0 and key LONG_MIN, value 0, negative timestamps (floor-divided cells: -1 and -10 are cells -1 and -1,
    -11 is cell -2), a session across cell 0, and a BIGINT sum that wraps."""
    kw = dict(R.SESSION_KW, gap_ms=10)
    aggs = [("COUNT", 0), ("COUNT_DISTINCT", 0), ("SUM_DISTINCT_I64", 0), ("AVG_DISTINCT_I64", 0)]
    big = (1 << 62) + 5
    recs = [(0, -11, 0), (0, -10, 0), (0, -1, 9), (0, 3, 9), (0, 4, 0),
            (LONG_MIN, -640, 0), (LONG_MIN, -635, 1), (LONG_MIN, -100, 0),
            (5, -7, big), (5, -3, big + 1), (5, 2, big), (5, 6, -3)]
    batches = [_batch(recs[:6], -700), _batch(recs[6:], -600), _step(-50), _step(A.LONG_MAX)]
    ref, _, _ = _run(eng_mod, kw, aggs, batches)
    assert _rows(ref, 3) == [(0, -11, 14, 2), (5, -7, 16, 3)]
    assert _rows(ref, 3, j=2) == [(0, -11, 14, 9), (5, -7, 16, R.LONG_MIN + 8)]     # 2^63 + 11 - 3 wraps
    assert _rows(ref, 1) == [(LONG_MIN, -640, -625, 2)] and _rows(ref, 2) == [(LONG_MIN, -100, -90, 1)]


def test_double_zero_and_minus_zero_are_two_values(eng_mod):
    kw = dict(R.SESSION_KW, gap_ms=100)
    aggs = [("COUNT_DISTINCT", 0), ("SUM_DISTINCT_F64", 0), ("AVG_DISTINCT_F64", 0)]
    k, t = _i64([1, 1, 1, 1, 2]), _i64([0, 10, 20, 30, 0])
    v = np.array([0.0, -0.0, 1.5, 0.0, -0.0])
    batches = [(k, t, [v], None, 50), (k[:0], t[:0], [v[:0]], None, A.LONG_MAX)]
    ref, _, _ = _run(eng_mod, kw, aggs, batches)
    assert _rows(ref, 1, j=0) == [(1, 0, 130, 3), (2, 0, 100, 1)]
    r = ref.rows[1]
    assert sorted(r["agg1"].tolist()) == [0.0, 1.5] and sorted(r["agg2"].tolist()) == [0.0, 0.5]


# ---- random streams: every session path, host and device pushes, with and without the caller's late indices ----

def _random_params():
    """Every stream on the general path and with the paths left to the engine, from the host with the caller's late
    indices and from the device without; two streams also in the two mixed combinations."""
    out = []
    for name in ("g50_count", "g500_all", "g50_nulls", "g3_blocks", "g50_ordered", "g3_ordered"):
        for cells in (0, -1):
            for device, late in ((False, True), (True, False), (False, False), (True, True)):
                if device != late or name in ("g50_count", "g50_ordered"):
                    out.append(pytest.param(name, cells, device, late, id="%s-%s-%s-%s" % (
                        name, "general" if cells == 0 else "adaptive", "device" if device else "host",
                        "late_indices" if late else "no_late_indices")))
    return out


@pytest.mark.parametrize("name,cells,device,late", _random_params())
def test_random_streams(eng_mod, name, cells, device, late):
    kw, aggs, batches, ref = R.random_case(name)
    _, opts, paths = _run(eng_mod, kw, aggs, batches, ref=ref, options={"session_cells": cells}, device=device, late=late)
    print("session paths", name, cells, paths, opts)
    if cells == 0:
        assert set(paths) == {0}
    elif name == "g50_ordered":
        assert set(paths) == {2}                          # cell pre-aggregation: few cells per push, nothing late
    elif name == "g3_ordered":
        assert 1 in paths                                 # more than 16 cells per push: the sort-based cell path
    else:
        assert 0 in paths                                 # late records hand the push back to the general path
    if name == "g50_nulls":                               # sessions of only NULLs: COUNT 0, SUM NULL
        assert any(((r["agg1"] == 0) & (r["null2"] != 0)).any() for r in ref.rows if len(r["key"]))


@pytest.mark.parametrize("name", ["g500_shanghai", "g500_los_angeles"])
def test_shift_time_zone_across_a_transition(eng_mod, name):
    kw, aggs, batches, ref = R.random_case(name)
    lts = np.concatenate([R.tz_local(b[1], kw["tz"]) - b[1] for b in batches if len(b[0])])
    assert len(np.unique(lts)) == 2                       # the stream crosses the transition
    _run(eng_mod, kw, aggs, batches, ref=ref)


# ---- rebuilds between fires that cleared part of an entry's bits ----

@pytest.mark.parametrize("name,slots,grows", [("g50_nulls", 64, True), ("g50_nulls", 2048, False), ("g3_blocks", 64, True)],
                         ids=["grow_then_in_place", "in_place", "grow_in_place_grow"])
def test_rebuilds_mid_stream(eng_mod, name, slots, grows):
    """The bound of a push (records x columns on top of the entries the table holds, dead ones included) passes half of
    a small table at almost every push, while the live entries -- those with a bit left after the fires -- stay near
    a hundred: a table of 64 slots grows to 2048 at the first push and is then rebuilt in place, one of 2048 slots is
    rebuilt in place from the second push on; the stream of gap 3 grows, rebuilds in place and grows again."""
    kw, aggs, batches, ref = R.random_case(name)
    _, opts, _ = _run(eng_mod, kw, aggs, batches, ref=ref, options={"distinct_slots": slots})
    assert opts["distinct_rebuilds"] >= 2, opts
    assert (opts["distinct_slots"] > slots) == grows, opts
    assert 0 < opts["distinct_live"] < 400, opts          # the last rebuild kept only entries with bits


# ---- snapshot mid-stream, restored into one handle and into two ----

def test_snapshot_restore_with_rescale(eng_mod):
    from flink_amd import snapshot as S
    kw, aggs, batches, ref = R.random_case("g50_nulls")
    cut = 4
    mid = R.SessionReference(kw, aggs, batches[:cut])
    g = eng_mod.WindowAggregator(R.session_cfg(kw, aggs))
    R.check_engine(g, ref, batches, last=cut)
    blob = g.snapshot()
    R.check_engine(g, ref, batches, first=cut)            # the snapshot's rebuild left the uninterrupted handle intact
    g.close()
    d = S.parse(blob)["distinct"]
    live = mid.live_tuples()
    assert d["n"] == len(live) > 0 and d["agg_mask"] == 0b11110
    assert (d["slice_start"] % kw["gap_ms"] == 0).all()
    got = set(zip(d["key"].tolist(), d["value"].tolist(), (d["slice_start"] // kw["gap_ms"]).tolist(), d["column"].tolist()))
    assert got == live

    h = eng_mod.WindowAggregator(R.session_cfg(kw, aggs))
    h.restore(blob)
    R.check_engine(h, ref, batches, first=cut)
    h.close()

    keys_all = np.concatenate([b[0] for b in batches])
    kg_of = dict(zip(keys_all.tolist(), eng_mod.key_groups(keys_all, 128, 1, A.KEY_JAVA_LONG)[0].tolist()))
    hs = []
    for lo, hi in ((0, 63), (64, 127)):
        x = eng_mod.WindowAggregator(R.session_cfg(kw, aggs, kg_start=lo, kg_end=hi))
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
        assert_sum_rows_equal({f: np.concatenate([r[f] for r in outs]) for f in outs[0]}, ref.rows[b], ref.names)
    for _lo, _hi, x in hs:
        x.close()


def test_snapshot_of_a_plain_session_handle_is_refused_and_the_reverse(eng_mod):
    kw = dict(R.SESSION_KW, gap_ms=50)
    k = _i64([1, 2])
    plain = eng_mod.WindowAggregator(A.make_config(aggs=[("COUNT", 0), ("COUNT", 0)], **kw))
    dist = eng_mod.WindowAggregator(R.session_cfg(kw, DA))
    for g in (plain, dist):
        g.push(k, k, [k])
    bp, bd = plain.snapshot(), dist.snapshot()
    for blob, into in ((bp, R.session_cfg(kw, DA)), (bd, A.make_config(aggs=[("COUNT", 0), ("COUNT", 0)], **kw))):
        h = eng_mod.WindowAggregator(into)
        with pytest.raises(eng_mod.EngineError) as ei:
            h.restore(blob)
        assert ei.value.code == -1 and "DISTINCT" in str(ei.value)     # header word 27
        h.close()
    plain.close()
    dist.close()


# ---- refusals ----

def _refused(eng_mod, **kw):
    with pytest.raises(eng_mod.EngineError) as ei:
        eng_mod.WindowAggregator(A.make_config(**kw))
    assert ei.value.code == -7 and "DISTINCT" in str(ei.value), str(ei.value)
    return str(ei.value)


def test_refused_configurations_under_the_flag(eng_mod):
    fl = dict(distinct_session=True, window_kind="SESSION", gap_ms=500, aggs=DA)
    _refused(eng_mod, semantics="TABLE", allowed_lateness_ms=1, **fl)
    _refused(eng_mod, semantics="TABLE", gap_col=0, **fl)
    _refused(eng_mod, semantics="DATASTREAM", **fl)
    _refused(eng_mod, semantics="DATASTREAM", reduce=True, **dict(fl, aggs=[("COUNT_DISTINCT", 0)]))
    _refused(eng_mod, semantics="TABLE", key_kind=A.KEY_PREHASHED, **fl)
    for sum_kind in ("SUM_DISTINCT_I64", "AVG_DISTINCT_F64"):
        _refused(eng_mod, semantics="TABLE", allowed_lateness_ms=1, **dict(fl, aggs=[("COUNT", 0), (sum_kind, 0)]))
    # without the flag, and under the range flag: refused as before
    _refused(eng_mod, window_kind="SESSION", semantics="TABLE", gap_ms=500, aggs=DA)
    _refused(eng_mod, window_kind="SESSION", semantics="TABLE", gap_ms=500, aggs=DA, distinct_range=True)
    # on handles that are not SESSION the flag changes nothing
    _refused(eng_mod, window_kind="SLIDE", semantics="TABLE", size_ms=4000, slide_ms=1000, aggs=DA, distinct_session=True)
    g = eng_mod.WindowAggregator(A.make_config(window_kind="TUMBLE", semantics="TABLE", size_ms=1000, aggs=DA,
                                               distinct_session=True))
    g.push(_i64([1, 1]), _i64([5, 6]), [_i64([3, 3])])
    assert g.advance_watermark(A.LONG_MAX)["agg1"].tolist() == [1]
    with pytest.raises(eng_mod.EngineError):
        g.get_option("distinct_count_steps")               # (fire-time counters: not this handle's)
    g.close()
    # ... and on a SESSION handle without a distinct aggregate
    g = eng_mod.WindowAggregator(A.make_config(window_kind="SESSION", semantics="TABLE", gap_ms=10, aggs=[("COUNT", 0)],
                                               distinct_session=True))
    g.push(_i64([1, 1]), _i64([5, 6]), [_i64([3, 3])])
    assert g.advance_watermark(A.LONG_MAX)["agg0"].tolist() == [2]
    g.close()


def test_refused_entry_points_on_an_accepted_handle(eng_mod):
    L = eng_mod.lib()
    g = eng_mod.WindowAggregator(R.session_cfg(dict(R.SESSION_KW, gap_ms=50), DA, output_on_device=1))
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


# ---- a push the ingest refuses marks nothing; fill_out twice ----

def test_refused_push_marks_nothing(eng_mod):
    """A batch with a key outside the handle's key groups is refused by the ingest: none of its values reaches the set
    (the snapshot's section is empty), and the values pushed again under owned keys count from scratch."""
    from flink_amd import snapshot as S
    kw = dict(R.SESSION_KW, gap_ms=10)
    keys = np.arange(1, 200, dtype=np.int64)
    kgs = eng_mod.key_groups(keys, 128, 1, A.KEY_JAVA_LONG)[0]
    own, other = int(keys[kgs < 64][0]), int(keys[kgs >= 64][0])
    g = eng_mod.WindowAggregator(R.session_cfg(kw, DA, kg_start=0, kg_end=63))
    with pytest.raises(eng_mod.EngineError) as ei:
        g.push(_i64([own, other]), _i64([0, 0]), [_i64([7, 8])])
    assert ei.value.code == -3
    assert S.parse(g.snapshot())["distinct"]["n"] == 0
    g.push(_i64([own, own]), _i64([0, 10]), [_i64([7, 7])])  # touching windows merge: [0, 20), cells 0 and 1
    assert S.parse(g.snapshot())["distinct"]["n"] == 2    # one value in two cells
    assert g.advance_watermark(A.LONG_MAX)["agg1"].tolist() == [1]
    g.close()


def test_fired_output_gives_the_same_finished_rows(eng_mod):
    """fwa_fired_output behind fwa_advance_watermark_async (the step itself hands out no rows, fill_out runs at the
    take) returns the finished rows fwa_advance_watermark returns: SUM / AVG are finished into plan-owned columns, never
    in place, so AVG is divided once whichever call fills the output."""
    kw = dict(R.SESSION_KW, gap_ms=10)
    aggs = [("COUNT_DISTINCT", 0), ("AVG_DISTINCT_I64", 0), ("SUM_DISTINCT_I64", 0)]
    rows = []
    for take in (False, True):
        g = eng_mod.WindowAggregator(R.session_cfg(kw, aggs))
        g.push(_i64([1, 1, 1, 2]), _i64([0, 3, 6, 0]), [_i64([10, 20, 10, 7])])
        if take:
            g.advance_watermark_async(A.LONG_MAX)
            rows.append(g.fired_output())
            with pytest.raises(eng_mod.EngineError):
                g.fired_output_raw()                       # taken
        else:
            rows.append(g.advance_watermark(A.LONG_MAX))
        assert g.get_option("distinct_count_steps") == 1
        g.close()
    for r in rows:
        got = sorted(zip(r["key"].tolist(), r["agg0"].tolist(), r["agg1"].tolist(), r["agg2"].tolist()))
        assert got == [(1, 2, 15, 30), (2, 1, 7, 7)]      # AVG is not divided twice
