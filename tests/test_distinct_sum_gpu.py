"""SUM(DISTINCT col) / AVG(DISTINCT col) over Table windows on the GPU (FWA_AGG_DISTINCT, flink_amd/csrc/distinct.inc).

TUMBLE: the marking pass writes w = first occurrence ? value : 0 beside the 0/1 column, the fire sums both and a finish
step gives NULL flags and AVG's division. HOP / CUMULATE (FWA_CFG_DISTINCT_RANGE): the fire's pass over the set adds
each counted value to a per-row sum. Small hand-written shapes sit where the code can go wrong (the stored stand-in of
value 0, wrap-around, truncation, NULL-only windows, the hidden counter, block boundaries); every case is compared after
every watermark with the reference of distinct_sum_ref.py, which never calls the engine."""
import numpy as np
import pytest

import distinct_sum_ref as R
from flink_amd import _abi as A

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
CNT, SUM, AVG = "COUNT_DISTINCT", "SUM_DISTINCT_I64", "AVG_DISTINCT_I64"
FSUM, FAVG = "SUM_DISTINCT_F64", "AVG_DISTINCT_F64"
ALL3 = [("COUNT", 0), (CNT, 0), (SUM, 0), (AVG, 0)]


@pytest.fixture(scope="module")
def eng_mod():
    from flink_amd import engine
    engine.lib()
    return engine


def _b(keys, ts, cols, wm, nulls=None, dtypes=None):
    """One batch: int64 keys / timestamps, value columns (int64 unless dtypes says otherwise), NULL flags or None."""
    dt = dtypes or [np.int64] * len(cols)
    return (np.asarray(keys, np.int64), np.asarray(ts, np.int64), [np.asarray(c, d) for c, d in zip(cols, dt)],
            None if nulls is None else [None if z is None else np.asarray(z, np.uint8) for z in nulls], wm)


def _steps(wms, ncols=1, dtypes=None):
    return [_b([], [], [[]] * ncols, wm, dtypes=dtypes) for wm in wms]


def _vals(ref, batches=None):
    """{(key, start, end): (per aggregate: value, or None when NULL)} of the reference rows."""
    out = {}
    for b, r in enumerate(ref.rows):
        if batches is not None and b not in batches:
            continue
        for i in range(len(r["key"])):
            row = []
            for j in range(len(ref.names)):
                z = r.get("null%d" % j)
                v = r["agg%d" % j][i]
                row.append(None if z is not None and z[i] else (v.item() if hasattr(v, "item") else v))
            out[(int(r["key"][i]), int(r["win_start"][i]), int(r["win_end"][i]))] = tuple(row)
    return out


def _tumble(eng_mod, aggs, ncols, batches, kw=None, options=None, **check):
    kw = dict(R.TUMBLE_KW, **(kw or {}))
    ref = R.TumbleReference(kw, aggs, ncols, batches)
    g = eng_mod.WindowAggregator(R.tumble_cfg(kw, aggs), options=options)
    assert R.check_engine(g, ref, batches, **check) == ref.n_rows
    return ref, g


def _range(eng_mod, kw, aggs, batches, options=None, **check):
    ref = R.RangeReference(kw, aggs, batches)
    g = eng_mod.WindowAggregator(R.range_cfg(kw, aggs), options=options)
    assert R.check_engine(g, ref, batches, **check) == ref.n_rows
    assert g.stats().late_dropped == ref.n_late
    g.close()
    return ref


# ---- 1. the smallest TUMBLE shape, with and without the caller's own COUNT_DISTINCT (the hidden counter) ----

@pytest.mark.parametrize("own_count", [True, False], ids=["own_count", "hidden_counter"])
def test_smallest_tumble_shape(eng_mod, own_count):
    aggs = ALL3 if own_count else [a for a in ALL3 if a[0] != CNT]
    z4 = [[0, 0, 0, 0]]
    batches = [_b([1] * 4, [100, 200, 300, 400], [[5, 5, 7, 5]], 999, nulls=z4),
               _b([1, 1], [1100, 1200], [[3, 4]], 1999, nulls=[[1, 1]])]
    ref, g = _tumble(eng_mod, aggs, 1, batches, kw=dict(nullable_cols=(0,)))
    g.close()
    want = {(1, 0, 1000): (4, 2, 12, 6), (1, 1000, 2000): (2, 0, None, None)}      # the NULL-only row exists
    if not own_count:
        want = {k: (v[0],) + v[2:] for k, v in want.items()}
    assert _vals(ref) == want


def test_null_flags_without_a_nullable_declaration(eng_mod):
    """agg_null is a real array even when the column is not declared nullable (check_engine asserts it)."""
    ref, g = _tumble(eng_mod, [("COUNT", 0), (SUM, 0)], 1, [_b([1, 2], [10, 20], [[4, 4]], A.LONG_MAX)])
    g.close()
    assert _vals(ref) == {(1, 0, 1000): (1, 4), (2, 0, 1000): (1, 4)}


# ---- 2. zero value and zero key: the set stores 0 as 1 plus a flag ----

def test_zero_value_and_zero_key(eng_mod):
    batches = [_b([0, 0, 0, 9, 0], [10, 20, 30, 40, 1500], [[0, 0, 1, 0, 1]], A.LONG_MAX)]
    ref, g = _tumble(eng_mod, ALL3, 1, batches)
    g.close()
    assert _vals(ref) == {(0, 0, 1000): (3, 2, 1, 0), (9, 0, 1000): (1, 1, 0, 0),   # [0] alone: sum 0, not NULL
                          (0, 1000, 2000): (1, 1, 1, 1)}                            # the stand-in 1 is a value too


# ---- 3. integer arithmetic ----

def test_wrap_and_truncation(eng_mod):
    batches = [_b([1, 1, 1, 2, 2, 3, 3], [1] * 7, [[I64_MAX, 1, 1, -7, 2, 7, -2]], A.LONG_MAX)]
    ref, g = _tumble(eng_mod, ALL3, 1, batches)
    g.close()
    got = _vals(ref)
    assert got[(1, 0, 1000)][2] == I64_MIN                                          # LONG_MAX + 1 wraps
    assert got[(2, 0, 1000)] == (2, 2, -5, -2) and got[(3, 0, 1000)] == (2, 2, 5, 2)  # toward zero, both signs


# ---- 4. repeats: across pushes, windows, keys; a dropped late record ----

def test_repeats_across_pushes_windows_keys_and_a_late_record(eng_mod):
    batches = [_b([1, 1, 2], [100, 1100, 100], [[5, 5, 5]], -1),
               _b([1, 1, 2], [200, 1200, 300], [[5, 6, 5]], 999),                   # repeats of push 1 add nothing
               _b([1, 1], [500, 1300], [[77, 6]], A.LONG_MAX)]                      # (500, 77): window [0, 1 s) fired
    ref, g = _tumble(eng_mod, ALL3, 1, batches)
    g.close()
    assert ref.late[2].tolist() == [0]
    assert _vals(ref) == {(1, 0, 1000): (2, 1, 5, 5), (2, 0, 1000): (2, 1, 5, 5), (1, 1000, 2000): (3, 2, 11, 5)}


# ---- 5. mixed handles ----

def test_two_distinct_columns_and_a_column_a_plain_sum_also_reads(eng_mod):
    """Column 0: SUM and AVG(DISTINCT) and a plain SUM_I64 (its w and m take free indices); column 1: its own pair."""
    aggs = [("SUM_I64", 0), (SUM, 0), (AVG, 0), (AVG, 1), (CNT, 1), ("COUNT", 0)]
    batches = [_b([1, 1, 1, 2], [1, 2, 3, 4], [[4, 4, 6, 4], [10, 20, 10, 0]], 999, nulls=[None, [0, 0, 0, 1]]),
               _b([1], [1001], [[4], [10]], A.LONG_MAX, nulls=[None, [0]])]
    ref, g = _tumble(eng_mod, aggs, 2, batches, kw=dict(nullable_cols=(1,)))
    g.close()
    assert _vals(ref) == {(1, 0, 1000): (14, 10, 5, 15, 2, 3), (2, 0, 1000): (4, 4, 4, None, 0, 1),
                          (1, 1000, 2000): (4, 4, 4, 10, 1, 1)}


def _create_status(eng_mod, cfg):
    try:
        eng_mod.WindowAggregator(cfg).close()
        return 0, ""
    except eng_mod.EngineError as e:
        return e.code, str(e)


def test_budgets_and_argument_errors(eng_mod):
    import ctypes as C
    mk = lambda aggs: A.make_config(aggs=aggs, **R.TUMBLE_KW)
    seven = [("SUM_I64", c) for c in range(7)]
    assert _create_status(eng_mod, mk(seven + [(CNT, 7)]))[0] == 0                  # m takes the source's index
    code, why = _create_status(eng_mod, mk(seven + [(SUM, 7)]))                     # ... and w finds none
    assert code == -7 and "FWA_MAX_COLS" in why, why
    assert _create_status(eng_mod, mk([("COUNT", 0)] * 6 + [(CNT, 0), (SUM, 0)]))[0] == 0
    code, why = _create_status(eng_mod, mk([("COUNT", 0)] * 7 + [(SUM, 0)]))        # no slot for the hidden counter
    assert code == -7 and "FWA_MAX_AGGS" in why, why
    for base in ("COUNT_DISTINCT", "COUNT_COL", "COUNT", "MIN_I64", "MAX_F64", "SUM_F32", "AVG_F32", "SUM_DEC"):
        cfg = mk([("COUNT", 0), ("SUM_I64", 0)])
        cfg.aggs[1].kind = A.AGG_DISTINCT | A.AGG_KINDS[base]
        h = C.c_void_p()
        code = eng_mod.lib().fwa_create(C.byref(cfg), C.byref(h))              # (the wrapper has no name for the kind)
        why = eng_mod.lib().fwa_last_error(None).decode()
        assert code == -1, (base, code, why)
        if base in ("SUM_F32", "AVG_F32", "SUM_DEC"):
            assert "FLOAT" in why and "INT" in why and "DECIMAL" in why, why
    assert _create_status(eng_mod, mk([(SUM, 0), (FAVG, 0)]))[0] == -1              # BIGINT and DOUBLE over one column
    assert _create_status(eng_mod, mk([(SUM, 0), (FAVG, 1)]))[0] == 0
    # accepted and refused as COUNT_DISTINCT is
    hop = dict(window_kind="SLIDE", semantics="TABLE", size_ms=4000, slide_ms=1000)
    for kw in (hop, dict(window_kind="SESSION", semantics="TABLE", gap_ms=500),
               dict(window_kind="TUMBLE", semantics="DATASTREAM", size_ms=1000), dict(R.TUMBLE_KW, size_ms=32),
               dict(R.TUMBLE_KW, key_kind=A.KEY_PREHASHED)):
        code, why = _create_status(eng_mod, A.make_config(aggs=[("COUNT", 0), (SUM, 0)], **kw))
        assert code == -7 and "DISTINCT" in why, (kw, code, why)
    assert _create_status(eng_mod, A.make_config(aggs=[("COUNT", 0), (SUM, 0)], distinct_range=True, **hop))[0] == 0


def test_refused_entry_points_and_the_callers_configuration(eng_mod):
    import ctypes as C
    g = eng_mod.WindowAggregator(A.make_config(aggs=[("COUNT", 0), (SUM, 0)], output_on_device=1, **R.TUMBLE_KW))
    k = np.zeros(1, np.int64)
    g.push(k, k, [k])
    for call in (lambda: g.drain_partials(10), lambda: g.push_partials(k, k, k, [k, k]), lambda: g.snapshot_heap()):
        with pytest.raises(eng_mod.EngineError) as ei:
            call()
        assert ei.value.code == -7 and "DISTINCT" in str(ei.value)
    out = A.Config()
    assert eng_mod.lib().fwa_get_config(g.h, C.byref(out)) == 0
    assert out.num_aggs == 2 and (out.aggs[1].kind, out.aggs[1].col) == (0x101, 0)  # no hidden counter shows
    assert g.advance_watermark_raw(A.LONG_MAX).num_aggs == 2
    g.close()


# ---- 6. DOUBLE ----

F8 = [np.float64]


def test_double_exact_stream_bit_for_bit(eng_mod):
    """Multiples of 2^-10 below 2^6: every sum is exactly representable, so the bound is 0."""
    rng = np.random.default_rng(8)
    n = 4000
    keys, ts = rng.integers(0, 20, n), np.sort(rng.integers(0, 5000, n))
    vals = rng.integers(-64, 64, n) / 1024.0
    nul = rng.random(n) < 0.2
    aggs = [("COUNT", 0), (CNT, 0), (FSUM, 0), (FAVG, 0)]
    batches = [_b(keys[:2000], ts[:2000], [vals[:2000]], 1999, nulls=[nul[:2000]], dtypes=F8),
               _b(keys[2000:], ts[2000:], [vals[2000:]], A.LONG_MAX, nulls=[nul[2000:]], dtypes=F8)]
    ref, g = _tumble(eng_mod, aggs, 1, batches, kw=dict(nullable_cols=(0,)))
    g.close()
    assert ref.n_rows > 50


def test_double_special_values(eng_mod):
    aggs = [(CNT, 0), (FSUM, 0), (FAVG, 0)]
    nan, inf = float("nan"), float("inf")
    batches = [_b([1, 1, 2, 2, 3, 4, 4, 5, 5], [1] * 9, [[-0.0, 0.0, nan, nan, inf, inf, -inf, 0.25, 0.5]], A.LONG_MAX,
                  dtypes=F8)]
    g = eng_mod.WindowAggregator(R.tumble_cfg(R.TUMBLE_KW, aggs))
    g.push(*batches[0][:3])
    r = g.advance_watermark(A.LONG_MAX)
    got = {int(k): (int(c), float(s), float(a), int(z)) for k, c, s, a, z in
           zip(r["key"], r["agg0"], r["agg1"], r["agg2"], r["null1"])}
    g.close()
    assert got[1] == (2, 0.0, 0.0, 0)                                               # -0.0 and 0.0: two values
    assert got[2][0] == 1 and np.isnan(got[2][1]) and np.isnan(got[2][2])           # one NaN pushed twice
    assert got[3] == (1, inf, inf, 0)
    assert got[4][0] == 2 and np.isnan(got[4][1])
    assert got[5] == (2, 0.75, 0.375, 0)
    ref = R.TumbleReference(R.TUMBLE_KW, aggs, 1, batches)                          # ... and the reference agrees
    R.assert_sum_rows_equal(r, ref.rows[0], ref.names)


# ---- 7. push paths ----

@pytest.mark.parametrize("path", ["host", "device", "async_push", "async_watermark", "lists", "rebuild", "shift_zone"])
def test_random_tumble_stream_on_every_path(eng_mod, path):
    kw, batches, ref = R.random_case("tumble")
    kw, options, check = dict(kw), None, {}
    if path in ("device", "async_push", "async_watermark"):
        check = dict(device=True, sync=path == "device", async_wm=path == "async_watermark")
    if path == "lists":                                    # record lists: no nullable columns
        kw = dict(kw, record_lists=True, nullable_cols=())
        batches = [(k, t, c, None, wm) for k, t, c, _z, wm in batches]
        ref = R.TumbleReference(kw, R.RANDOM_AGGS, 3, batches)
    if path == "rebuild":
        options = {"distinct_slots": 64}
    if path == "shift_zone":
        from helpers import load_tz_kats
        kw["tz"] = {c["zone"]: c["tz"] for c in load_tz_kats()["timer"]}["Asia/Shanghai"]
        batches = [(k, t + 1615593600000, c, z, wm if wm == A.LONG_MAX else wm + 1615593600000)
                   for k, t, c, z, wm in batches]
        ref = R.TumbleReference(kw, R.RANDOM_AGGS, 3, batches)
    g = eng_mod.WindowAggregator(R.tumble_cfg(kw, R.RANDOM_AGGS), options=options)
    assert R.check_engine(g, ref, batches, **check) == ref.n_rows > 1000
    assert g.stats().late_dropped == ref.n_late > 0
    if path == "rebuild":
        assert g.get_option("distinct_rebuilds") > 0 and g.get_option("distinct_slots") > 64
    g.close()


def test_decimal_count_distinct_and_sum_distinct_on_one_handle(eng_mod):
    """The DECIMAL plan renumbers the internal aggregates behind the distinct plan: both finish steps map through it."""
    aggs = [("SUM_DEC", 0, 2), (SUM, 1), ("COUNT", 0), (CNT, 1), ("AVG_DEC", 0, 2), (AVG, 2)]
    rng = np.random.default_rng(9)
    n = 3000
    keys, ts = rng.integers(0, 400, n), np.sort(rng.integers(0, 4000, n))
    cols = [rng.integers(-10**6, 10**6, n), rng.integers(-5, 5, n), rng.integers(0, 4, n) << 50]
    nul = [None, rng.random(n) < 0.3, rng.random(n) < 0.6]
    cut = n // 2
    batches = [_b(keys[:cut], ts[:cut], [c[:cut] for c in cols], 1500, nulls=[None] + [z[:cut] for z in nul[1:]]),
               _b(keys[cut:], ts[cut:], [c[cut:] for c in cols], A.LONG_MAX, nulls=[None] + [z[cut:] for z in nul[1:]])]
    ref, g = _tumble(eng_mod, aggs, 3, batches, kw=dict(nullable_cols=(1, 2)))
    g.close()
    assert ref.n_rows > 50 and any(v[5] is None for v in _vals(ref).values())


# ---- 8. snapshot mid-window, restored into one subtask and into two ----

def _restore_and_finish(eng_mod, make, blob, ref, batches, cut):
    h = make()
    h.restore(blob)
    R.check_engine(h, ref, batches, first=cut)
    h.close()
    keys_all = np.concatenate([b[0] for b in batches])
    kg_of = dict(zip(keys_all.tolist(), eng_mod.key_groups(keys_all, 128, 1, A.KEY_JAVA_LONG)[0].tolist()))
    hs = []
    for lo, hi in ((0, 63), (64, 127)):
        x = make(kg_start=lo, kg_end=hi)
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
        R.assert_sum_rows_equal({f: np.concatenate([r[f] for r in outs]) for f in outs[0]}, ref.rows[b], ref.names,
                                ctx="two subtasks, batch %d" % b)
    for _lo, _hi, x in hs:
        x.close()


@pytest.mark.parametrize("name", ["tumble", "hop"])
def test_snapshot_restore_with_rescale(eng_mod, name):
    """The watermark of the cut lies inside a window (1 s under the newest timestamp, the stream is out of order by up to
    6 s): later pushes repeat values of before the checkpoint, and the results equal the uninterrupted reference."""
    from flink_amd import snapshot as S
    kw, batches, ref = R.random_case(name)
    cfg = R.tumble_cfg if name == "tumble" else R.range_cfg
    make = lambda **more: eng_mod.WindowAggregator(cfg(kw, R.RANDOM_AGGS, **more))
    cut = 4
    g = make()
    R.check_engine(g, ref, batches, last=cut)
    blob = g.snapshot()
    R.check_engine(g, ref, batches, first=cut)            # the snapshot's rebuild left the uninterrupted handle intact
    g.close()
    d = S.parse(blob)["distinct"]
    assert d["n"] > 0 and d["agg_mask"] == 0b011100       # word 27: a bit per distinct aggregate of either form
    assert set(d["column"].tolist()) == {0, 1}
    _restore_and_finish(eng_mod, make, blob, ref, batches, cut)


# ---- 9. range mode ----

RA = [("COUNT", 0), (CNT, 0), (SUM, 0), (AVG, 0)]


def _boundary(sign, wms_from):
    """distinct_range tests' block-boundary stream: HOP 4 s / 1 s, one key, value 5 in slices 62 and 65, value 9 only in
    slice 63 (the block boundary is q = 64); sign = -1 mirrors it across q = -64."""
    recs = [(62_100, 5), (62_900, 5), (63_500, 9), (65_200, 5)]
    lo = 60_000 if sign > 0 else -70_000
    return [_b([7] * 4, [sign * t for t, _v in recs], [[v for _t, v in recs]], lo - 1)] + _steps(wms_from(lo))


@pytest.mark.parametrize("sign", [1, -1], ids=["q64", "q_minus64"])
@pytest.mark.parametrize("jump", [False, True], ids=["one_window_per_step", "one_jump"])
def test_range_block_boundary(eng_mod, sign, jump):
    """One window per step (launch_fire), or one watermark jump over all seven windows (the carried-sum fire)."""
    wms = (lambda lo: [lo + 12_000]) if jump else (lambda lo: range(lo + 999, lo + 12_000, 1000))
    ref = _range(eng_mod, R.HOP_KW, RA, _boundary(sign, wms))
    got = _vals(ref)
    assert len(got) == 7
    if sign > 0:
        assert [got[(7, s, s + 4000)][2] for s in range(59_000, 66_000, 1000)] == [5, 14, 14, 14, 14, 5, 5]
        assert [got[(7, s, s + 4000)][3] for s in range(59_000, 66_000, 1000)] == [5, 7, 7, 7, 7, 5, 5]
    else:
        assert sorted(v[2] for v in got.values()) == [5, 5, 5, 14, 14, 14, 14]


def test_range_hidden_count_only(eng_mod):
    """No COUNT_DISTINCT of the caller's: the per-row distinct count still decides NULL and divides AVG."""
    ref = _range(eng_mod, R.HOP_KW, [("COUNT", 0), (AVG, 0)], _boundary(1, lambda lo: [lo + 12_000]))
    assert sorted(v[1] for v in _vals(ref).values()) == [5, 5, 5, 7, 7, 7, 7]


def test_range_wide_windows_span_three_blocks(eng_mod):
    kw = dict(window_kind="SLIDE", semantics="TABLE", size_ms=130, slide_ms=1)
    recs = [(3, 10, 1), (3, 70, 1), (3, 135, 1), (3, 20, 2), (3, 130, 2), (3, 100, 3), (4, 63, 8), (4, 64, 8), (4, 192, 8)]
    batches = [_b([r[0] for r in recs], [r[1] for r in recs], [[r[2] for r in recs]], -1000)]
    batches += _steps([-50, 9, 10, 63, 64, 100, 139, 140, 141, 149, 200, 264, 265, 400])
    got = _vals(_range(eng_mod, kw, RA, batches))
    assert got[(3, 6, 136)][1:3] == (3, 6) and got[(3, 101, 231)][1:3] == (2, 3) and got[(3, 131, 261)][1:3] == (1, 1)
    assert got[(4, 63, 193)][1:3] == (1, 8)


def test_range_cumulate_null_only_window_and_value_zero(eng_mod):
    """CUMULATE 4 s / 1 s: key 1's first window holds only a NULL, its later ones value 0 alone (sum 0, not NULL) and
    then {0, 12}; key 0 repeats value 12 across slices."""
    batches = [_b([1, 1, 0, 1, 0, 1], [100, 1100, 200, 2100, 2200, 1200], [[99, 0, 12, 12, 12, 0]], A.LONG_MAX,
                  nulls=[[1, 0, 0, 0, 0, 0]])]
    got = _vals(_range(eng_mod, dict(R.CUMULATE_KW, nullable_cols=(0,)), RA, batches))
    assert got[(1, 0, 1000)] == (1, 0, None, None) and got[(1, 0, 2000)] == (3, 1, 0, 0)
    assert got[(1, 0, 3000)] == (4, 2, 12, 6) and got[(0, 0, 4000)] == (2, 1, 12, 12)


def test_range_double(eng_mod):
    aggs = [("COUNT", 0), (CNT, 0), (FSUM, 0), (FAVG, 0)]
    b = _boundary(1, lambda lo: range(lo + 999, lo + 12_000, 1000))
    b = [(k, t, [c[0].astype(np.float64) + 0.25], z, wm) for k, t, c, z, wm in b]
    got = _vals(_range(eng_mod, R.HOP_KW, aggs, b))
    assert [got[(7, s, s + 4000)][2] for s in range(59_000, 66_000, 1000)] == [5.25, 14.5, 14.5, 14.5, 14.5, 5.25, 5.25]
    assert got[(7, 60_000, 64_000)][3] == 7.25


@pytest.mark.parametrize("name,device", [("hop", False), ("cumulate", True)])
def test_range_random_streams_vs_brute_force(eng_mod, name, device):
    kw, batches, ref = R.random_case(name)
    assert ref.stats["union"] > 0 and ref.stats["null"] > 0 and ref.stats["differ"] > 0
    g = eng_mod.WindowAggregator(R.range_cfg(kw, R.RANDOM_AGGS))
    assert R.check_engine(g, ref, batches, device=device) == ref.n_rows > 1000
    assert g.stats().late_dropped == ref.n_late > 0
    g.close()


def test_range_rebuilds_keep_the_sums(eng_mod):
    kw, batches, ref = R.random_case("hop")
    g = eng_mod.WindowAggregator(R.range_cfg(kw, R.RANDOM_AGGS), options={"distinct_slots": 64})
    R.check_engine(g, ref, batches)
    assert g.get_option("distinct_rebuilds") > 0 and g.get_option("distinct_slots") > 64
    g.close()


def test_facade_over_slide_with_avg_distinct(eng_mod):
    from flink_amd.assigners import SliceAssigners
    from flink_amd.operators import SlicingWindowProcessor
    p = SlicingWindowProcessor(SliceAssigners.hopping(2000, 1000), [("COUNT", 0), (AVG, 0)]).open()
    assert p.cfg.flags & A.CFG_DISTINCT_RANGE
    for key, v, ts in ((1, 7, 100), (1, 7, 1200), (1, 10, 1300), (2, 7, 400)):
        assert p.process_element(key, (v,), ts) is False
    # windows [-1, 1) s and [0, 2) s: key 1 has {7} then {7, 10} -> 17 / 2 truncates to 8
    assert sorted(p.advance_progress(1999)) == [(1, 1, 7, -1000, 1000), (1, 3, 8, 0, 2000), (2, 1, 7, -1000, 1000),
                                               (2, 1, 7, 0, 2000)]
    p.close()
    t = SlicingWindowProcessor(SliceAssigners.tumbling(1000), [("COUNT", 0), (AVG, 0)])
    assert not t.cfg.flags & A.CFG_DISTINCT_RANGE
    t.close()


# ---- 10. no change for handles that carry only COUNT_DISTINCT ----

def test_count_distinct_only_handles_are_unchanged(eng_mod):
    """The stream and aggregates of tests/test_distinct_snapshot_gpu.py: two handles in one process give the rows of the
    first-occurrence reference and the same snapshot: header (word 27 = the COUNT_DISTINCT bit alone) and key-group
    offsets byte for byte, the accumulator entries and the set entries
    as sorted lists. Inside a key group the blob keeps the order of the key table's and of the set's slots, and which of
    two colliding inserts wins a slot differs from run to run (two handles of the parent build differ there as well), so
    the bytes behind the offsets are compared as the entries they encode."""
    from distinct_ref import run_vs_reference
    from flink_amd import snapshot as S
    rng = np.random.default_rng(21)
    n = 20_000
    keys = rng.integers(0, 200, n).astype(np.int64)
    ts = np.sort(rng.integers(0, 10_000, n)).astype(np.int64) - rng.integers(0, 2500, n)
    cols = [rng.integers(-50, 50, n).astype(np.int64), rng.integers(0, 30, n).astype(np.int64)]
    nulls = [None, (rng.random(n) < 0.1).astype(np.uint8)]
    aggs = [("COUNT", 0), ("SUM_I64", 0), ("COUNT_DISTINCT", 1)]
    kw = dict(R.TUMBLE_KW, key_capacity=1024, nullable_cols=(1,))
    cut = n // 2
    wm1 = int(ts[:cut].max()) - 400
    blobs = []
    for _handle in range(2):
        g = eng_mod.WindowAggregator(A.make_config(aggs=aggs, **kw))
        g.push(keys[:cut], ts[:cut], [c[:cut] for c in cols], nulls=[None, nulls[1][:cut]])
        rows = g.advance_watermark(wm1)
        assert "null2" not in rows and g.advance_watermark_raw(wm1).num_aggs == 3
        blobs.append((g.snapshot(), rows))
        g.close()
    (b1, r1), (b2, r2) = blobs
    from helpers import assert_rows_equal
    assert_rows_equal(r1, r2, [a[0] for a in aggs])
    s1, s2 = S.parse(b1), S.parse(b2)
    assert s1["distinct"]["agg_mask"] == 0b100 and s1["aggs"] == [0, 1, 1]
    fixed = 8 * (32 + 128 + 1)                            # header words and the body's key-group offsets
    assert len(b1) == len(b2) and b1[:fixed] == b2[:fixed]
    body = lambda s: sorted(zip(s["key"].tolist(), s["slice_start"].tolist(), s["count"].tolist(),
                                *(a.tolist() for a in s["acc"] + s["hidden"])))
    assert body(s1) == body(s2) and s1["n"] > 0
    assert np.array_equal(s1["distinct"]["kg_offsets"], s2["distinct"]["kg_offsets"])
    entries = lambda s: sorted(zip(*(s["distinct"][f].tolist() for f in ("key", "value", "slice_start", "column"))))
    assert entries(s1) == entries(s2) and s1["distinct"]["n"] > 0
    batches = [(keys[:cut], ts[:cut], [c[:cut] for c in cols], [None, nulls[1][:cut]], wm1),
               (keys[cut:], ts[cut:], [c[cut:] for c in cols], [None, nulls[1][cut:]], A.LONG_MAX)]
    rows, late, _st, _opts = run_vs_reference(eng_mod, kw, aggs, 2, batches)
    assert rows > 0 and late > 0
