"""COUNT(DISTINCT col) over Table TUMBLE windows on the GPU (FWA_COUNT_DISTINCT, flink_amd/csrc/distinct.inc).

Small shapes with hand-written expectations exercise the lock-free set insert (one wave, one block, many blocks on
three slots, the EMPTY sentinels, negative slice numbers, pushes that repeat values, growth, reclaiming, NULLs);
random streams and the two-phase ingest are compared with the oracle over first-occurrence columns (distinct_ref.py);
the WindowAggregateITCase row is replayed with all five of its aggregates on one handle."""
import json
import os

import numpy as np
import pytest

from distinct_ref import run_vs_reference
from flink_amd import _abi as A
from helpers import GOLDEN, load_tz_kats

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
TABLE = dict(window_kind="TUMBLE", semantics="TABLE", size_ms=1000)


@pytest.fixture(scope="module")
def eng_mod():
    from flink_amd import engine
    engine.lib()
    return engine


def _handle(eng_mod, aggs=(("COUNT", 0), ("COUNT_DISTINCT", 0)), options=None, **kw):
    return eng_mod.WindowAggregator(A.make_config(aggs=list(aggs), **{**TABLE, **kw}), options=options)


def _fire(g, wm=A.LONG_MAX, agg=1):
    r = g.advance_watermark(wm)
    assert "null%d" % agg not in r
    return {(int(k), int(s)): int(c) for k, s, c in zip(r["key"], r["win_start"], r["agg%d" % agg])}


def _i64(x):
    return np.asarray(x, np.int64)


# ---- one wave ----

def test_one_wave_one_triple(eng_mod):
    g = _handle(eng_mod)
    g.push(np.full(64, 7, np.int64), np.full(64, 500, np.int64), [np.full(64, 42, np.int64)])
    assert _fire(g) == {(7, 0): 1}
    g.close()


def test_one_wave_64_values(eng_mod):
    g = _handle(eng_mod)
    g.push(np.full(64, 7, np.int64), np.full(64, 500, np.int64), [np.arange(64, dtype=np.int64)])
    assert _fire(g) == {(7, 0): 64}
    g.close()


def test_one_wave_two_windows(eng_mod):
    g = _handle(eng_mod)
    ts = _i64([500, 1500] * 32)
    g.push(np.full(64, 7, np.int64), ts, [np.full(64, 42, np.int64)])
    assert _fire(g) == {(7, 0): 1, (7, 1000): 1}
    g.close()


# ---- one block, many blocks ----

def test_one_block_one_triple(eng_mod):
    g = _handle(eng_mod)
    g.push(np.full(256, -5, np.int64), np.full(256, 999, np.int64), [np.full(256, 9, np.int64)])
    assert _fire(g) == {(-5, 0): 1}
    g.close()


def test_many_blocks_three_triples(eng_mod):
    n = 1 << 16
    pick = np.random.default_rng(1).integers(0, 3, n)
    keys = _i64([1, 1, 2])[pick]
    vals = _i64([10, 11, 10])[pick]
    g = _handle(eng_mod)
    g.push(keys, np.full(n, 10, np.int64), [vals])
    r = g.advance_watermark(A.LONG_MAX)
    got = {int(k): (int(c), int(d)) for k, c, d in zip(r["key"], r["agg0"], r["agg1"])}
    assert got == {1: (int((pick < 2).sum()), 2), 2: (int((pick == 2).sum()), 1)}
    g.close()


# ---- sentinels: keys and values equal to the set's EMPTY word, and their stand-ins ----

@pytest.mark.parametrize("t0", [100, -4100], ids=["q0", "negative_q"])
def test_sentinel_keys_and_values(eng_mod, t0):
    ks, vs = [0, 1, -1, I64_MIN], [0, 1, -1, I64_MIN, I64_MAX]
    keys = _i64([k for k in ks for v in vs for _ in range(3)])
    vals = _i64([v for k in ks for v in vs for _ in range(3)])
    g = _handle(eng_mod)
    g.push(keys, np.full(len(keys), t0, np.int64), [vals])
    start = (t0 // 1000) * 1000
    assert _fire(g) == {(k, start): 5 for k in ks}
    g.close()


# ---- across pushes ----

@pytest.mark.parametrize("mode", ["host", "device", "async"])
def test_same_triple_in_two_pushes_counts_once(eng_mod, mode):
    import torch
    g = _handle(eng_mod)
    conv = (lambda a: a) if mode == "host" else (lambda a: torch.from_numpy(a).cuda())
    keep = []
    for vals in ([5, 5, 6], [6, 5, 7, 7]):
        n = len(vals)
        cols = (conv(np.full(n, 3, np.int64)), conv(np.full(n, 250, np.int64)), conv(_i64(vals)))
        keep.append(cols)
        g.push(cols[0], cols[1], [cols[2]], sync=mode != "async")
    assert _fire(g) == {(3, 0): 3}
    g.close()


# ---- growth, rebuild, reclaiming ----

def test_growth_from_a_small_table(eng_mod):
    g = _handle(eng_mod, options={"distinct_slots": 64})
    assert g.get_option("distinct_slots") == 64
    vals = np.arange(1000, dtype=np.int64) * 7919
    for _ in range(2):
        g.push(np.full(1000, 1, np.int64), np.full(1000, 1, np.int64), [vals])
    assert g.get_option("distinct_rebuilds") > 0 and g.get_option("distinct_slots") >= 2048
    assert g.get_option("distinct_live") == 1000          # the second push's rebuild found the first push's entries
    assert _fire(g) == {(1, 0): 1000}
    with pytest.raises(eng_mod.EngineError):              # the first size can no longer change
        g.set_option("distinct_slots", 128)
    g.close()


def test_fired_windows_are_reclaimed(eng_mod):
    n = 2000
    g = _handle(eng_mod)
    vals = np.arange(n, dtype=np.int64)
    slots = []
    for p in range(40):
        g.push(np.full(n, 1, np.int64), np.full(n, 1000 * p + 10, np.int64), [vals])
        got = _fire(g, 1000 * p - 1)                      # fires window p - 1
        assert got == ({(1, 1000 * (p - 1)): n} if p else {})
        slots.append(g.get_option("distinct_slots"))
    assert g.get_option("distinct_rebuilds") > 0
    assert g.get_option("distinct_live") <= n            # at a rebuild only the last pushed window has not fired
    assert max(slots) <= 8 * n and len(set(slots[8:])) == 1, slots
    assert _fire(g) == {(1, 39000): n}
    g.close()


# ---- NULLs ----

def test_nulls_are_ignored_and_never_equal(eng_mod):
    g = _handle(eng_mod, nullable_cols=(0,))
    keys = _i64([1, 1, 1, 2, 2, 2, 2])
    vals = _i64([0, 0, 0, 0, 0, 4, 4])                    # key 1: all NULL; key 2: NULL, 0, 4, NULL (its value ignored)
    nul = np.array([1, 1, 1, 1, 0, 0, 1], np.uint8)
    g.push(keys, np.full(7, 1, np.int64), [vals], nulls=[nul])
    r = g.advance_watermark(A.LONG_MAX)
    assert "null1" not in r and "null0" not in r
    assert {int(k): (int(c), int(d)) for k, c, d in zip(r["key"], r["agg0"], r["agg1"])} == {1: (3, 0), 2: (4, 2)}
    g.close()


# ---- random streams against the oracle over first-occurrence columns ----

def _stream(seed, pushes, per, nkeys, nvals, span, disorder, t0=0, null_p=0.1):
    rng = np.random.default_rng(seed)
    n = pushes * per
    keys = rng.integers(0, nkeys, n).astype(np.int64)
    ts = t0 + np.sort(rng.integers(0, span, n)).astype(np.int64) - rng.integers(0, disorder + 1, n)
    cols = [rng.integers(-1000, 1000, n).astype(np.int64), rng.integers(0, nvals, n).astype(np.int64),
            rng.integers(-nvals // 2, nvals // 2, n).astype(np.int64) << 40]
    nulls = [None, (rng.random(n) < null_p).astype(np.uint8), (rng.random(n) < null_p).astype(np.uint8)]
    return keys, ts, cols, nulls


def _batches(stream, pushes, delay):
    keys, ts, cols, nulls = stream
    per, mx, out = len(keys) // pushes, I64_MIN, []
    for b in range(pushes):
        sl = slice(b * per, (b + 1) * per)
        mx = max(mx, int(ts[sl].max()))
        out.append((keys[sl], ts[sl], [c[sl] for c in cols], [None if z is None else z[sl] for z in nulls], mx - delay))
    out.append((keys[:0], ts[:0], [c[:0] for c in cols], None, A.LONG_MAX))
    return out


RANDOM_AGGS = [("COUNT", 0), ("SUM_I64", 0), ("COUNT_DISTINCT", 1), ("COUNT_DISTINCT", 2)]


@pytest.mark.parametrize("late_idx", [False, True], ids=["", "late_indices"])
@pytest.mark.parametrize("layout", ["dense", "lists"])
@pytest.mark.parametrize("zone", ["UTC", "Asia/Shanghai"])
@pytest.mark.parametrize("offset", [0, 300])
def test_random_streams_vs_reference(eng_mod, offset, zone, layout, late_idx):
    """6 pushes x 20 000 records, 50 keys x 40 values per column, out of order (up to 3 s) behind a watermark 1.5 s
    under the newest timestamp after every push, so every parameterisation drops late records and fires rows. Record
    lists are UTC-only (FWA_CFG_RECORD_LISTS): with a shift time zone the handle is refused as before."""
    tz = None if zone == "UTC" else {c["zone"]: c["tz"] for c in load_tz_kats()["timer"]}[zone]
    kw = dict(TABLE, offset_ms=offset, key_capacity=1024, nullable_cols=(1, 2), record_lists=layout == "lists")
    if tz:
        kw["tz"] = tz
    if layout == "lists" and tz:
        with pytest.raises(eng_mod.EngineError) as ei:
            eng_mod.WindowAggregator(A.make_config(aggs=RANDOM_AGGS, **kw))
        assert ei.value.code == -7
        return
    stream = _stream(11, 6, 20_000, 50, 40, 60_000, 3000, t0=1615593600000)
    rows, late, _st, _opts = run_vs_reference(eng_mod, kw, RANDOM_AGGS, 3, _batches(stream, 6, 1500),
                                              late_indices=late_idx)
    assert late > 0 and rows > 0


def test_device_async_random_stream_vs_reference(eng_mod):
    """The same stream as device tensors pushed with FWA_PUSH_ASYNC: the marked column outlives the call."""
    kw = dict(TABLE, key_capacity=1024, nullable_cols=(1, 2))
    stream = _stream(12, 4, 20_000, 50, 40, 40_000, 3000)
    rows, late, _st, _opts = run_vs_reference(eng_mod, kw, RANDOM_AGGS, 3, _batches(stream, 4, 1500), device=True,
                                              sync=False)
    assert late > 0 and rows > 0


def test_dense_two_phase_ingest_carries_the_marked_column(eng_mod):
    """2^18 records over 1000 keys with a nullable distinct column nothing else reads: its nullable bit is cleared in
    the internal configuration, so the push stays on the two-phase ingest (partition_ms > 0)."""
    rng = np.random.default_rng(5)
    n = 1 << 18
    keys = rng.integers(0, 1000, n).astype(np.int64)
    ts = np.sort(rng.integers(0, 4000, n)).astype(np.int64)
    cols = [rng.integers(0, 1 << 30, n).astype(np.int64), rng.integers(0, 50, n).astype(np.int64)]
    nulls = [None, (rng.random(n) < 0.1).astype(np.uint8)]
    aggs = [("COUNT", 0), ("SUM_I64", 0), ("COUNT_DISTINCT", 1)]
    kw = dict(TABLE, key_capacity=4096, nullable_cols=(1,))
    rows, _late, st, _opts = run_vs_reference(eng_mod, kw, aggs, 2, [(keys, ts, cols, nulls, A.LONG_MAX)])
    assert rows > 0 and st.partition_ms > 0


def test_get_config_returns_the_callers_configuration(eng_mod):
    import ctypes as C
    g = _handle(eng_mod, aggs=[("COUNT", 0), ("COUNT_DISTINCT", 2), ("SUM_I64", 2)], nullable_cols=(2,))
    out = A.Config()
    assert eng_mod.lib().fwa_get_config(g.h, C.byref(out)) == 0
    assert [(out.aggs[j].kind, out.aggs[j].col) for j in range(3)] == [(0, 0), (33, 2), (1, 2)]
    assert out.nullable_cols == 4
    g.close()


def test_slicing_window_processor_accepts_the_aggregate(eng_mod):
    """operators.SlicingWindowProcessor (the Table facade) with a COUNT(DISTINCT) column: rows per watermark, the late
    record of a fired window reported and left out of the count."""
    from flink_amd.assigners import SliceAssigners
    from flink_amd.operators import SlicingWindowProcessor
    p = SlicingWindowProcessor(SliceAssigners.tumbling(1000), [("COUNT", 0), ("COUNT_DISTINCT", 0)]).open()
    for key, v, ts in ((1, 7, 100), (1, 7, 200), (1, 8, 300), (2, 7, 400), (1, 9, 1100)):
        assert p.process_element(key, (v,), ts) is False
    assert sorted(p.advance_progress(999)) == [(1, 3, 2, 0, 1000), (2, 1, 1, 0, 1000)]
    assert p.process_element(1, (5,), 500) is True           # window [0, 1000) fired
    assert p.process_element(1, (9,), 1500) is False
    assert sorted(p.advance_progress(A.LONG_MAX)) == [(1, 2, 1, 1000, 2000)]
    assert p.num_late_records_dropped == 1
    p.close()


# ---- the reference's own numbers: WindowAggregateITCase.testEventTimeTumbleWindow with COUNT(DISTINCT string) ----

def test_itcase_tumble_row_with_all_five_aggregates(eng_mod):
    from flink_amd.keydict import KeyDictionary
    with open(os.path.join(GOLDEN, "sql_distinct_kats.json")) as f:
        case = json.load(f)["operators"][0]
    cfg = A.make_config(window_kind="TUMBLE", semantics="TABLE", size_ms=case["size_ms"], offset_ms=case["offset_ms"],
                        aggs=[tuple(a) for a in case["aggs"]], nullable_cols=case["nullable_cols"])
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
    assert dropped == case["late_dropped"] == 1
    assert len("Comment#1".encode()) == 9                        # past the 7 inline bytes: the long-string path
    g.close()
    d.close()


# ---- refusals ----

def _refused(eng_mod, **kw):
    with pytest.raises(eng_mod.EngineError) as ei:
        eng_mod.WindowAggregator(A.make_config(**kw))
    assert ei.value.code == -7 and "DISTINCT" in str(ei.value), str(ei.value)
    assert "DISTINCT" in eng_mod.lib().fwa_last_error(None).decode()


DA = [("COUNT", 0), ("COUNT_DISTINCT", 0)]


def test_refused_configurations(eng_mod):
    _refused(eng_mod, window_kind="SLIDE", semantics="TABLE", size_ms=4000, slide_ms=1000, aggs=DA)
    _refused(eng_mod, window_kind="CUMULATE", semantics="TABLE", size_ms=4000, slide_ms=1000, aggs=DA)
    _refused(eng_mod, window_kind="SESSION", semantics="TABLE", gap_ms=500, aggs=DA)
    _refused(eng_mod, window_kind="TUMBLE", semantics="DATASTREAM", size_ms=1000, aggs=DA)
    _refused(eng_mod, window_kind="TUMBLE", semantics="DATASTREAM", size_ms=1000, aggs=[("COUNT_DISTINCT", 0)], reduce=True)
    _refused(eng_mod, window_kind="TUMBLE", semantics="TABLE", size_ms=1000, aggs=DA, key_kind=A.KEY_PREHASHED)
    _refused(eng_mod, window_kind="TUMBLE", semantics="TABLE", size_ms=32, aggs=DA)     # the documented 64 ms limit
    eight = [("SUM_I64", c) for c in range(7)] + [("COUNT_DISTINCT", 0)]                # 7 read columns + the source's
    g = eng_mod.WindowAggregator(A.make_config(**TABLE, aggs=eight))                    # ... marked column: index 7
    g.close()


def test_refused_entry_points(eng_mod):
    import ctypes as C
    L = eng_mod.lib()
    g = _handle(eng_mod, output_on_device=1)
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


def test_foreign_key_group_still_raises(eng_mod):
    g = _handle(eng_mod, kg_start=0, kg_end=3)
    keys = np.arange(64, dtype=np.int64)                  # 64 keys over 128 key groups: some fall outside [0, 3]
    with pytest.raises(eng_mod.EngineError) as ei:
        g.push(keys, np.zeros(64, np.int64), [keys])
    assert ei.value.code == -3
    g.close()
