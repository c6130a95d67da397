"""SUM(FLOAT) as the reference's float32 arrival-order fold on the GPU (FWA_CFG_F32_FOLD, flink_amd/csrc/f32fold.inc).

Every case compares all rows exactly (assert_rows_equal(..., rtol=None)) with an Oracle built from the same
configuration without the flag: the oracle's SUM_F32 is the arrival-order float32 fold (test_f32_fold_cpu.py pins that,
and that more than a quarter of these streams' rows differ from a float64 sum rounded once, which is what the engine
returns without the flag). Late-drop totals must be equal too."""
import numpy as np
import pytest

from f32_fold_ref import SIZE, make_stream, mixed_values
from flink_amd import _abi as A
from flink_amd.operators import reduction_aggs
from helpers import assert_rows_equal, load_tz_kats

pytestmark = pytest.mark.gpu

AGGS = [("COUNT", 0), ("SUM_F32", 1), ("MIN_F32", 1), ("AVG_F32", 1), ("SUM_I64", 0)]
TUMBLE = dict(window_kind="TUMBLE", size_ms=SIZE, key_capacity=1 << 15)
TABLE = dict(TUMBLE, semantics="TABLE")
STREAM = dict(TUMBLE, semantics="DATASTREAM")


@pytest.fixture(scope="module")
def eng_mod():
    from flink_amd import engine
    engine.lib()
    return engine


@pytest.fixture(scope="module")
def stream():
    return make_stream(seed=7)


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def run_vs_oracle(eng_mod, cfg_kw, batches, mode="host", options=None, final=True):
    """Push `batches` through a handle with the flag and an oracle without it, a watermark after each push, then
    Long.MAX_VALUE; every step's rows and the late-drop totals must be equal. Returns the engine's rebuild count."""
    from oracle.oracle import Oracle
    off = A.make_config(**cfg_kw)
    names = A.agg_names(off)
    g = eng_mod.WindowAggregator(A.make_config(f32_fold=True, **cfg_kw), options=options)
    o = Oracle(off)
    late_o, rows, keep = 0, 0, []
    steps = list(batches) + ([(None, None, None, None, A.LONG_MAX)] if final else [])
    for step, (k, t, cols, nulls, wm) in enumerate(steps):
        if k is not None:
            late_o += o.push(k, t, cols, nulls=nulls)
            if mode == "host":
                g.push(k, t, cols, nulls=nulls)
            else:
                dev = (_dev(k), _dev(t), [_dev(c) for c in cols], None if nulls is None else [_dev(x) for x in nulls])
                keep.append(dev)
                g.push(dev[0], dev[1], dev[2], nulls=dev[3], sync=mode != "async")
        if mode == "async":
            g.advance_watermark_async(wm)
            rg = g.fired_output()
        else:
            rg = g.advance_watermark(wm)
        ro = o.advance_watermark(wm)
        assert_rows_equal(rg, ro, names, rtol=None, ctx="step %d wm=%d" % (step, wm))
        rows += len(ro["key"])
    assert g.stats().late_dropped == late_o
    rebuilds = g.get_option("f32_fold_rebuilds")
    g.close()
    o.close()
    assert rows > 0
    return rebuilds


# ---- 1: the parity matrix ----

@pytest.mark.parametrize("mode", ["host", "device", "async"])
@pytest.mark.parametrize("sem", ["table_offset", "datastream"])
def test_parity_matrix(eng_mod, stream, sem, mode):
    kw = dict(TABLE, offset_ms=250) if sem == "table_offset" else STREAM
    run_vs_oracle(eng_mod, dict(kw, aggs=AGGS), stream, mode=mode)


# ---- 2: two folded columns, and two SUM_F32 over one column ----

def test_two_columns_and_a_shared_fold(eng_mod):
    aggs = [("SUM_F32", 1), ("COUNT", 0), ("SUM_F32", 2), ("SUM_F32", 1), ("MAX_F32", 2)]
    batches = make_stream(seed=11, ncols=2)
    for kw in (TABLE, STREAM):
        run_vs_oracle(eng_mod, dict(kw, aggs=aggs), batches)


# ---- 3: nullable column ----

def test_nullable_column(eng_mod):
    batches = make_stream(seed=9, null_frac=0.1)
    k, t, cols, nulls, wm = batches[0]
    extra = 5                                               # key 999: a window holding only NULLs -> a NULL result
    batches[0] = (np.concatenate([k, np.full(extra, 999, np.int64)]), np.concatenate([t, np.full(extra, int(t.max()), np.int64)]),
                  [np.concatenate([cols[0], np.zeros(extra, np.int64)]), np.concatenate([cols[1], np.ones(extra, np.float32)])],
                  [None, np.concatenate([nulls[1], np.ones(extra, np.uint8)])], wm)
    from oracle.oracle import Oracle
    cfg_kw = dict(TABLE, aggs=AGGS, nullable_cols=(1,))
    o = Oracle(A.make_config(**cfg_kw))
    o.push(*batches[0][:3], nulls=batches[0][3])
    r = o.advance_watermark(A.LONG_MAX)
    o.close()
    assert r["null1"][r["key"] == 999].all() and not r["null1"][r["key"] != 999].all()
    for mode in ("host", "device"):
        run_vs_oracle(eng_mod, cfg_kw, batches, mode=mode)


# ---- 4: reduce handles ----

@pytest.mark.parametrize("types,pos", [(("F32", "I64"), 1), (("F32", "F32", "I64"), 2)], ids=["tuple3", "two_floats"])
def test_reduce_handle_sum_of_a_float_field(eng_mod, types, pos):
    rng = np.random.default_rng(13)
    batches = []
    for (k, t, cols, _, wm) in make_stream(seed=13):
        fields = [mixed_values(rng, len(k)) if ty == "F32" else cols[0] for ty in types]
        fields[pos - 1] = cols[1]
        batches.append((k, t, fields, None, wm))
    run_vs_oracle(eng_mod, dict(STREAM, aggs=reduction_aggs("sum", pos, types), reduce=True), batches)


# ---- 5: run shapes ----

def _one_push(keys, ts, seed):
    rng = np.random.default_rng(seed)
    n = len(keys)
    return [(keys, ts, [rng.integers(-9, 9, n).astype(np.int64), mixed_values(rng, n)], None, int(ts.max()) - 1)]


def test_one_key_holds_the_whole_batch(eng_mod):
    n = 20_000
    run_vs_oracle(eng_mod, dict(STREAM, aggs=AGGS), _one_push(np.full(n, 5, np.int64), np.arange(n, dtype=np.int64) % SIZE, 1))


def test_every_run_has_one_record(eng_mod):
    n = 20_000
    keys = np.random.default_rng(2).permutation(n).astype(np.int64) - 100      # (key 0 and negative keys included)
    run_vs_oracle(eng_mod, dict(STREAM, aggs=AGGS), _one_push(keys, np.full(n, 10, np.int64), 2))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_small_batches(eng_mod, n):
    rng = np.random.default_rng(n)
    batches = []
    for p in range(3):
        keys = rng.integers(0, 7, n).astype(np.int64)
        ts = rng.integers(0, 2 * SIZE, n).astype(np.int64) + p * SIZE
        batches += [(keys, ts, [keys.copy(), mixed_values(rng, n)], None, p * SIZE - 1)]
    run_vs_oracle(eng_mod, dict(TABLE, aggs=AGGS), batches)


def test_empty_push(eng_mod, stream):
    k, t, cols, nulls, wm = stream[0]
    empty = (k[:0], t[:0], [c[:0] for c in cols], None, wm - 1)
    run_vs_oracle(eng_mod, dict(STREAM, aggs=AGGS), [empty, stream[0], empty, stream[1]])
    run_vs_oracle(eng_mod, dict(STREAM, aggs=AGGS), [empty, stream[0], empty, stream[1]], mode="device")


# ---- 6: a fold carried over pushes ----

def test_fold_continues_over_pushes(eng_mod):
    rng = np.random.default_rng(6)
    batches = []
    for p in range(12):
        keys = np.repeat(np.arange(40, dtype=np.int64), 5)
        rng.shuffle(keys)
        n = len(keys)
        batches.append((keys, rng.integers(0, SIZE, n).astype(np.int64), [keys.copy(), mixed_values(rng, n)], None, -1))
    run_vs_oracle(eng_mod, dict(TABLE, aggs=AGGS), batches)


# ---- 7: set growth and rebuild ----

@pytest.mark.parametrize("keys", [40, 5000])
def test_growth_and_rebuild_from_the_smallest_set(eng_mod, stream, keys):
    batches = stream if keys == 40 else make_stream(seed=17, keys=keys)
    g = eng_mod.WindowAggregator(A.make_config(f32_fold=True, aggs=AGGS, **STREAM), options={"f32_fold_slots": 64})
    assert g.get_option("f32_fold_slots") == 64 and g.get_option("f32_fold_rebuilds") == 0
    g.close()
    rebuilds = run_vs_oracle(eng_mod, dict(STREAM, aggs=AGGS), batches, options={"f32_fold_slots": 64})
    assert rebuilds >= (2 if keys == 40 else 3)            # growth from 64 slots, then rebuilds after windows fired


# ---- 8: record lists ----

def test_record_lists(eng_mod, stream):
    for kw in (TABLE, STREAM):
        g = eng_mod.WindowAggregator(A.make_config(f32_fold=True, aggs=AGGS, record_lists=True, **kw))
        assert g.record_lists
        g.close()
        run_vs_oracle(eng_mod, dict(kw, aggs=AGGS, record_lists=True), stream)


# ---- 9: shift time zone ----

def test_shift_time_zone_across_dst(eng_mod):
    tz = {c["zone"]: c["tz"] for c in load_tz_kats()["timer"]}["America/Los_Angeles"]
    rng = np.random.default_rng(19)
    batches = []
    for t0 in (1615593600000, 1636156800000):             # 2021-03-13 and 2021-11-06, 00:00 UTC
        n = 6000
        base = t0 + np.sort(rng.integers(0, 3 * 86_400_000, n)).astype(np.int64)
        ts = base - rng.integers(0, 600_000, n)
        keys = rng.integers(0, 8, n).astype(np.int64)
        vi, vf = rng.integers(-1000, 1000, n).astype(np.int64), mixed_values(rng, n)
        for b in range(12):
            sl = slice(b * n // 12, (b + 1) * n // 12)
            batches.append((keys[sl], ts[sl], [vi[sl], vf[sl]], None, int(ts[sl].max()) - 600_001))
    run_vs_oracle(eng_mod, dict(window_kind="TUMBLE", semantics="TABLE", size_ms=3_600_000, tz=tz, aggs=AGGS,
                                key_capacity=2048), batches)


# ---- 10: snapshot / restore ----

@pytest.mark.parametrize("sem", ["table", "datastream"])
def test_snapshot_restore_with_rescale(eng_mod, stream, sem):
    from flink_amd import snapshot as S
    from oracle.oracle import Oracle
    kw = dict(TABLE if sem == "table" else STREAM, aggs=AGGS)
    names = [a[0] for a in AGGS]
    o = Oracle(A.make_config(**kw))
    g = eng_mod.WindowAggregator(A.make_config(f32_fold=True, **kw))
    for (k, t, cols, _, wm) in stream[:6]:
        o.push(k, t, cols)
        g.push(k, t, cols)
        assert_rows_equal(g.advance_watermark(wm), o.advance_watermark(wm), names)
    wm6 = stream[5][4]
    assert (wm6 + 1) % SIZE != 0                           # inside a window: its fold continues after the checkpoint
    blob = g.snapshot()
    g.close()
    late2, ref = 0, []
    for (k, t, cols, _, wm) in stream[6:]:
        late2 += o.push(k, t, cols)
        ref.append(o.advance_watermark(wm))
    ref.append(o.advance_watermark(A.LONG_MAX))
    o.close()
    ref = {f: np.concatenate([r[f] for r in ref]) for f in ref[0]}
    assert late2 > 0
    snap = S.parse(blob)
    f = snap["f32_fold"]
    assert f["agg_mask"] == 2 and f["n"] > 0 and (f["column"] == 0).all() and snap["watermark"] == wm6
    assert (f["slice_start"] + SIZE - 1 > wm6).all() and int(f["kg_offsets"][-1]) == f["n"]
    for layout in ([(0, 127)], [(0, 31), (32, 127)]):
        outs, late = [], 0
        for lo, hi in layout:
            h = eng_mod.WindowAggregator(A.make_config(f32_fold=True, kg_start=lo, kg_end=hi, **kw))
            h.restore(blob)
            for (k, t, cols, _, wm) in stream[6:] + [(None, None, None, None, A.LONG_MAX)]:
                if k is not None:
                    m = eng_mod.key_groups(k, 128, 1, A.KEY_JAVA_LONG)[0]
                    m = (m >= lo) & (m <= hi)
                    late += h.push(k[m], t[m], [c[m] for c in cols])
                outs.append(h.advance_watermark(wm))
            h.close()
        assert late == late2
        assert_rows_equal({f: np.concatenate([r[f] for r in outs]) for f in outs[0]}, ref, names)


def test_blobs_with_and_without_the_flag_do_not_mix(eng_mod, stream):
    k, t, cols, _, _ = stream[0]
    kw = dict(TABLE, aggs=AGGS)
    blobs = {}
    for flag in (False, True):
        g = eng_mod.WindowAggregator(A.make_config(f32_fold=flag, **kw))
        g.push(k, t, cols)
        blobs[flag] = g.snapshot()
        g.close()
    for flag in (False, True):
        h = eng_mod.WindowAggregator(A.make_config(f32_fold=flag, **kw))
        with pytest.raises(eng_mod.EngineError, match="header word 29") as ei:
            h.restore(blobs[not flag])
        assert ei.value.code == -1
        h.restore(blobs[flag])                             # ... and its own kind is accepted
        h.close()


# ---- 11: without the flag nothing changes ----

def test_without_the_flag_nothing_changes(eng_mod, stream):
    from oracle.oracle import Oracle
    cfg_kw = dict(STREAM, aggs=AGGS)
    names = [a[0] for a in AGGS]
    a, b, o = (eng_mod.WindowAggregator(A.make_config(**cfg_kw)), eng_mod.WindowAggregator(A.make_config(**cfg_kw)),
               Oracle(A.make_config(**cfg_kw)))
    tol = {"SUM_F32": 2e-4, "AVG_F32": 1e-6}               # tests/test_gpu_parity.py TOL
    for (k, t, cols, _, wm) in stream:
        for h in (a, b, o):
            h.push(k, t, cols)
        ra, rb, ro = a.advance_watermark(wm), b.advance_watermark(wm), o.advance_watermark(wm)
        assert_rows_equal(ra, ro, names, rtol=lambda name: tol.get(name, 0.0))
        assert_rows_equal(rb, ro, names, rtol=lambda name: tol.get(name, 0.0))
    assert a.stats().ingest_launches == b.stats().ingest_launches > 0
    with pytest.raises(eng_mod.EngineError) as ei:
        a.get_option("f32_fold_slots")
    assert ei.value.code == -7
    for h in (a, b, o):
        h.close()
    # the flag on a handle without a SUM_F32 aggregate is accepted and does nothing
    h = eng_mod.WindowAggregator(A.make_config(window_kind="SLIDE", size_ms=2000, slide_ms=1000, f32_fold=True,
                                               aggs=[("COUNT", 0), ("AVG_F32", 1)]))
    with pytest.raises(eng_mod.EngineError):
        h.get_option("f32_fold_slots")
    h.close()


# ---- 12: refusals ----

REFUSED = {
    "datastream_slide": dict(window_kind="SLIDE", size_ms=2000, slide_ms=1000),
    "table_hop": dict(window_kind="SLIDE", semantics="TABLE", size_ms=2000, slide_ms=1000),
    "table_cumulate": dict(window_kind="CUMULATE", semantics="TABLE", size_ms=4000, slide_ms=1000),
    "session": dict(window_kind="SESSION", gap_ms=1000),
    "table_session": dict(window_kind="SESSION", semantics="TABLE", gap_ms=1000),
    "allowed_lateness": dict(window_kind="TUMBLE", size_ms=1000, allowed_lateness_ms=500),
    "prehashed": dict(window_kind="TUMBLE", size_ms=1000, key_kind=A.KEY_PREHASHED),
    "with_distinct": dict(window_kind="TUMBLE", semantics="TABLE", size_ms=1000,
                          aggs=[("SUM_F32", 1), ("COUNT_DISTINCT", 0)]),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_configurations(eng_mod, name):
    kw = dict(aggs=[("COUNT", 0), ("SUM_F32", 1)])
    kw.update(REFUSED[name])
    with pytest.raises(eng_mod.EngineError, match="FWA_CFG_F32_FOLD") as ei:
        eng_mod.WindowAggregator(A.make_config(f32_fold=True, **kw))
    assert ei.value.code == -7
    eng_mod.WindowAggregator(A.make_config(**kw)).close()   # the flag is what is refused


def test_refused_entry_points(eng_mod, stream):
    k, t, cols, _, wm = stream[0]
    g = eng_mod.WindowAggregator(A.make_config(f32_fold=True, semantics="TABLE", window_kind="TUMBLE", size_ms=SIZE,
                                               aggs=[("COUNT", 0), ("SUM_F32", 1)]))
    g.push(k, t, cols)
    for call in (lambda: g.drain_partials(wm), lambda: g.drain_route(wm, 2), lambda: g.snapshot_heap(),
                 lambda: g.push_partials(k[:1], t[:1], k[:1], [k[:1], k[:1]])):
        with pytest.raises(eng_mod.EngineError, match="FWA_CFG_F32_FOLD") as ei:
            call()
        assert ei.value.code == -7
    g.close()
