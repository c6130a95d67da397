"""GPU tests: the tumbling fire that walks a watermark's windows per key chunk and retires their slots in the same
pass (fire_walk_kernel), against the oracle. The sizes are the smallest that reach the edges:
key capacities whose capacity + 1 is no multiple of the kernel's key chunk (with Long.MIN_VALUE in the side slot),
the window count at which the window table leaves the kernel arguments, slots recycled after the fire cleared them,
a failed speculation, allowed lateness (fired slots stay), output regrowth and the A/B switch."""
import numpy as np
import pytest

from flink_amd import _abi as A
from helpers import assert_rows_equal

pytestmark = pytest.mark.gpu

LONG_MIN = -2**63
SUM2 = [("COUNT", 0), ("SUM_I64", 0)]
MINMAX = [("COUNT", 0), ("SUM_I64", 0), ("MIN_I64", 0), ("MAX_I64", 0)]
OLD_FIRE = 256                                  # FWA_OPT_INGEST_VARIANT bit 8


def _stream(seed, n, nkeys, span, delay, nb, late_frac=0.0, min_key_frac=0.0):
    """nb batches (keys, ts, vals, watermark) of an almost ordered stream; a share of the records carries the key
    Long.MIN_VALUE, a share is late by more than the watermark delay."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, nkeys, n).astype(np.int64)
    keys[rng.random(n) < min_key_frac] = LONG_MIN
    ts = np.sort(rng.integers(0, span, n)).astype(np.int64) - rng.integers(0, delay + 1, n)
    late = rng.random(n) < late_frac
    ts[late] -= rng.integers(delay, 4 * delay + 1, late.sum())
    vals = rng.integers(-2**31, 2**31, n).astype(np.int64)
    out, mx = [], -2**63
    for b in range(nb):
        sl = slice(b * n // nb, (b + 1) * n // nb)
        mx = max(mx, int(ts[sl].max()))
        out.append((keys[sl], ts[sl], vals[sl], mx - delay - 1))
    return out


_EXPECTED = {}


def _expected(tag, kw, batches):
    """The oracle's rows per watermark (the last one Long.MAX_VALUE) and its late drops: computed once per stream."""
    if tag not in _EXPECTED:
        from oracle.oracle import Oracle
        o = Oracle(A.make_config(**kw))
        rows = []
        for k, t, v, wm in batches:
            o.push(k, t, [v])
            rows.append(o.advance_watermark(wm))
        rows.append(o.advance_watermark(A.LONG_MAX))
        _EXPECTED[tag] = (rows, o.stats().late_dropped)
        o.close()
    return _EXPECTED[tag]


def _run(kw, batches, mode, options=None):
    """Push the batches and advance the watermark after each one, pipelined (asynchronous push and watermark, device
    inputs) or synchronous (host inputs); returns (rows per watermark, stats, fused fires, slot-reset launches)."""
    import torch
    from flink_amd import engine
    g = engine.WindowAggregator(A.make_config(output_on_device=1 if mode == "async" else 0, **kw), options)
    got = []
    if mode == "async":
        dev = [(torch.from_numpy(k).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(v).cuda()) for k, t, v, _ in batches]
        for b, (k, t, v) in enumerate(dev):
            g.push(k, t, [v], sync=False)
            if b > 0:
                got.append(g.fired_output())
            g.advance_watermark_async(batches[b][3])
        got.append(g.fired_output())
        g.advance_watermark_async(A.LONG_MAX)
        got.append(g.fired_output())
    else:
        for k, t, v, wm in batches:
            g.push(k, t, [v])
            got.append(g.advance_watermark(wm))
        got.append(g.advance_watermark(A.LONG_MAX))
    st = g.stats()
    fused, resets = g.get_option("fused_fires"), g.get_option("reset_launches")
    g.close()
    return got, st, fused, resets


def _check(tag, kw, batches, mode, options=None):
    exp, late = _expected(tag, kw, batches)
    got, st, fused, resets = _run(kw, batches, mode, options)
    names = A.agg_names(A.make_config(**kw))
    assert len(got) == len(exp)
    for b, (rg, ro) in enumerate(zip(got, exp)):
        assert_rows_equal(rg, ro, names, ctx="%s watermark %d" % (tag, b))
    assert st.records_in == sum(len(k) for k, _, _, _ in batches)
    assert st.late_dropped == late
    return st, fused, resets


@pytest.mark.parametrize("mode", ["async", "sync"])
@pytest.mark.parametrize("aggs", [SUM2, MINMAX], ids=["sum", "minmax"])
@pytest.mark.parametrize("kc", [64, 1024, 5000])
def test_kid_chunk_edges_with_side_slot(kc, aggs, mode):
    """capacity + 1 keys end inside a chunk (and inside a 16-byte pair); Long.MIN_VALUE lives at index capacity. Six
    rounds, so later slices land in slots the fire cleared: a stale COUNT / SUM / MIN / MAX would show in the rows."""
    kw = dict(window_kind="TUMBLE", size_ms=1_000, aggs=aggs, key_capacity=kc)
    batches = _stream(11 + kc, 1 << 14, kc - 1, 12_000, 300, 6, min_key_frac=1 / 16)
    _, fused, _ = _check("edges-%d-%d" % (kc, len(aggs)), kw, batches, mode)
    assert fused > 0


def _windows_at_one_watermark(w):
    """Round 0 fills and fires window [0, 1000); round 1 fills w windows of 1 s and one late watermark fires them all."""
    rng = np.random.default_rng(5 + w)
    out = []
    for lo, hi in ((0, 1_000), (1_000, 1_000 + 1_000 * w)):
        n = 4096
        out.append((rng.integers(0, 700, n).astype(np.int64), rng.integers(lo, hi, n).astype(np.int64),
                    rng.integers(-2**31, 2**31, n).astype(np.int64), hi - 1))
    return out


@pytest.mark.parametrize("mode", ["async", "sync"])
@pytest.mark.parametrize("w", [1, 2, 8, 9])
def test_window_table_by_value_limit(w, mode):
    """Up to 8 windows travel in the kernel arguments and are retired by the fire; 9 take the uploaded table, the
    per-window kernels and the separate slot reset."""
    kw = dict(window_kind="TUMBLE", size_ms=1_000, aggs=SUM2, key_capacity=1024)
    _, fused, resets = _check("limit-%d" % w, kw, _windows_at_one_watermark(w), mode)
    assert fused == (2 if w <= 8 else 1)        # round 0's window, and round 1's when they fit
    assert (resets > 0) == (w > 8)


@pytest.mark.parametrize("aggs", [SUM2, MINMAX], ids=["sum", "minmax"])
def test_failed_speculation_clears_nothing(aggs):
    """The first push of a handle replays its slice misses, and batch 2 holds records whose key and value need 64 bits
    on a narrow handle: the asynchronous fires behind those pushes are discarded and must neither emit nor clear; the
    rows of those and of the following watermarks equal the oracle's."""
    kw = dict(window_kind="TUMBLE", size_ms=1_000, aggs=aggs, key_capacity=1024)
    batches = _stream(23, 1 << 14, 900, 12_000, 300, 6)
    k, t, v, wm = batches[2]
    k, v = k.copy(), v.copy()
    k[:3] = 2**40 + 7
    v[3:6] = 2**62 + 5
    batches[2] = (k, t, v, wm)
    st, fused, _ = _check("spec-%d" % len(aggs), kw, batches, "async")
    assert st.replay_records > 0 and fused > 0


@pytest.mark.parametrize("mode", ["async", "sync"])
def test_allowed_lateness_keeps_fired_slots(mode):
    """Allowed lateness 2 s: a fired window still takes late records, so its slot is not cleared by the fire; the late
    firings equal the oracle's."""
    kw = dict(window_kind="TUMBLE", semantics="DATASTREAM", size_ms=1_000, aggs=SUM2, key_capacity=1024,
              allowed_lateness_ms=2_000)
    batches = _stream(29, 1 << 14, 900, 12_000, 300, 6, late_frac=0.02)
    _check("lateness", kw, batches, mode)


@pytest.mark.parametrize("mode", ["async", "sync"])
def test_output_growth_relaunches_without_clearing(mode):
    """out_min_rows forced small: the first fires count their rows, grow the output columns and fire again, which only
    a non-clearing fire may do."""
    kw = dict(window_kind="TUMBLE", size_ms=1_000, aggs=SUM2, key_capacity=1024)
    batches = _stream(31, 1 << 14, 900, 12_000, 300, 6)
    _check("growth", kw, batches, mode, options={"out_min_rows": 64})


@pytest.mark.parametrize("span_s", [1, 40])
def test_slice_span_of_one_push(span_s):
    """One push whose live slices span a single slice, and one spanning 40 (more than 32 relative slices); a later
    push mixes late records in, and the late drops are counted as the oracle counts them."""
    rng = np.random.default_rng(37 + span_s)
    n = 8192
    first = (rng.integers(0, 900, n).astype(np.int64), np.sort(rng.integers(0, 1_000 * span_s, n)).astype(np.int64),
             rng.integers(-2**31, 2**31, n).astype(np.int64), 1_000 * span_s - 1)
    second = (rng.integers(0, 900, n).astype(np.int64), rng.integers(0, 1_000 * (span_s + 1), n).astype(np.int64),
              rng.integers(-2**31, 2**31, n).astype(np.int64), 1_000 * (span_s + 1) - 1)
    kw = dict(window_kind="TUMBLE", size_ms=1_000, aggs=SUM2, key_capacity=1024)
    for mode in ("async", "sync"):
        st, _, _ = _check("span-%d" % span_s, kw, [first, second], mode)
        assert st.late_dropped > 0


@pytest.mark.parametrize("aggs", [SUM2, MINMAX], ids=["sum", "minmax"])
def test_ab_bit_restores_the_separate_reset(aggs):
    """Variant bit 8: the same stream gives the same rows through the per-window fire and reset_slots_kernel."""
    kw = dict(window_kind="TUMBLE", size_ms=1_000, aggs=aggs, key_capacity=1024)
    batches = _stream(23, 1 << 14, 900, 12_000, 300, 6)
    for mode in ("async", "sync"):
        _, fused, resets = _check("spec-ab-%d" % len(aggs), kw, batches, mode, options={"ingest_variant": OLD_FIRE})
        assert fused == 0 and resets > 0
