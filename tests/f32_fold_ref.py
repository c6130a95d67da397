"""Streams and the reference rule of the float32 arrival-order fold (FWA_CFG_F32_FOLD, flink_amd/csrc/f32fold.inc).

The rule: per fired (key, window), acc = +0.0f; for each accepted non-NULL record in arrival order
acc = float32(acc + v). fold_model() is that rule in numpy; test_f32_fold_cpu.py pins it to the oracle's SUM_F32, the
GPU tests compare the engine with the oracle on the same streams."""
import numpy as np

from flink_amd import _abi as A

SIZE = 1000                                    # TUMBLE 1 s
DELAY = 1500                                   # bounded out-of-orderness of the watermarks


def mixed_values(rng, n):
    """Mixed-magnitude floats N(0, 1) * exp(U(-7, 14)) with a few subnormals, +-0.0 and exact cancellations
    (x, -x in neighbouring records) sprinkled in."""
    v = (rng.standard_normal(n) * np.exp(rng.uniform(-7, 14, n))).astype(np.float32)
    pick = rng.random(n)
    v[pick < 0.01] = np.float32(1e-40) * rng.integers(1, 1000, int((pick < 0.01).sum())).astype(np.float32)
    v[(pick >= 0.01) & (pick < 0.015)] = np.float32(0.0)
    v[(pick >= 0.015) & (pick < 0.02)] = np.float32(-0.0)
    return v


def make_stream(seed=7, n=20_000, keys=40, span=20_000, pushes=12, late=0.02, ncols=1, null_frac=0.0):
    """[(keys, ts, [int64 column 0, float32 columns 1..ncols], [NULL flags per column or None], watermark)] per push.
    Records arrive in event-time order up to DELAY ms of disorder; `late` of them lag far enough to be dropped; the
    watermark after each push is the largest timestamp seen minus DELAY minus 1. A cancellation pair (x, -x) shares
    key and timestamp, so both records meet in one window."""
    rng = np.random.default_rng(seed)
    base = np.sort(rng.integers(0, span, n)).astype(np.int64)
    ts = base - rng.integers(0, DELAY, n)
    lag = rng.random(n) < late
    ts[lag] -= 3 * DELAY
    k = rng.integers(0, keys, n).astype(np.int64)
    fcols = [mixed_values(rng, n) for _ in range(ncols)]
    pair = np.nonzero(rng.random(n - 1) < 0.01)[0]
    k[pair + 1] = k[pair]
    ts[pair + 1] = ts[pair]
    for c in fcols:
        c[pair + 1] = -c[pair]
    icol = rng.integers(-1000, 1000, n).astype(np.int64)
    nulls = None
    if null_frac:
        nulls = [None] + [(rng.random(n) < null_frac).astype(np.uint8) for _ in range(ncols)]
    out = []
    edges = np.linspace(0, n, pushes + 1).astype(int)
    for p in range(pushes):
        lo, hi = edges[p], edges[p + 1]
        wm = int(base[hi - 1]) - DELAY - 1 if hi > lo else A.LONG_MIN
        out.append((k[lo:hi].copy(), ts[lo:hi].copy(), [icol[lo:hi].copy()] + [c[lo:hi].copy() for c in fcols],
                    None if nulls is None else [None] + [x[lo:hi].copy() for x in nulls[1:]], wm))
    return out


def window_start(ts, size=SIZE, offset=0):
    """TimeWindow.getWindowStartWithOffset for a tumbling window."""
    return ts - (ts - offset) % size


def fold_model(batches, col=1, size=SIZE, offset=0):
    """The rule, in numpy. Returns {(key, window_start): (float32 fold or None when no non-NULL record was accepted,
    [the accepted non-NULL values in arrival order])} over every window the stream fires, and the records dropped."""
    wm, dropped, acc, vals = A.LONG_MIN, 0, {}, {}
    for (k, t, cols, nulls, w) in batches:
        start = window_start(t, size, offset)
        nul = None if nulls is None or nulls[col] is None else nulls[col]
        for i in range(len(k)):
            if start[i] + size - 1 <= wm:                 # the window fired: dropped as late
                dropped += 1
                continue
            g = (int(k[i]), int(start[i]))
            vals.setdefault(g, [])
            if nul is not None and nul[i]:
                continue
            acc[g] = np.float32(acc.get(g, np.float32(0.0)) + cols[col][i])
            vals[g].append(cols[col][i])
        wm = max(wm, w)
    return {g: (acc.get(g), v) for g, v in vals.items()}, dropped


def f32_bits(x):
    return np.asarray(x, np.float32).view(np.uint32)
