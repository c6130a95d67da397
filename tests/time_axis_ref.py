"""A plain big-integer reference of the time axis: slice numbers, window starts and the rows of a TUMBLE and of a
DataStream SLIDE stream under one final watermark, in Python integers only (no numpy arithmetic touches a timestamp),
and the stream builder that tests/test_time_axis_cpu.py and tests/test_time_axis_gpu.py share.

The engine turns every timestamp into a slice number floor((ts - offset) / g) in about a dozen hand-written device
copies (Phase P's 32-bit and 64-bit forms, the v1 ingest, the late fire, record lists, reductions, partial rows, the
session cells) and once more on the host. The matrix below moves along that axis: slice sizes of all three modes of
jm::udiv64_make, on both sides of Phase P's g * 4096 < 2^32 bound, time bases at 0, today's epoch and +-2^62, and
first live slice numbers on both sides of +-2^40."""
import functools
import math

import numpy as np

MASK64 = (1 << 64) - 1
REL_CAP = 4096                    # Phase P's relative slice table (ingest.inc, kRelCap)
REL_TAB = 32                      # ... and the one it passes by value (engine.hip, kRelTabN)

# jm::udiv64_make modes: 0 a power of two, 1 a 64-bit magic, 2 a 65-bit magic with the add fix-up
SIZES = (1, 3, 7, 700, 1000, 60_000, 524_288, 524_289, 600_000, 900_000, 1_048_575, 1_048_576, 1_048_577, 3_600_000,
         86_400_000, 604_800_000)
BASES = (0, 1_700_000_000_000, -1_700_000_000_000, 1 << 62, -(1 << 62))
SLIDES = ((3_600_000, 600_000), (600_000, 420_000), (3_145_725, 1_048_575), (86_400_000, 3_600_000), (21, 7))


def offsets(g):
    return (0, -(g // 3), g - 1)


def wrap64(x):
    """x as a Java long (two's complement wrap-around)."""
    x &= MASK64
    return x - (1 << 64) if x >> 63 else x


def slice_number(ts, off, g):
    """floor((ts - off) / g): Python's // floors for either sign."""
    return (ts - off) // g


def slice_first_ms(q, off, g):
    return off + q * g


def window_start(ts, off, size):
    """TimeWindow.getWindowStartWithOffset without overflow: the largest off + k * size that is <= ts."""
    return ts - (ts - off) % size


def slide_slice(size, slide):
    """The slice size of a sliding window: the largest g dividing both size and slide."""
    return math.gcd(size, slide)


def tumble_rows(keys, ts, vals, off, size):
    """{(key, window start): (count, wrapped int64 sum)} of a tumbling stream in which no record is late."""
    acc = {}
    for k, t, v in zip(keys, ts, vals):
        w = (k, window_start(t, off, size))
        c, s = acc.get(w, (0, 0))
        acc[w] = (c + 1, s + v)
    return {w: (c, wrap64(s)) for w, (c, s) in acc.items()}


def slide_rows(keys, ts, vals, off, size, slide):
    """The same for SlidingEventTimeWindows.assignWindows: every start = last_start - j * slide > ts - size."""
    acc = {}
    for k, t, v in zip(keys, ts, vals):
        start = window_start(t, off, slide)
        while start > t - size:
            c, s = acc.get((k, start), (0, 0))
            acc[(k, start)] = (c + 1, s + v)
            start -= slide
    return {w: (c, wrap64(s)) for w, (c, s) in acc.items()}


def rows_as_dict(rows, size):
    """Fired [COUNT, SUM_I64] rows as {(key, start): (count, sum)}; every row's end must be start + size."""
    out = {}
    for k, s, e, c, v in zip(rows["key"].tolist(), rows["win_start"].tolist(), rows["win_end"].tolist(),
                             rows["agg0"].tolist(), rows["agg1"].tolist()):
        assert e == s + size, (k, s, e)
        assert (k, s) not in out, (k, s)
        out[(k, s)] = (c, v)
    return out


def fast_form_expected(g, q_base, has_tz, off=0):
    """The host's condition for Phase P's 32-bit division (ingest_host.inc, fill_part_args): no shift time zone, the
    relative table spans less than 2^32 ms, the first live slice number is inside +-2^40 and its first ms inside
    +-2^62."""
    if has_tz or g <= 0 or g * REL_CAP >= 1 << 32:
        return False
    if not -(1 << 40) < q_base < (1 << 40):
        return False
    b = off + q_base * g
    return -(1 << 63) // 2 < b < ((1 << 63) - 1) // 2


@functools.lru_cache(maxsize=None)
def key_pool(n_keys=3000, lo=-20_000, hi=20_000, seed=5):
    return np.random.default_rng(seed).permutation(np.arange(lo, hi, dtype=np.int64))[:n_keys]


def build_stream(base, off, g, n, seed, slices=range(-3, 4), keys=None, wide=False, edges_only=False):
    """n records around time `base`: each falls in one of the slices q0 + d, d in `slices`, q0 = floor((base - off) / g)
    -- at the slice's first ms, its second, its middle, its last, or (two in six) a random one. Keys come from `keys`
    (default about 3000 values in +-20 000); BIGINT values span the signed 32-bit range without its two lowest values,
    so narrow bucket entries stay narrow. wide: keys and values that need 64 bits. edges_only: first and last ms only.
    Returns (keys, ts, values) as int64 arrays; every timestamp is computed in Python integers."""
    rng = np.random.default_rng(seed)
    pool = key_pool() if keys is None else keys
    q0 = slice_number(base, off, g)
    first = [slice_first_ms(q0 + d, off, g) for d in slices]
    which = rng.integers(0, len(first), n).tolist()
    fixed = (0, min(1, g - 1), g // 2, g - 1)
    kind = rng.integers(0, 2 if edges_only else 6, n).tolist()
    rnd = rng.integers(0, g, n).tolist()
    if edges_only:
        pos = [0 if c == 0 else g - 1 for c in kind]
    else:
        pos = [fixed[c] if c < 4 else r for c, r in zip(kind, rnd)]
    ts = [first[w] + p for w, p in zip(which, pos)]
    assert all(-(1 << 63) < t < (1 << 63) - 1 for t in ts)
    k = rng.choice(pool, n).astype(np.int64)
    v = rng.integers(-(1 << 31) + 2, 1 << 31, n).astype(np.int64)
    if wide:                                               # bit 40 set in every key, values past 32 bits
        k = k ^ np.int64(1 << 40)
        v = v * np.int64(1 << 20) + np.int64(12345)
    return k, np.array(ts, dtype=np.int64), v
