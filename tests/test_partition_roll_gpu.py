"""Phase P's rolling issue of the next tile's loads (partition3 ROLL, DESIGN.md §5 "Rolling tile loads") against the
oracle and against the previous order on the same build (FWA_OPT_INGEST_VARIANT bit 10). Every case runs both orders:
rows are bit-exact with the oracle and with each other, late drops per push and replayed records agree.

What can go wrong is a pair's registers being overwritten before their last use, and the tile-edge arithmetic, so the
record counts sit on tile and grid edges (tile = 1024 lanes x ITEMS records, grid = min(tiles, 256) blocks, a block's
last tile reloads itself), and the records of the cold branches -- the ones that wait for every load in flight -- sit
in the last pair of a tile and the first pair of the next. A push reaches Phase P's buckets only for slices that exist,
so every case first pushes one record per slice."""
import functools

import numpy as np
import pytest

from flink_amd import _abi as A
from helpers import assert_rows_equal

pytestmark = pytest.mark.gpu

PARENT_ORDER = 1024                # FWA_OPT_INGEST_VARIANT bit 10
CAP = 1 << 15
GRID = 256
SIZE_MS = 1000
SLICES = 3                         # seeded slices 0..2; slice 0 is fired (late) before the main push
UNSEEDED = 5                       # a slice inside the relative range without a slot (kCodeSlow)
FAR_TS = 10**12 + 7                # outside the 32-bit division range: the exact 64-bit division
OPTS = {"narrow_entries": 1, "skew_merge": 0, "window_passes": 0}

# handle: (aggregates, semantics, records per tile, value column dtypes)
NARROW = ([("COUNT", 0), ("SUM_I64", 0)], "DATASTREAM", 6 * 1024, ("i8",))
NARROW2 = ([("COUNT", 0), ("SUM_F64", 1), ("AVG_F64", 1), ("MAX_F32", 0), ("MAX_F64", 1)], "TABLE", 4 * 1024,
           ("f4", "f8"))
COUNT_ONLY = ([("COUNT", 0)], "DATASTREAM", 8 * 1024, ("i8",))


@pytest.fixture(scope="module")
def eng_mod():
    from flink_amd import engine
    engine.lib()
    return engine


@functools.lru_cache(maxsize=None)
def key_pool():
    return np.random.default_rng(21).permutation(np.arange(-(1 << 16), 1 << 16, dtype=np.int64))[:12_000]


def make_cfg(handle):
    aggs, sem, _, _ = handle
    return A.make_config(window_kind="TUMBLE", semantics=sem, size_ms=SIZE_MS, aggs=aggs, key_capacity=CAP)


def seed_push(handle, slices=SLICES):
    ts = np.arange(slices, dtype=np.int64) * SIZE_MS + 1
    return np.full(slices, int(key_pool()[0]), np.int64), ts, [np.ones(slices, np.dtype(d)) for d in handle[3]]


def records(handle, n, seed, lo_slice=1, hi_slice=SLICES):
    """n records over the key pool, timestamps ascending over slices [lo_slice, hi_slice). Float columns hold small
    integers, so every sum is exact in any order."""
    rng = np.random.default_rng(seed)
    k = rng.choice(key_pool(), n).astype(np.int64)
    ts = np.sort(rng.integers(lo_slice * SIZE_MS, hi_slice * SIZE_MS, n)).astype(np.int64)
    cols = []
    for d in handle[3]:
        if d == "i8":
            cols.append(rng.integers(-2**31, 2**31, n).astype(np.int64))
        else:
            cols.append(rng.integers(-1000, 1000, n).astype(np.dtype(d)))
    return k, ts, cols


def plant_specials(handle, k, ts, cols):
    """The five cold-branch records around tile boundaries -- the last pair of a tile (b - 2, b - 1) and the first pair
    of the next (b, b + 1) -- rotated so that each kind meets each of the four places, at the first boundaries and at
    the last ones of the push (a block's last tile). Returns how many of each kind were planted."""
    n, tile = len(k), handle[2]
    bounds = [b for b in range(tile, n - 1, tile)]
    if len(bounds) > 10:
        bounds = bounds[:5] + bounds[-5:]
    kinds = ["late", "wide_key", "wide_val", "far_ts", "no_slot"]
    planted = dict.fromkeys(kinds, 0)
    for bi, b in enumerate(bounds):
        for off in (-2, -1, 0, 1):
            i = b + off
            if not 0 <= i < n:
                continue
            kind = kinds[(bi + off + 2) % len(kinds)]
            if kind == "late":
                ts[i] = 5                                   # slice 0: fired by the watermark ahead of the push
            elif kind == "wide_key":
                k[i] = (1 << 40) + i
            elif kind == "wide_val":
                if cols[0].dtype != np.int64:
                    continue
                cols[0][i] = (1 << 40) + i
            elif kind == "far_ts":
                ts[i] = FAR_TS
            else:
                ts[i] = UNSEEDED * SIZE_MS + 3
            planted[kind] += 1
    return planted


def run_gpu(eng_mod, handle, steps, variant, to_device=None, sync=True, opts=OPTS):
    """steps: ("push", keys, ts, cols) / ("wm", watermark). Returns late drops per push, the rows of every watermark
    and of the final one, and the counters the orders are compared on."""
    g = eng_mod.WindowAggregator(make_cfg(handle), options=dict(opts, ingest_variant=variant))
    res = {"late": [], "rows": []}
    try:
        assert g.get_option("ingest_variant") == variant
        for st in steps:
            if st[0] == "push":
                _, k, t, cols = st
                if to_device is not None:
                    k, t, cols = to_device(k, t, cols)
                res["late"].append(g.push(k, t, cols, sync=sync))
            else:
                res["rows"].append(g.advance_watermark(st[1]))
        res["rows"].append(g.advance_watermark(A.LONG_MAX))
        s = g.stats()
        assert s.partition_ms > 0, "the two-phase ingest did not run"
        res.update(late_total=s.late_dropped, replay=s.replay_records, records_in=s.records_in,
                   narrow=g.get_option("narrow_entries"))
        return res
    finally:
        g.close()


def run_oracle(handle, steps):
    from oracle.oracle import Oracle
    o = Oracle(make_cfg(handle))
    res = {"late": [], "rows": []}
    for st in steps:
        if st[0] == "push":
            res["late"].append(o.push(st[1], st[2], st[3]))
        else:
            res["rows"].append(o.advance_watermark(st[1]))
    res["rows"].append(o.advance_watermark(A.LONG_MAX))
    o.close()
    return res


def sorted_rows(rows, names):
    order = np.lexsort((rows["key"], rows["win_start"], rows["win_end"]))
    return [rows[f][order] for f in ["win_end", "win_start", "key"] + ["agg%d" % j for j in range(len(names))]]


def both_orders(eng_mod, handle, steps, to_device=None, sync=True, opts=OPTS):
    """The oracle once, then the rolling order and the previous one."""
    names = A.agg_names(make_cfg(handle))
    want = run_oracle(handle, steps)
    out = []
    for variant in (0, PARENT_ORDER):
        r = run_gpu(eng_mod, handle, steps, variant, to_device, sync, opts)
        if sync:
            assert r["late"] == want["late"], "variant %d late drops per push" % variant
        assert r["late_total"] == sum(want["late"]), "variant %d late drops" % variant
        assert len(r["rows"]) == len(want["rows"])
        for i, (a, b) in enumerate(zip(r["rows"], want["rows"])):
            assert_rows_equal(a, b, names, ctx="variant %d watermark %d" % (variant, i))
        out.append(r)
    new, old = out
    for a, b in zip(new["rows"], old["rows"]):              # row for row, sorted by (win_end, win_start, key)
        for x, y in zip(sorted_rows(a, names), sorted_rows(b, names)):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
    for f in ("late", "late_total", "replay", "records_in", "narrow"):
        assert new[f] == old[f], f
    return new


def main_steps(handle, n, seed, specials=True):
    k, ts, cols = records(handle, n, seed)
    planted = plant_specials(handle, k, ts, cols) if specials else {}
    sk, st, sc = seed_push(handle)
    # the watermark fires slice 0 ahead of the main push: its "late" records are dropped in Phase P
    return [("push", sk, st, sc), ("wm", SIZE_MS - 1), ("push", k, ts, cols)], planted


T6 = NARROW[2]
NARROW_COUNTS = [1, 2, T6 - 1, T6, T6 + 1,                  # one block
                 GRID * T6 - 1, GRID * T6, GRID * T6 + 1,   # every block one tile; the last tile reloads itself
                 GRID * T6 + 100 * T6 + 3,                  # some blocks with a second tile, an odd tail
                 3 * GRID * T6 + 12345]                     # three or four tiles per block; the unpaired last record


@pytest.mark.parametrize("n", NARROW_COUNTS)
def test_narrow_tile_and_grid_edges(eng_mod, n):
    """COUNT + SUM(BIGINT), narrow entries: the kernel with the rolling order. Every count with the cold-branch
    records around its tile boundaries (counts of one tile at most have no boundary)."""
    steps, planted = main_steps(NARROW, n, seed=n)
    new = both_orders(eng_mod, NARROW, steps)
    assert new["narrow"] == 1                               # the wide records stayed under 1/64: still narrow entries
    if n > T6 + 1:
        assert all(c > 0 for c in planted.values()), planted
        # wide keys / values, the far timestamp, the slice without a slot (and the unpaired last record of an odd
        # push) take the v1 replay; the seed push's records too
        assert new["replay"] >= sum(planted[x] for x in ("wide_key", "wide_val", "far_ts", "no_slot"))
        assert new["late_total"] == planted["late"]


@pytest.mark.parametrize("n", [T6 + 1, GRID * T6 + 1, 3 * GRID * T6 + 12345])
def test_wide_entries_tile_and_grid_edges(eng_mod, n):
    """The same handle with 64-bit bucket entries (narrow entries off): the other paired-load kernel, which keeps the
    previous order under both settings of the switch (it shares the load code that was split into pairs). Wide keys
    and values are ordinary entries here."""
    steps, planted = main_steps(NARROW, n, seed=n + 1)
    new = both_orders(eng_mod, NARROW, steps, opts=dict(OPTS, narrow_entries=0))
    assert new["narrow"] == 0
    assert new["replay"] >= planted["far_ts"] + planted["no_slot"]
    assert new["late_total"] == planted["late"]


@pytest.mark.parametrize("which", ["keys", "ts", "value"])
def test_unaligned_column_takes_the_single_record_kernel(eng_mod, which):
    """A device column that is not 16-byte aligned (a tensor sliced by one element): the kernel with one record per
    load, which keeps the previous order under both settings of the switch."""
    import torch
    n = GRID * T6 + 7 * T6 + 5
    steps, _ = main_steps(NARROW, n, seed=77)

    def to_device(k, t, cols):
        def dev(x, shifted):
            off = int(shifted)
            buf = torch.empty(len(x) + 2, dtype=torch.from_numpy(x[:1]).dtype, device="cuda:0")
            buf[off:off + len(x)] = torch.from_numpy(x).to("cuda:0")
            v = buf[off:off + len(x)]
            assert (v.data_ptr() % 16 != 0) == (off == 1)
            return v
        return dev(k, which == "keys"), dev(t, which == "ts"), [dev(cols[0], which == "value")]
    both_orders(eng_mod, NARROW, steps, to_device=to_device)


@pytest.mark.parametrize("handle,tiles", [(NARROW2, 1), (NARROW2, 3), (COUNT_ONLY, 1), (COUNT_ONLY, 3)],
                         ids=["narrow2-1", "narrow2-3", "count-1", "count-3"])
def test_other_handles(eng_mod, handle, tiles):
    """C5's two value columns (DOUBLE beside FLOAT, tile 4096) and COUNT only (tile 8192), one and three tiles per
    block with an odd tail."""
    n = tiles * GRID * handle[2] + (0 if tiles == 1 else 4321)
    steps, _ = main_steps(handle, n, seed=tiles)
    both_orders(eng_mod, handle, steps)


@pytest.mark.parametrize("sync", [True, False], ids=["sync", "async"])
def test_three_pushes_with_watermarks(eng_mod, sync):
    """Three pushes with a watermark between them: stale slots and the speculative fire read the min_q / max_q that
    Phase P writes. Asynchronous pushes take device tensors."""
    import torch
    n = GRID * T6 + 50 * T6 + 1
    sk, st, sc = seed_push(NARROW, 6)
    steps = [("push", sk, st, sc)]
    for i in range(3):
        k, ts, cols = records(NARROW, n, seed=100 + i, lo_slice=i, hi_slice=i + 3)
        steps += [("push", k, ts, cols), ("wm", (i + 1) * SIZE_MS - 1)]

    def to_device(k, t, cols):
        return (torch.from_numpy(k).to("cuda:0"), torch.from_numpy(t).to("cuda:0"),
                [torch.from_numpy(c).to("cuda:0") for c in cols])
    both_orders(eng_mod, NARROW, steps, to_device=to_device, sync=sync)
