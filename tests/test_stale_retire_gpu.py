"""GPU tests: stale retirement. The tumbling fire releases the slots it retires without storing
their identities; the combiner of the next two-phase push overwrites a stale slot it reaches, and every other path
restores it first. Every case compares the rows of every watermark with the oracle, with the retirement on and off
(FWA_OPT_INGEST_VARIANT bit 9), through the lean and the general combiner body (bit 1), with synchronous calls and with
the asynchronous push / watermark pair the benchmark uses.

How a stream reaches a stale slot (1 s windows, pushes spanning at most two slices, so the lookahead stays at 4):
  seed   one record in slices 0 and 1: the slices 0 .. 5 exist from here on (this push replays: not two-phase);
  A0     a few records in slices 0 - 1 through the two-phase ingest, no watermark: a fire retires stale only behind a
         settled push that needed no replay, and the asynchronous watermark of A decides before A is settled;
  A      records in slices 0 - 1; watermark 999 fires window 0 and retires its slot S0;
  B      records in slices 1 - 2: its settle extends the lookahead to slice 6, which takes S0, still stale;
         watermark 1999 fires window 1 (slot S1 stale as well);
  C      the case's push, with records of slice 6: the first to land on S0.
Window 0 held every key, so whatever C leaves of it in S0 shows as a wrong or an extra row of window 6."""
import numpy as np
import pytest

from flink_amd import _abi as A
from helpers import assert_rows_equal
from key_place import mix64

pytestmark = pytest.mark.gpu

SUM2 = [("COUNT", 0), ("SUM_I64", 0)]
CMIN = [("COUNT", 0), ("MIN_I64", 0)]            # general combiner body, ~0 identities
IDENTITY_STORES = 512                            # FWA_OPT_INGEST_VARIANT bit 9
OLD_BODY = 2                                     # bit 1
NKEYS = 3000
I32 = 2**31


def batch(rng, keys, n, lo_ms, hi_ms, wm, sort=True):
    """n records (n even: an unpaired last record would take the replay) over keys, each key at least once."""
    assert n % 2 == 0 and n >= len(keys)
    k = rng.permutation(np.concatenate([keys, rng.choice(keys, n - len(keys))])).astype(np.int64)
    ts = rng.integers(lo_ms, hi_ms, n).astype(np.int64)
    if sort:
        ts.sort()
    return [k, ts, rng.integers(-I32, I32, n).astype(np.int64), wm, None]


def seed(key=1):
    return [np.full(2, key, np.int64), np.array([1, 1001], np.int64), np.ones(2, np.int64), -1, None]


def prefix(rng, keys, b=None):
    """seed, A0, A, B of the module docstring."""
    # (4000 records: a push is one Phase P tile then, and half a tile still fits one sub-bucket list of the two
    # partitions of the small table; a list that overflows sends its rest through the replay)
    return [seed(), batch(rng, keys[:1000], 2000, 0, 2000, -1), batch(rng, keys, 4000, 0, 2000, 999),
            b or batch(rng, keys, 4000, 1000, 3000, 1999)]


SNAP_AT = 3                                      # B's index: the state right behind its watermark


def stream(case):
    rng = np.random.default_rng(41)
    keys = np.arange(NKEYS, dtype=np.int64)
    sub = keys[::3]                               # a strict subset of window 0's keys
    if case == "reuse":
        return prefix(rng, keys) + [batch(rng, sub, 4000, 5000, 7000, 6999)]
    if case == "unreached":
        # C holds slice 5 only: slice 6 (on S0) is due at the watermark, but no record reached it: it must emit nothing
        # (a speculative fire lists it) and stay usable for the last push
        return prefix(rng, keys) + [batch(rng, sub, 4000, 5000, 6000, 6999), batch(rng, sub, 4000, 7000, 9000, 8999)]
    if case == "partition_hole":
        # C brings slice 6 the keys of one combiner block only (equal top 4 hash bits: one partition of up to 16); D
        # brings the other blocks' keys for slice 6: the read-modify-write merge on top of what C's blocks left there
        one = keys[(mix64(keys) >> np.uint64(60)) == 0]
        assert 50 < len(one) < NKEYS // 4
        c = batch(rng, sub, 4000, 5000, 6000, 4999)
        c6 = batch(rng, one, 2000, 6000, 7000, 4999)
        c = [np.concatenate([c[0], c6[0]]), np.concatenate([c[1], c6[1]]), np.concatenate([c[2], c6[2]]), 4999, None]
        return prefix(rng, keys) + [c, batch(rng, keys, 8000, 6000, 8000, 7999)]
    if case in ("stragglers", "stragglers_below"):
        # B spans slices 1 - 4 (lookahead 8: slices up to 12 exist, slice 6 on S0). C is two Phase P tiles of 6144
        # records in event-time order over the slices 6 - 9, the last third of the second tile back in slice 6: records
        # of the stale slice after its merge. _below: slice 6 only in that tail, which lies behind the first chunk of
        # every sub-bucket list (a tile gives a partition 768 entries or more, a chunk takes 384 at most), so every
        # block's window starts above slice 6 and never merges it.
        b = batch(rng, keys, 8000, 1000, 5000, 4999)
        c = batch(rng, sub, 2 * 6144, 6000 if case == "stragglers" else 7000, 10000, 9999)
        c[1][-2100:] = rng.integers(6000, 7000, 2100)
        return prefix(rng, keys, b) + [c]
    if case in ("replay", "replay_null"):
        # C carries, in slice 6, a key and a value that need 64 bits (narrow entries) or a NULL row (nullable column):
        # the v1 replay writes a slot the combiner has just overwritten; the other stale slots are reset ahead of it
        c = batch(rng, sub, 4000, 5000, 7000, 6999)
        c[1][-2:] = 6500
        if case == "replay":
            c[0][-1] += 2**40
            c[2][-2] += 2**40
        else:
            c[4] = np.zeros(4000, np.uint8)
            c[4][-2:] = 1
        return prefix(rng, keys) + [c, batch(rng, sub, 4000, 7000, 9000, 8999)]
    raise KeyError(case)


def config_kw(case, aggs, cap):
    kw = dict(window_kind="TUMBLE", size_ms=1_000, aggs=aggs, key_capacity=cap)
    if case == "replay_null":
        kw.update(semantics="TABLE", nullable_cols=(0,))
    return kw


_EXPECTED = {}


def expected(tag, kw, batches):
    """The oracle's rows per watermark (the last one Long.MAX_VALUE): once per stream and configuration."""
    if tag not in _EXPECTED:
        from oracle.oracle import Oracle
        o = Oracle(A.make_config(**kw))
        rows = []
        for k, t, v, wm, nul in batches:
            o.push(k, t, [v], nulls=None if nul is None else [nul])
            rows.append(o.advance_watermark(wm))
        rows.append(o.advance_watermark(A.LONG_MAX))
        o.close()
        _EXPECTED[tag] = rows
    return _EXPECTED[tag]


def options(variant):
    return {"ingest_variant": variant, "narrow_entries": 1, "skew_merge": 0, "window_passes": 0}


def run(kw, batches, mode, variant, snapshot_after=None):
    """Push the batches and advance the watermark after each; returns (rows per watermark, counters, snapshot blob).
    snapshot_after: index of the batch after whose watermark the state moves to a fresh handle."""
    import torch
    from flink_amd import engine
    cfg = A.make_config(output_on_device=1 if mode == "async" else 0, **kw)
    g = engine.WindowAggregator(cfg, options(variant))
    got, blob, stale = [], None, 0
    for b, (k, t, v, wm, nul) in enumerate(batches):
        if mode == "async":
            dev = [torch.from_numpy(x).cuda() for x in (k, t, v)]
            g.push(dev[0], dev[1], [dev[2]], sync=False, nulls=None if nul is None else [torch.from_numpy(nul).cuda()])
            g.advance_watermark_async(wm)
            got.append(g.fired_output())
        else:
            g.push(k, t, [v], nulls=None if nul is None else [nul])
            got.append(g.advance_watermark(wm))
        if b == snapshot_after:
            blob = g.snapshot()
            stale += g.get_option("stale_retires")
            g.close()
            g = engine.WindowAggregator(cfg, options(variant))
            g.restore(blob)
    got.append(g.advance_watermark(A.LONG_MAX))
    ctr = dict(stale=stale + g.get_option("stale_retires"), resets=g.get_option("reset_launches"),
               stragglers=g.get_option("stragglers"), replay=g.stats().replay_records)
    g.close()
    return got, ctr, blob


def check(case, aggs, cap, mode, variant, snapshot_after=None):
    kw = config_kw(case, aggs, cap)
    batches = stream(case)
    exp = expected((case, len(aggs), aggs[1][0], cap), kw, batches)
    got, ctr, blob = run(kw, batches, mode, variant, snapshot_after)
    names = A.agg_names(A.make_config(**kw))
    assert len(got) == len(exp)
    for b, (rg, ro) in enumerate(zip(got, exp)):
        assert_rows_equal(rg, ro, names, ctx="%s variant %d %s watermark %d" % (case, variant, mode, b))
    assert (ctr["stale"] > 0) == (not variant & IDENTITY_STORES), ctr
    return ctr, blob


def blob_in_entry_order(blob):
    """The snapshot's bytes with the entries of each key group sorted by (key, slice). A snapshot takes its entries
    from a fire whose blocks reserve their rows with one atomic each, so the order inside a key group changes from
    run to run of one handle; everything else in the blob is fixed."""
    from flink_amd import snapshot
    sn = snapshot.parse(blob)
    w = np.frombuffer(bytes(blob), dtype="<i8").copy()
    n, maxp = sn["n"], sn["max_parallelism"]
    lo = snapshot.HDR_WORDS + maxp + 1
    body = w[lo:lo + (w.size - lo) // max(n, 1) * n].reshape(-1, n) if n else w[lo:lo]
    if n:
        kg = np.repeat(np.arange(maxp), np.diff(sn["kg_offsets"]))
        body[:] = body[:, np.lexsort((body[1], body[0], kg))]
    return w.tobytes()


MODES = ["sync", "async"]
VARIANTS = [0, IDENTITY_STORES, OLD_BODY, OLD_BODY | IDENTITY_STORES]
# COUNT + SUM(long): the lean body and, with bit 1, the general one; COUNT + MIN: the general body whatever bit 1 says
WIDE = [(SUM2, 16384, v) for v in VARIANTS] + [(CMIN, 16384, v) for v in VARIANTS[:2]]
ALL = [(SUM2, 4096, v) for v in VARIANTS] + WIDE
ids = lambda combos: ["%s-%d-v%d" % (a[1][0], c, v) for a, c, v in combos]  # noqa: E731


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("aggs,cap,variant", ALL, ids=ids(ALL))
def test_reuse(aggs, cap, variant, mode):
    """Window 6 lands on window 0's slot with a third of its keys; nothing is reset by the separate kernel."""
    ctr, _ = check("reuse", aggs, cap, mode, variant)
    assert ctr["resets"] == 0, ctr


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ["unreached", "partition_hole"])
@pytest.mark.parametrize("aggs,cap,variant", WIDE, ids=ids(WIDE))
def test_slices_and_partitions_without_records(aggs, cap, case, variant, mode):
    check(case, aggs, cap, mode, variant)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ["stragglers", "stragglers_below"])
@pytest.mark.parametrize("aggs,cap,variant", WIDE, ids=ids(WIDE))
def test_stragglers_of_a_stale_slice(aggs, cap, case, variant, mode):
    ctr, _ = check(case, aggs, cap, mode, variant)
    assert ctr["stragglers"] > 0, ctr


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", ["replay", "replay_null"])
def test_replay_into_a_stale_slot(case, variant, mode):
    ctr, _ = check(case, SUM2, 4096, mode, variant)
    assert ctr["replay"] >= 2, ctr


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("aggs,cap,body", [(SUM2, 16384, 0), (SUM2, 16384, OLD_BODY), (CMIN, 16384, 0)],
                         ids=["sum-lean", "sum-general", "min"])
def test_snapshot_between_retirement_and_next_push(aggs, cap, body, mode):
    """After B's watermark S0 is stale under slice 6 and S1 stale and free: the state moves to a fresh handle there. The
    rows go on to equal the oracle's, and the blob is, byte for byte once its entries are put in one order, the one
    a handle that stores the identities writes."""
    _, stale_blob = check("reuse", aggs, cap, mode, body, snapshot_after=SNAP_AT)
    _, clean_blob = check("reuse", aggs, cap, mode, body | IDENTITY_STORES, snapshot_after=SNAP_AT)
    assert len(stale_blob) == len(clean_blob) > 8 * 200
    assert blob_in_entry_order(stale_blob) == blob_in_entry_order(clean_blob)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kw", [dict(window_kind="TUMBLE", semantics="DATASTREAM", allowed_lateness_ms=2_000),
                                dict(window_kind="HOP", slide_ms=500)], ids=["lateness", "hop"])
def test_not_eligible(kw, mode):
    """Allowed lateness keeps fired slots, a HOP window spans slices: both retire with identity stores as before."""
    kw = dict(size_ms=1_000, aggs=SUM2, key_capacity=4096, **kw)
    batches = stream("reuse")
    exp = expected(("reuse", kw["window_kind"], kw.get("allowed_lateness_ms")), kw, batches)
    got, ctr, _ = run(kw, batches, mode, 0)
    names = A.agg_names(A.make_config(**kw))
    for b, (rg, ro) in enumerate(zip(got, exp)):
        assert_rows_equal(rg, ro, names, ctx="%s watermark %d" % (kw["window_kind"], b))
    assert ctr["stale"] == 0, ctr
