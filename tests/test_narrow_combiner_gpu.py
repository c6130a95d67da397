"""The narrow combiner's lean body (combine3, DESIGN.md §5 "Lean narrow combiner": 4-byte key image in LDS, first probes
in batches, misses deferred to one pass per chunk, wave-uniform adds) against the oracle and against the general body
on the same build (FWA_OPT_INGEST_VARIANT bit 1). Every case runs both bodies; rows are bit-exact with the oracle, and
late drops, replayed records and stragglers agree between the bodies.

The key sets are built on the CPU with the engine's own hash (mix64: the top bits pick the key table segment = combiner
block, the low bits the 8-slot home bucket), so a case can aim keys at one bucket, one segment or one sub-bucket list.
A push reaches the combiner only for slices that exist, so every case first pushes one record per slice."""
import functools

import numpy as np
import pytest

from flink_amd import _abi as A
from helpers import assert_rows_equal
from key_place import mix64

pytestmark = pytest.mark.gpu

AGGS = [("COUNT", 0), ("SUM_I64", 0)]
CAP = 1 << 15                     # key_capacity: a 2^16-slot table = 16 segments of 4096 slots (one combiner block each)
SEG_LOG, PART_BITS, BUCKET = 12, 4, 8
IT = 6                            # entries per lane and chunk of the narrow combiner (both bodies)
TILE = 6 * 1024                   # records per partition3 tile; tile t of a push feeds sub-bucket t % 16
OLD_BODY = 2                      # FWA_OPT_INGEST_VARIANT bit 1
I32_MIN, I32_MAX = -2**31, 2**31 - 1


def seg_of(keys):
    return (mix64(keys) >> np.uint64(64 - PART_BITS)).astype(np.int64)


def bucket_of(keys):
    return ((mix64(keys) & np.uint64((1 << SEG_LOG) - 1)) >> np.uint64(3)).astype(np.int64)


def place(keys):
    """(segment, home bucket) as one number."""
    return seg_of(keys) * (1 << (SEG_LOG - 3)) + bucket_of(keys)


def groups_by_place(cand, size, count, rng):
    """`count` sets of `size` keys of cand that share one (segment, home bucket) each."""
    pl = place(cand)
    order = np.argsort(pl, kind="stable")
    spl, sk = pl[order], cand[order]
    starts = np.flatnonzero(np.r_[True, spl[1:] != spl[:-1]])
    lens = np.diff(np.r_[starts, len(spl)])
    ok = starts[lens >= size]
    assert len(ok) >= count, "candidate pool too small"
    pick = rng.choice(ok, count, replace=False)
    return [sk[s:s + size].copy() for s in pick]


@functools.lru_cache(maxsize=None)
def narrow_pool():
    return np.random.default_rng(11).permutation(np.arange(-(1 << 20), 1 << 20, dtype=np.int64))


def probe_distance_buckets(keys):
    """Linear probing of `keys` into an empty segment, as key_slot does (home = the bucket's first slot): the largest
    distance, in buckets, between a key's slot and its home bucket. All keys must be of one segment."""
    seg = 1 << SEG_LOG
    tab = np.zeros(seg, bool)
    worst = 0
    for b in bucket_of(keys):
        s = int(b) * BUCKET
        d = 0
        while tab[(s + d) % seg]:
            d += 1
        tab[(s + d) % seg] = True
        worst = max(worst, d // BUCKET)
    return worst


@pytest.fixture(scope="module")
def eng_mod():
    from flink_amd import engine
    engine.lib()
    return engine


def seed_push(slices, key, size_ms=1000):
    """One record per slice, so the slices exist when the next push is partitioned (these records take the v1 path)."""
    ts = np.arange(slices, dtype=np.int64) * size_ms + 1
    return np.full(slices, key, np.int64), ts, np.ones(slices, np.int64)


def run_gpu(eng_mod, pushes, variant, cap=CAP, size_ms=1000, after=None):
    """Push every (keys, ts, vals) through a fresh handle; returns what the bodies are compared on, the rows fired at
    the end among it. The first failing push ends the run: {"error": (push index, status)}. after(handle, stats):
    more steps on the handle before the rows are fired; it may return a replacement handle."""
    cfg = A.make_config(window_kind="TUMBLE", size_ms=size_ms, aggs=AGGS, key_capacity=cap)
    g = eng_mod.WindowAggregator(cfg, options={"ingest_variant": variant, "narrow_entries": 1, "skew_merge": 0,
                                               "window_passes": 0})
    res = {"late": []}
    try:
        for i, (k, t, v) in enumerate(pushes):
            try:
                res["late"].append(g.push(k, t, [v]))
            except eng_mod.EngineError as err:
                res["error"] = (i, err.code)
                return res
        assert g.get_option("narrow_entries") == 1 and g.get_option("window_passes") == 0
        st = g.stats()
        assert st.partition_ms > 0, "the two-phase ingest did not run"
        res.update(replay=st.replay_records, stragglers=g.get_option("stragglers"),
                   digest=g.get_option("key_table_digest"))
        if after is not None:
            g = after(g, res) or g
        res["rows"] = g.advance_watermark(A.LONG_MAX)
        res["late_total"] = g.stats().late_dropped
        return res
    finally:
        g.close()


def both_bodies(eng_mod, pushes, cap=CAP, size_ms=1000, same_replay=True, more=()):
    """The oracle once, then the lean and the general body: rows equal the oracle's, the bodies agree on the rest.
    more: pushes made after a snapshot / restore into a fresh handle (both bodies, the oracle just goes on)."""
    from oracle.oracle import Oracle
    cfg = A.make_config(window_kind="TUMBLE", size_ms=size_ms, aggs=AGGS, key_capacity=cap)
    names = A.agg_names(cfg)
    o = Oracle(cfg)
    late = [o.push(k, t, [v]) for k, t, v in list(pushes) + list(more)]
    want = o.advance_watermark(A.LONG_MAX)
    o.close()
    out = []
    for variant in (0, OLD_BODY):
        def after(g, res, variant=variant):
            if not more:
                return None
            blob = g.snapshot()
            g.close()
            h = eng_mod.WindowAggregator(cfg, options={"ingest_variant": variant, "narrow_entries": 1,
                                                       "skew_merge": 0, "window_passes": 0})
            h.restore(blob)
            for k, t, v in more:
                res["late"].append(h.push(k, t, [v]))
            assert h.stats().partition_ms > 0
            return h
        r = run_gpu(eng_mod, pushes, variant, cap, size_ms, after)
        assert "error" not in r, r
        assert r["late"] == late, "variant %d late drops per push" % variant
        assert_rows_equal(r["rows"], want, names, ctx="variant %d" % variant)
        out.append(r)
    new, old = out
    assert new["late_total"] == old["late_total"]
    assert new["stragglers"] == old["stragglers"]
    if same_replay:
        assert new["replay"] == old["replay"]
    return new, old


def records(rng, keys, n, slices=2, size_ms=1000, sort=True):
    """n records over `keys` (each at least once when n allows), values over the signed 32-bit range, timestamps
    ascending over `slices` slices."""
    k = np.concatenate([keys, rng.choice(keys, n - len(keys))]) if n >= len(keys) else rng.choice(keys, n)
    k = rng.permutation(k).astype(np.int64)
    ts = rng.integers(0, slices * size_ms, n).astype(np.int64)
    if sort:
        ts.sort()
    vals = rng.integers(I32_MIN, 1 << 31, n).astype(np.int64)
    return k, ts, vals


def test_built_displacement_chains(eng_mod):
    """Sets of 40 keys with one home bucket each (8 slots): most of a set lives 2 to 4 buckets from home, and keys of
    the buckets behind it are pushed on in turn. One push inserts them all (misses through the deferred pass, next
    buckets, CAS), a second finds them again through the same probes."""
    rng = np.random.default_rng(1)
    sets = groups_by_place(narrow_pool()[:1 << 20], 40, 24, rng)
    for s in sets:
        assert len(set(place(s))) == 1 and len(np.unique(s)) == 40
    assert min(probe_distance_buckets(s) for s in sets) >= 2          # checked before any GPU call
    assert max(probe_distance_buckets(s) for s in sets) <= 5
    chain = np.concatenate(sets)
    filler = narrow_pool()[(1 << 20):(1 << 20) + 12_000]
    keys = np.concatenate([chain, filler])
    n = (1 << 16) + 1
    p1 = records(rng, keys, n)
    p2 = records(rng, keys, n)
    p2 = (p2[0], p2[1] + 1000, p2[2])                                 # slices 1 and 2: the window slides too
    new, _ = both_bodies(eng_mod, [seed_push(3, int(filler[0])), p1, p2])
    assert new["replay"] < n // 8


@pytest.mark.parametrize("case", ["same_key_many_lanes", "distinct_keys_one_slot", "segment_to_last_slot"])
def test_insert_races(eng_mod, case):
    """Every key of the main push is new. same_key_many_lanes: 48 keys over 2^16 records, so most lanes of a chunk
    carry a key another lane inserts at that moment (CAS returns the lane's own key). distinct_keys_one_slot: sets of
    24 keys per home bucket, so lanes with different keys compete for one empty slot (the loser re-reads the bucket).
    segment_to_last_slot: one segment receives exactly its 4096th key in this push; none is refused."""
    rng = np.random.default_rng(2)
    pool = narrow_pool()
    n = 1 << 16
    if case == "same_key_many_lanes":
        keys = pool[:48]
    elif case == "distinct_keys_one_slot":
        keys = np.concatenate(groups_by_place(pool[:1 << 20], 24, 64, rng))
    else:
        cand = pool[:1 << 18]
        in_seg = cand[seg_of(cand) == 5]
        assert len(in_seg) >= 4096
        others = cand[seg_of(cand) != 5][:3000]
        keys = np.concatenate([in_seg[:4096], others])
    main = records(rng, keys, n)
    if case == "segment_to_last_slot":                                # three records per key of the segment: its
        k = rng.choice(others, n)                                     # sub-bucket lists must not overflow
        k[rng.choice(n, 3 * 4096, replace=False)] = np.tile(in_seg[:4096], 3)
        main = (k.astype(np.int64), main[1], main[2])
    new, _ = both_bodies(eng_mod, [seed_push(2, int(keys[0])), main])
    assert new["replay"] < n // 8                                     # the combiner, not the replay, took the push


def test_table_full_raises_where_the_general_body_does(eng_mod):
    """A segment holds 4096 keys; a push that brings its 4097th and more fails with FWA_E_OOM, with both bodies at the
    same push, after pushes that filled the segment without error."""
    rng = np.random.default_rng(3)
    cand = narrow_pool()[:1 << 18]
    in_seg = cand[seg_of(cand) == 9]
    assert len(in_seg) >= 4200
    others = cand[seg_of(cand) != 9][:2000]
    fill = records(rng, np.concatenate([in_seg[:4000], others]), 1 << 16)
    last = records(rng, np.concatenate([in_seg[4000:4096], others]), 1 << 16)
    over = records(rng, np.concatenate([in_seg[4096:4200], others]), 1 << 16)
    pushes = [seed_push(2, int(others[0])), fill, last, over]
    got = [run_gpu(eng_mod, pushes, v) for v in (0, OLD_BODY)]
    assert got[0].get("error") == (3, -5), got[0]                      # FWA_E_OOM at the push past the capacity
    assert got[1].get("error") == got[0]["error"]
    assert got[0]["late"] == got[1]["late"]


def test_foreign_residents(eng_mod):
    """64-bit keys in the buckets narrow keys probe: they reach the table through the v1 replay (under 1/64 of the
    records, so the handle stays narrow) and are held in the 4-byte image as occupied and foreign. The narrow keys
    pushed afterwards probe past them, are inserted behind them, and the wide keys' slots are not rewritten."""
    rng = np.random.default_rng(4)
    wide_cand = (np.int64(1) << 40) + np.arange(1 << 21, dtype=np.int64) * 3 + 1
    wide_cand[::2] = -wide_cand[::2]
    low = wide_cand.astype(np.int32).astype(np.int64)                  # their low words, narrow keys of their own
    narrow_cand = np.setdiff1d(narrow_pool()[:1 << 20], low)
    wsets = groups_by_place(wide_cand, 12, 16, rng)
    by_place = {int(place(s[:1])[0]): s for s in wsets}
    npl = place(narrow_cand)
    nsets = []
    for pl in by_place:
        m = narrow_cand[npl == pl]
        assert len(m) >= 12
        nsets.append(m[:12])
    wide = np.concatenate(wsets)
    narrow = np.concatenate(nsets)
    filler = narrow_cand[-9000:]
    n = 1 << 16
    k1, t1, v1 = records(rng, filler, n)
    at = rng.choice(n, 5 * len(wide), replace=False)                   # 960 wide records: under n / 64
    assert len(at) * 64 < n
    k1[at] = np.tile(wide, 5)
    k2, t2, v2 = records(rng, np.concatenate([narrow, filler, low[:64]]), n)
    k3, t3, v3 = records(rng, np.concatenate([narrow, filler]), n)
    at = rng.choice(n, 2 * len(wide), replace=False)
    k3[at] = np.tile(wide, 2)                                          # the wide keys again: still found
    both_bodies(eng_mod, [seed_push(2, int(filler[0])), (k1, t1, v1), (k2, t2, v2), (k3, t3, v3)])


def test_edge_keys_in_one_push(eng_mod):
    """The ends of the narrow key range next to the two marker values in one push: INT32_MAX, -1, 0 and INT32_MIN + 2
    are combiner entries; INT32_MIN and INT32_MIN + 1 (the image's empty and foreign marks) take the v1 replay."""
    rng = np.random.default_rng(5)
    n = (1 << 16) + 3
    filler = narrow_pool()[:8000]
    k, t, v = records(rng, filler, n)
    edge = np.array([I32_MAX, -1, 0, I32_MIN + 2], np.int64)
    marks = np.array([I32_MIN, I32_MIN + 1], np.int64)
    at = rng.choice(n, 4000 + 800, replace=False)
    k[at[:4000]] = np.tile(edge, 1000)
    k[at[4000:]] = np.tile(marks, 400)                                 # 800 records: under n / 64
    k2, t2, v2 = records(rng, np.concatenate([filler, edge, marks]), n)
    new, _ = both_bodies(eng_mod, [seed_push(2, 7), (k, t, v), (k2, t2 + 1000, v2)])
    assert new["replay"] >= 800 + 2


def test_chunk_edges_per_sub_bucket(eng_mod):
    """Sub-bucket lists of one partition with 1, 2, 63, 64, 65, 64 * IT - 1, 64 * IT and 64 * IT + 1 entries (whole
    chunks, chunks with one lane, one lane short), others empty, in a push with an odd record count: tile t of a push
    feeds sub-bucket t % 16, so each tile holds exactly that many records of the partition."""
    rng = np.random.default_rng(6)
    cand = narrow_pool()[:1 << 17]
    mine = cand[seg_of(cand) == 3][:600]
    rest = cand[seg_of(cand) != 3][:20_000]
    counts = [1, 2, 63, 64, 65, 64 * IT - 1, 64 * IT, 64 * IT + 1, 0, 129, 7]
    n = len(counts) * TILE - 1001                                      # 11 tiles, the last one short; odd
    assert n % 2 == 1
    k, t, v = records(rng, rest, n)
    for tile, c in enumerate(counts):
        lo, hi = tile * TILE, min((tile + 1) * TILE, n)
        at = lo + rng.choice(hi - lo, c, replace=False)
        k[at] = rng.choice(mine, c)
    assert [int((seg_of(k[i * TILE:(i + 1) * TILE]) == 3).sum()) for i in range(len(counts))] == counts
    both_bodies(eng_mod, [seed_push(2, int(rest[0])), (k, t, v)])


def test_window_slides_and_straggler_overflow(eng_mod):
    """One push over 6 slices in event-time order, its last tenth back in the first slice: every combiner block has
    slid its 2-slice window past that slice by then, so those entries straggle, far more than the 256 a block lists
    in LDS (the rest goes to the slots with device atomics at once). Both bodies count the same stragglers: the push
    has 16 tiles, one per sub-bucket, so the order of a sub-bucket's list, and with it which entries straggle, does
    not depend on how two Phase P blocks interleave their appends."""
    rng = np.random.default_rng(7)
    n = 16 * TILE - 1
    keys = narrow_pool()[:20_000]
    k, t, v = records(rng, keys, n, slices=6)
    tail = n // 10
    t[-tail:] = rng.integers(0, 1000, tail)
    new, _ = both_bodies(eng_mod, [seed_push(6, int(keys[0])), (k, t, v)])
    assert new["stragglers"] > 256 * 16                               # more than 256 in at least one of the 16 blocks


def test_published_keys_snapshot_restore(eng_mod):
    """Keys inserted by the lean body are published sign-extended into the 64-bit table: the table equals, word for
    word, the one the general body leaves (FWA_OPT_KEY_TABLE_DIGEST), and a snapshot restored into a fresh handle goes
    on to equal the oracle. The stream makes the placement independent of the order lanes insert in: every push
    brings at most one new key per home bucket, four pushes in all, so no bucket fills and a key's slot is the number
    of keys its bucket held before."""
    rng = np.random.default_rng(8)
    cand = narrow_pool()[:1 << 19]
    pl = place(cand)
    order = np.argsort(pl, kind="stable")
    spl, sk = pl[order], cand[order]
    starts = np.flatnonzero(np.r_[True, spl[1:] != spl[:-1]])
    lens = np.diff(np.r_[starts, len(spl)])
    starts = starts[lens >= 4][:5000]
    waves = [sk[starts + j] for j in range(4)]                         # wave j: the j-th key of 5000 buckets
    for w in waves:
        assert len(set(place(w))) == len(w)
    n = (1 << 16) + 1
    pushes = [seed_push(5, int(waves[0][0]))]
    for j, w in enumerate(waves):
        known = np.concatenate(waves[:j]) if j else w[:0]
        k, t, v = records(rng, np.concatenate([w, known]), n)
        pushes.append((k, t + 1000 * j, v))
    later = records(rng, np.concatenate(waves + [cand[-3000:]]), n)
    later = (later[0], later[1] + 3000, later[2])
    new, old = both_bodies(eng_mod, pushes, more=[later])
    assert new["digest"] == old["digest"]
