"""The key axis: 64-bit key sets aimed at chosen places of the key table (tests/key_place.py), through every path that
probes it. The probe order of key_slot (ingest.inc) is written out again in key_find, the combiner's general body, the
sessions' s5 resolve, key_probe8 / key_probe8_find (sessions, reductions), the fires' presence test and the restore;
two copies that disagree store a key twice or lose a displaced key's records, and only for keys that probing displaced.
Random keys in a table at load 0.5 are displaced by a bucket at most and wrap a segment by luck; these sets are built
per handle from its reported shape (FWA_OPT_KEY_TABLE_SHAPE), and every property a set is named for is asserted on
the CPU model before the first GPU call.

The reference is the oracle, which knows nothing of tables. Rows are exact: integer aggregates, MIN / MAX, and double
sums over integer-valued doubles below 2^20. stats().live_keys (keys ever inserted) must equal the number of distinct
keys pushed: a key stored twice shows there even where its rows would add up."""
import ctypes
import functools

import numpy as np
import pytest

import key_place as K
from flink_amd import _abi as A
from helpers import assert_rows_equal

pytestmark = pytest.mark.gpu

SETS = ["chain", "wrap", "dense", "race", "edge"]
PER_KEY = {"chain": 40, "wrap": 28, "dense": 12, "race": 20, "edge": 60}      # records per key and push
I32 = 1 << 31


@pytest.fixture(scope="module")
def eng_mod():
    from flink_amd import engine
    engine.lib()
    return engine


# ---- which keys a handle owns (key-group ranges), and the hashes of a PREHASHED handle ---------------------------------
def hash_of(keys):
    """A caller-supplied key.hashCode() per id, unrelated to the id's place in the table."""
    k = np.asarray(keys, np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        h = (k * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(29)
    return (h & np.uint64(0xffffffff)).astype(np.uint32).view(np.int32)


def key_group(key, key_kind, max_par=128):
    from oracle import oracle
    return oracle.lib().or_key_group(ctypes.c_int64(int(key)), key_kind, int(hash_of([key])[0]), max_par)


def owned(key_kind, lo, hi):
    return lambda k: lo <= key_group(k, key_kind) <= hi


# ---- the paths ---------------------------------------------------------------------------------------------------------
# cols: the value columns' types; comb: the two-phase ingest must have run (slices are seeded first, partition_ms > 0)
V2_OFF = {"skew_merge": 0, "window_passes": 0, "narrow_entries": 0}
AGGS_NW2 = [("COUNT", 0), ("SUM_F64", 1), ("AVG_F64", 1), ("MAX_F32", 0), ("MAX_F64", 1), ("MIN_F32", 0)]
AGGS_SESS = [("COUNT", 0), ("SUM_I64", 0), ("MAX_I64", 0)]


def tumble(aggs, cols, comb=True, options=None, cap=1 << 13, **kw):
    return dict(cfg=dict(window_kind="TUMBLE", size_ms=1000, aggs=aggs, key_capacity=cap, **kw), cols=cols, comb=comb,
                options=dict(V2_OFF, **(options or {})))


def session(sem, gap, options=None, path=None, aggs=AGGS_SESS, cols=("i64",), cap=1 << 13, **kw):
    return dict(cfg=dict(window_kind="SESSION", semantics=sem, gap_ms=gap, size_ms=0, aggs=aggs, key_capacity=cap, **kw),
                cols=cols, comb=False, options=options or {}, session=gap, path=path)


def reduce_list(op, pos):
    from flink_amd.operators import reduction_aggs
    return reduction_aggs(op, pos, ("I32", "F64", "I64"))


PATHS = {
    # (a) the one-pass ingest: a handle the two-phase plan refuses (three value columns)
    "v1_three_columns": tumble([("COUNT", 0), ("SUM_I64", 0), ("MAX_I64", 1), ("MIN_I64", 2)], ("i64",) * 3, comb=False),
    "v1_unaligned_device_columns": dict(tumble([("COUNT", 0), ("SUM_I64", 0), ("MAX_I64", 1), ("MIN_I64", 2)],
                                               ("i64",) * 3, comb=False), unaligned=True),
    # (b) combine3's general body
    "comb_layout0_nv1": tumble([("COUNT", 0), ("MAX_I64", 0)], ("i64",)),
    "comb_layout0_nv2": tumble([("COUNT", 0), ("SUM_I64", 0), ("MAX_I64", 1)], ("i64", "i64")),
    "comb_layout2_count": tumble([("COUNT", 0)], ()),
    "comb_layout1_wide_entries": tumble([("COUNT", 0), ("SUM_I64", 0)], ("i64",)),
    "comb_nw2_float_double": dict(tumble(AGGS_NW2, ("f32", "f64"), options={"narrow_entries": 1}, semantics="TABLE"),
                                  narrow=True),
    "comb_skew_merge": tumble([("COUNT", 0), ("SUM_I64", 0)], ("i64",), options={"skew_merge": 1}),
    "comb_window_passes": tumble([("COUNT", 0), ("SUM_I64", 0)], ("i64",), options={"window_passes": 1}),
    "comb_owned_key_groups": dict(tumble([("COUNT", 0), ("MAX_I64", 0)], ("i64",), kg_start=0, kg_end=63),
                                  keep=(A.KEY_JAVA_LONG, 0, 63)),
    "comb_prehashed": dict(tumble([("COUNT", 0), ("MAX_I64", 0)], ("i64",), kg_start=64, kg_end=127,
                                  key_kind=A.KEY_PREHASHED), keep=(A.KEY_PREHASHED, 64, 127), hashed=True),
    "comb_wide_list_small_segments": dict(tumble([("COUNT", 0), ("SUM_I64", 0), ("MIN_I64", 0), ("MAX_I64", 1),
                                                  ("SUM_F64", 1)], ("i64", "f64")), small_segments=True),
    "comb_unaligned_device_columns": dict(tumble([("COUNT", 0), ("MAX_I64", 0)], ("i64",)), unaligned=True),
    # (d) reductions (key_probe8_find, key_slot as fallback)
    "reduce_tumble_min_by": tumble(None, ("i32", "f64", "i64"), comb=False, reduce=True),
    "reduce_tumble_sum": tumble(None, ("i32", "f64", "i64"), comb=False, reduce=True),
    "reduce_session_min_by": session("DATASTREAM", 1000, aggs=[("MINBY_I64", 2)], cols=("i32", "f64", "i64"), reduce=True),
    "reduce_session_sum": session("DATASTREAM", 1000, aggs=[("SUM_I64", 2)], cols=("i32", "f64", "i64"), reduce=True),
}
# (c) sessions: the general path, the sorted-cell path, the cell pre-aggregation by both routes; both semantics
for _sem in ("DATASTREAM", "TABLE"):
    _s = _sem.lower()
    PATHS["session_general_" + _s] = session(_sem, 1000, options={"session_cells": 0}, path=0)
    PATHS["session_sorted_cells_" + _s] = session(_sem, 100, path=1)
    PATHS["session_preagg_s5_" + _s] = session(_sem, 1000, path=2)
    PATHS["session_preagg_s4_" + _s] = session(_sem, 1000, options={"ingest_variant": 8}, path=2)


def make_cfg(name, **over):
    kw = dict(PATHS[name]["cfg"], **over)
    if kw["aggs"] is None:
        kw["aggs"] = reduce_list("min_by" if "min_by" in name else "sum", 3)
    return A.make_config(**kw)


def open_pair(eng_mod, name, **over):
    """(handle, oracle, names, shape) of a path."""
    from oracle.oracle import Oracle
    cfg = make_cfg(name, **over)
    g = eng_mod.WindowAggregator(cfg, options=PATHS[name]["options"])
    return g, Oracle(make_cfg(name, **over)), A.agg_names(cfg), K.shape_of(g.get_option("key_table_shape"))


# ---- the sets, per shape: (keys of the first push, all keys), checked on the CPU model ------------------------------
def build_set(shape, name, narrow=False, keep=None):
    rng = np.random.default_rng([SETS.index(name), shape[0], shape[1], int(narrow)])
    kw = dict(wide=not narrow, keep=keep)
    if name == "chain":
        keys = K.chain_set(shape, rng, **kw)
        K.check_chain(shape, keys)
        return [keys]
    if name == "wrap":
        groups, segs = [], K.wrap_segments(shape)
        for segment in segs:
            main, own, other = K.wrap_set(shape, rng, segment, **kw)
            K.check_wrap(shape, main, own, other)
            K.check_wrap(shape, main, own, other, order=np.r_[own, other, main])
            groups += [main, own, other]
        t, _ = K.place_all(shape, np.concatenate(groups))                # together: still inside their segments
        assert t.wrapped and t.n_keys == sum(len(g) for g in groups)
        return groups
    if name == "dense":
        keys = K.dense_set(shape, rng, **kw)
        K.check_dense(shape, keys)
        return [keys]
    if name == "race":
        same, many = K.race_set(shape, rng, **kw)
        K.check_race(shape, same, many)
        return [same, many]
    ends, fam = K.edge_set()
    if narrow:                                                           # the ends of the 32-bit range instead
        ends, fam = np.array([0, 1, -1, I32 - 1, -I32, -I32 + 1, -I32 + 2], np.int64), ends[:0]
    allk = np.r_[ends, fam]
    if keep is not None:
        allk = np.array([k for k in allk.tolist() if keep(k)], np.int64)
        assert len(allk) >= 8
    t, slots = K.place_all(shape, allk)
    assert len(set(slots)) == len(allk) == t.n_keys                      # distinct keys, distinct slots
    return [allk]


@functools.lru_cache(maxsize=None)
def cached_set(shape, name, narrow, keep_spec):
    return build_set(shape, name, narrow, owned(*keep_spec) if keep_spec else None)


def columns(types, rng, n):
    """Value columns with exact aggregates in any order: integers over the signed 32-bit range, integer-valued floats
    and doubles below 2^20."""
    out = []
    for t in types:
        if t == "i64":
            out.append(rng.integers(-I32, I32, n).astype(np.int64))
        elif t == "i32":
            out.append(rng.integers(-1000, 1000, n).astype(np.int32))
        elif t == "f64":
            out.append(rng.integers(-(1 << 20) + 1, 1 << 20, n).astype(np.float64))
        else:
            out.append(rng.integers(-(1 << 20) + 1, 1 << 20, n).astype(np.float32))
    return out


def records(rng, keys, per_key, head=None):
    """Every key per_key times in random order, behind `head` (a block of one key)."""
    k = rng.permutation(np.repeat(np.asarray(keys, np.int64), per_key))
    return k if head is None else np.r_[head, k]


def stamps(spec, rng, n, phase):
    """Event times of a push. TUMBLE (1 s): slices 0-1, then 1-2, ascending. SESSION: a push is order-free (its windows
    end behind the watermark before it) and spans 3.5 s: 4 cells at a 1 s gap, 35 at 100 ms."""
    if spec.get("session"):
        t0 = 8000 * phase
        return np.where(rng.random(n) < 0.5, rng.integers(t0, t0 + 500, n), rng.integers(t0 + 3000, t0 + 3500, n)).astype(np.int64)
    return np.sort(rng.integers(1000 * phase, 1000 * phase + 2000, n)).astype(np.int64)


def watermark(spec, phase):
    return 8000 * phase + 2000 if spec.get("session") else 1000 * phase + 999


class Run:
    """A handle and the oracle in step: pushes with equal late drops, fires with equal rows."""

    def __init__(self, eng_mod, name, **over):
        self.spec, self.name = PATHS[name], name
        self.g, self.o, self.names, self.shape = open_pair(eng_mod, name, **over)
        self.keys, self.n, self.marks = set(), 0, 0

    def push(self, k, ts, cols):
        import torch
        kh = hash_of(k) if self.spec.get("hashed") else None
        late_o = self.o.push(k, ts, cols, key_hash=kh)
        if self.spec.get("unaligned"):                                   # device columns 8 bytes off a 16-byte border
            def dev(x):
                d = torch.empty(len(x) + 2, dtype=torch.int64, device="cuda")
                d[1:1 + len(x)].copy_(torch.from_numpy(np.ascontiguousarray(x, np.int64)))
                return d[1:1 + len(x)]
            cols_d = [dev(c) for c in cols]
            assert all(c.data_ptr() % 16 == 8 for c in cols_d)
            kd, td = torch.from_numpy(np.ascontiguousarray(k)).cuda(), torch.from_numpy(np.ascontiguousarray(ts)).cuda()
            late_g = self.g.push(kd, td, cols_d)
        else:
            late_g = self.g.push(k, ts, cols, key_hash=kh)
        assert late_g == late_o, "%s: late drops %d, oracle %d" % (self.name, late_g, late_o)
        self.keys.update(np.asarray(k).tolist())
        self.n += len(k)
        if self.spec.get("narrow"):          # the 4-byte key image's empty and foreign marks take the one-pass replay
            self.marks += int(np.isin(k, [-I32, -I32 + 1]).sum())
        if self.spec.get("path") is not None:
            assert self.g.get_option("session_path") == self.spec["path"], self.name

    def seed(self, key, slices=4):
        """One record per slice, so the slices exist when the next pushes are partitioned (these take the v1 path)."""
        rng = np.random.default_rng(7)
        self.push(np.full(slices, key, np.int64), np.arange(slices, dtype=np.int64) * 1000 + 1,
                  columns(self.spec["cols"], rng, slices))
        self.n -= slices

    def fire(self, wm, ctx=""):
        assert_rows_equal(self.g.advance_watermark(wm), self.o.advance_watermark(wm), self.names,
                          ctx="%s %s wm=%d" % (self.name, ctx, wm))

    def check_live_keys(self):
        assert self.g.stats().live_keys == len(self.keys), "%s: %d keys in the table, %d distinct keys pushed" % (
            self.name, self.g.stats().live_keys, len(self.keys))

    def check_combiner(self):
        if self.spec["comb"]:
            st = self.g.stats()
            assert st.partition_ms > 0, "the two-phase ingest did not run"
            assert st.replay_records - self.marks < max(64, self.n // 8), "%d of %d records replayed" % (
                st.replay_records, self.n)
            for opt in ("skew_merge", "window_passes", "narrow_entries"):
                assert self.g.get_option(opt) == self.spec["options"][opt], opt

    def close(self):
        self.g.close()
        self.o.close()


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("path", list(PATHS))
def test_aimed_keys(eng_mod, path, which):
    """Each set twice: the first push inserts, the second, behind a watermark that fires some windows, finds the keys
    again and adds to them. The race set's first push brings one new key in every lane of a tile and 24 new keys of one
    home bucket at once."""
    spec = PATHS[path]
    r = Run(eng_mod, path)
    try:
        if spec.get("small_segments"):
            assert r.shape[0] < 12, r.shape
        groups = cached_set(r.shape, which, bool(spec.get("narrow")), spec.get("keep"))       # CPU checks run here
        keys = np.concatenate(groups)
        rng = np.random.default_rng(3)
        if spec["comb"]:
            r.seed(int(keys[-1]))
        # (a push's records of one partition and one Phase P tile share a sub-bucket list of a little over 2048 entries:
        # more would overflow into the one-pass replay instead of reaching the combiner)
        head = np.full(1400, groups[0][0], np.int64) if which == "race" else None
        for phase in (0, 1):
            k = records(rng, keys, PER_KEY[which], head)
            r.push(k, stamps(spec, rng, len(k), phase), columns(spec["cols"], rng, len(k)))
            if phase == 0:
                r.check_live_keys()
                r.fire(watermark(spec, phase), which)
        r.check_live_keys()
        r.check_combiner()
        r.fire(A.LONG_MAX, which)
    finally:
        r.close()


def test_shape_option_is_read_only_and_needs_a_key_table(eng_mod):
    """FWA_OPT_KEY_TABLE_SHAPE: seg_log | part_bits << 8 of the table the handle allocated (2 * key_capacity slots and
    up), refused by fwa_set_option, FWA_E_UNSUPPORTED on a handle that keeps record lists."""
    g = eng_mod.WindowAggregator(A.make_config(window_kind="TUMBLE", size_ms=1000, key_capacity=1 << 15))
    try:
        v = g.get_option("key_table_shape")
        assert K.shape_of(v) == A.key_table_shape(v) == (12, 4) and v == 12 | 4 << 8 and A.OPT_KEY_TABLE_SHAPE == 34
        with pytest.raises(eng_mod.EngineError) as ei:
            g.set_option("key_table_shape", 12)
        assert ei.value.code == -1
    finally:
        g.close()
    g = eng_mod.WindowAggregator(A.make_config(window_kind="TUMBLE", size_ms=1000, key_capacity=1 << 15,
                                               record_lists=True))
    try:
        assert g.record_lists
        with pytest.raises(eng_mod.EngineError) as ei:
            g.get_option("key_table_shape")
        assert ei.value.code == -7
    finally:
        g.close()


# ---- where the keys landed: the table's digest against the model's ----------------------------------------------------
def wrap_waves(shape):
    """The wrap sets as pushes with at most one new key per segment each, so the order of insertion inside a segment is
    the order of the pushes: the main keys, then each segment's own guards, then the next segment's."""
    groups = build_set(shape, "wrap")
    waves = []
    for part, count in ((0, 40), (1, 8), (2, 8)):
        for j in range(count):
            w = [int(groups[3 * s + part][j]) for s in range(len(groups) // 3) if j < len(groups[3 * s + part])]
            assert len(set(K.segment_of(shape, np.array(w, np.int64)).tolist())) == len(w)
            waves.append(w)
    return waves


@pytest.mark.parametrize("path", ["v1_three_columns", "comb_layout0_nv1", "comb_layout1_wide_entries"])
def test_wrap_set_lands_where_the_model_puts_it(eng_mod, path):
    """FWA_OPT_KEY_TABLE_DIGEST against the sequential model's digest: the one check that sees where keys landed rather
    than whether the copies of the probe agree with each other. The one-pass ingest takes one new key per push; the
    combiner one new key per segment per push, beside the keys it already knows."""
    r = Run(eng_mod, path)
    try:
        spec, rng = PATHS[path], np.random.default_rng(5)
        waves = wrap_waves(r.shape)
        model = K.Table(r.shape)
        known = []
        if spec["comb"]:
            r.seed(waves[0][0])
            model.insert(waves[0][0])
        for i, w in enumerate(waves):
            pushes = [[k] for k in w] if not spec["comb"] else [w + known]
            for p in pushes:
                k = np.array(p, np.int64)
                r.push(k, stamps(spec, rng, len(k), 0), columns(spec["cols"], rng, len(k)))
            for key in w:
                assert model.insert(key) >= 0
            known += w
            if i in (7, 39, 47, len(waves) - 1):
                assert r.g.get_option("key_table_digest") == model.digest(), "after wave %d" % i
        assert model.wrapped
        r.check_live_keys()
        r.check_combiner()
        r.fire(A.LONG_MAX)
    finally:
        r.close()


def test_one_pass_ingest_and_combiner_alternate_on_one_table(eng_mod):
    """The general body and the one-pass ingest must agree on every slot: pushes whose slices are new replay through
    the one-pass ingest, the next ones go through the combiner, each bringing another sixth of chain, wrap and dense and
    all the keys before it."""
    path = "comb_layout0_nv1"
    r = Run(eng_mod, path)
    try:
        spec, rng = PATHS[path], np.random.default_rng(6)
        keys = rng.permutation(np.concatenate([np.concatenate(build_set(r.shape, s)) for s in ("chain", "wrap", "dense")]))
        parts = np.array_split(keys, 6)
        replayed = 0
        for i, part in enumerate(parts):
            k = records(rng, np.concatenate(parts[:i + 1]), 4)
            slice0 = 1000 * (i // 2)                        # even pushes open two new slices (far past the lookahead),
            ts = np.sort(rng.integers(1000 * slice0, 1000 * slice0 + 2000, len(k))).astype(np.int64)   # odd ones find them
            r.push(k, ts, columns(spec["cols"], rng, len(k)))
            now = r.g.stats().replay_records
            # (a record replays once per round of slice allocation, so at least once)
            assert (now - replayed >= len(k)) if i % 2 == 0 else (now - replayed < len(k) // 8), (i, now, replayed, len(k))
            replayed = now
            r.check_live_keys()
        assert r.g.stats().partition_ms > 0
        r.fire(A.LONG_MAX)
    finally:
        r.close()


# ---- a full segment ----------------------------------------------------------------------------------------------------
def fill_segment(r, parts, rng, per_push=2048):
    """The segment's keys over three pushes, then every key again (in pushes a sub-bucket list holds): all found."""
    spec = r.spec
    for phase, part in enumerate(list(parts) + ["again"]):
        k = np.concatenate(parts) if isinstance(part, str) else part
        for sl in np.array_split(rng.permutation(k), max(1, len(k) // per_push)):
            r.push(sl, stamps(spec, rng, len(sl), 0), columns(spec["cols"], rng, len(sl)))
        r.check_live_keys()


FULL = [("v1_three_columns", 512), ("v1_three_columns", 4096), ("comb_layout0_nv1", 512), ("comb_layout0_nv1", 4096),
        ("session_preagg_s5_datastream", 512)]


@pytest.mark.parametrize("path,cap", FULL, ids=["%s-%d" % pc for pc in FULL])
def test_full_segment(eng_mod, path, cap):
    """Exactly 2^seg_log keys of one segment at the two smallest tables (key_capacity 512: one segment of 1024 slots;
    4096: 8192 slots, two segments of 4096 where the aggregate list leaves the segments at that size), the s5 route at
    its smallest. Every key is stored and found again and the rows equal the oracle's; then the next new key of the
    segment fails the push with FWA_E_OOM "key table full", and on a second handle filled the same way a new key of
    another segment is accepted. Every probe loop runs to its bound here (DESIGN.md section 7 names the line that
    bounds each)."""
    spec = PATHS[path]
    parts = extra = other = None
    for second in (False, True):
        r = Run(eng_mod, path, key_capacity=cap)
        try:
            assert sum(r.shape) == (10 if cap == 512 else 13), r.shape
            if spec["comb"]:
                assert r.shape == ((10, 0) if cap == 512 else (12, 1)), r.shape
            rng = np.random.default_rng(8)
            if parts is None:
                parts, extra, other = K.full_set(r.shape, rng, K.n_segments(r.shape) - 1)
                K.check_full(r.shape, parts, extra, other)                 # before the first GPU call
            if second and other is None:
                break                                                    # one segment: there is no other one
            if spec["comb"]:
                r.seed(int(parts[0][0]), slices=2)
            fill_segment(r, parts, rng)
            assert r.g.stats().live_keys == 1 << r.shape[0]
            r.check_combiner()
            r.fire(watermark(spec, 0), "full")
            k = np.r_[np.concatenate(parts)[:100], other if second else extra]
            ts, cols = stamps(spec, rng, len(k), 1), columns(spec["cols"], rng, len(k))
            if second:
                r.push(k, ts, cols)
                r.check_live_keys()
                r.fire(A.LONG_MAX, "full")
            else:
                with pytest.raises(eng_mod.EngineError) as ei:
                    r.g.push(k, ts, cols, key_hash=None)
                assert ei.value.code == -5 and "key table full" in str(ei.value), str(ei.value)
        finally:
            r.close()


# ---- (e) PREHASHED ids, (f) restore, (g) partials -----------------------------------------------------------------------
def aimed_mix(shape, sets=("chain", "wrap", "dense")):
    return np.concatenate([np.concatenate(build_set(shape, s)) for s in sets])


def fire_all(handles, wm):
    parts = [h.advance_watermark(wm) for h in handles]
    return {f: np.concatenate([p[f] for p in parts]) for f in parts[0]}


@pytest.mark.parametrize("prehashed", [False, True], ids=["java_long", "prehashed"])
@pytest.mark.parametrize("fan", [1, 2], ids=["1_to_1", "1_to_2"])
def test_snapshot_restore_puts_keys_back_in_probe_order(eng_mod, prehashed, fan):
    """chain, wrap and dense in one table, snapshotted and restored by key group; the same sets pushed again must land
    on the restored keys and not beside them (live_keys stays each handle's share), every restored handle fires exactly
    its share, and a PREHASHED handle's kept hashes follow displaced and wrapped keys (the snapshot carries each key's
    hash; the second snapshot places the keys by it again)."""
    from flink_amd import keygroups as KG
    from flink_amd import snapshot as S
    from oracle.oracle import Oracle
    kind = A.KEY_PREHASHED if prehashed else A.KEY_JAVA_LONG
    kw = dict(window_kind="TUMBLE", size_ms=1000, aggs=[("COUNT", 0), ("SUM_I64", 0), ("MAX_I64", 0)],
              key_capacity=1 << 13, key_kind=kind)
    cfg = A.make_config(**kw)
    names = A.agg_names(cfg)
    one, o = eng_mod.WindowAggregator(cfg), Oracle(A.make_config(**kw))
    shape = K.shape_of(one.get_option("key_table_shape"))
    keys = aimed_mix(shape)
    kh = (lambda k: hash_of(k)) if prehashed else (lambda k: None)
    kgs = np.array([key_group(k, kind) for k in keys.tolist()])
    rng = np.random.default_rng(10)

    def batch(phase):
        """Every key four times in each of the slices phase and phase + 1."""
        k, sl = np.tile(keys, 8), np.repeat(np.arange(8) % 2, len(keys))
        order = rng.permutation(len(k))
        ts = (1000 * (phase + sl) + rng.integers(0, 1000, len(k))).astype(np.int64)
        return k[order], ts[order], [rng.integers(-I32, I32, len(k)).astype(np.int64)]

    k, ts, cols = batch(0)
    assert one.push(k, ts, cols, key_hash=kh(k)) == o.push(k, ts, cols, key_hash=kh(k)) == 0
    assert one.stats().live_keys == len(keys)
    blob = one.snapshot()
    one.close()
    snap = S.parse(blob)
    assert sorted(set(snap["key"].tolist())) == sorted(keys.tolist())
    if prehashed:
        assert np.array_equal(snap["key_hash"], hash_of(snap["key"]))
    ranges = [KG.key_group_range_for_operator(128, fan, i) for i in range(fan)]
    hs = [eng_mod.WindowAggregator(A.make_config(kg_start=lo, kg_end=hi, **kw)) for lo, hi in ranges]
    try:
        share = [(kgs >= lo) & (kgs <= hi) for lo, hi in ranges]
        assert all(m.sum() > 40 for m in share)
        for h, m in zip(hs, share):
            h.restore(blob)
            assert K.shape_of(h.get_option("key_table_shape")) == shape
            assert h.stats().live_keys == m.sum()
        k, ts, cols = batch(1)
        o.push(k, ts, cols, key_hash=kh(k))
        of = np.isin(k, keys[share[0]])
        for h, m, sel in zip(hs, share, [of, ~of] if fan == 2 else [np.ones(len(k), bool)]):
            h.push(k[sel], ts[sel], [cols[0][sel]], key_hash=kh(k[sel]))
            assert h.stats().live_keys == m.sum(), "a restored key was inserted beside itself"
        got = [h.advance_watermark(999) for h in hs]
        for rows, m in zip(got, share):
            assert set(rows["key"].tolist()) == set(keys[m].tolist())       # exactly its share
        want = o.advance_watermark(999)
        assert_rows_equal({f: np.concatenate([p[f] for p in got]) for f in got[0]}, want, names, ctx="after the restore")
        if prehashed:
            for h in hs:
                again = S.parse(h.snapshot())
                assert np.array_equal(again["key_hash"], hash_of(again["key"]))
        assert_rows_equal(fire_all(hs, A.LONG_MAX), o.advance_watermark(A.LONG_MAX), names, ctx="the rest")
    finally:
        for h in hs:
            h.close()
        o.close()


@pytest.mark.parametrize("aggs", [[("COUNT", 0), ("SUM_I64", 0)], [("COUNT", 0), ("SUM_I64", 0), ("MAX_I64", 0)]],
                         ids=["two_phase_rows", "one_pass_rows"])
@pytest.mark.parametrize("how", ["drain_then_push_partials", "drain_route_then_fire_partials"])
def test_partials_of_aimed_keys(eng_mod, how, aggs):
    """The local handle's partial rows of the wrap and dense sets, twice: drained and pushed into an owner's table,
    which inserts the keys from the first rows and finds them from the second; and drained by destination and fired on
    chip by the owner (the local's table and presence test alone)."""
    from oracle.oracle import Oracle
    kw = dict(window_kind="TUMBLE", size_ms=1000, aggs=aggs, key_capacity=1 << 13)
    names = A.agg_names(A.make_config(**kw))
    local = eng_mod.WindowAggregator(A.make_config(output_on_device=int(how != "drain_then_push_partials"), **kw))
    owner, o = eng_mod.WindowAggregator(A.make_config(**kw)), Oracle(A.make_config(**kw))
    try:
        shape = K.shape_of(owner.get_option("key_table_shape"))
        assert K.shape_of(local.get_option("key_table_shape")) == shape
        keys = aimed_mix(shape, ("wrap", "dense"))
        rng = np.random.default_rng(11)
        ship = [j for j, nm in enumerate(names) if nm != "COUNT"]
        cells = [2 if nm == "COUNT" else 3 + ship.index(j) for j, nm in enumerate(names)]
        for phase in (0, 1):
            k = records(rng, keys, 6)
            ts = np.sort(rng.integers(1000 * phase, 1000 * phase + 1000, len(k))).astype(np.int64)
            cols = [rng.integers(-I32, I32, len(k)).astype(np.int64)]
            assert local.push(k, ts, cols) == o.push(k, ts, cols) == 0
            wm = 1000 * phase + 999
            if how == "drain_then_push_partials":
                p = local.drain_partials(wm)
                assert len(p["key"]) == len(keys)
                owner.push_partials(p["key"], p["slice_start"], p["count"], [p["acc%d" % j] for j in range(len(names))])
                got = owner.advance_watermark(wm)
            else:
                parts, counts, m = local.drain_route(wm, 1)
                assert counts == [len(keys)] and m == 3 + len(ship)
                got = owner.fire_partials(parts[0], cells, wm)
            assert_rows_equal(got, o.advance_watermark(wm), names, ctx="%s phase %d" % (how, phase))
            assert local.stats().live_keys == len(keys)
            if how == "drain_then_push_partials":
                assert owner.stats().live_keys == len(keys)
            else:                                   # merged and fired on chip: the owner's table is not involved, the
                assert owner.get_option("fire_partials") == phase + 1      # local's is read in slot order by the drain
    finally:
        local.close()
        owner.close()
        o.close()
