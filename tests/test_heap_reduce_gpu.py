"""GPU tests: Flink heap checkpoints (fwa_snapshot_heap* / fwa_restore_heap*) of DataStream reductions and of
String-keyed handles.

 * the reference's own reduce checkpoint (win-op-migration-test-reduce-event-time-flink1.18-snapshot: a
   ReducingState<Tuple2<String, Integer>> keyed by a String) restored from its key-group section as it stands, replayed
   as WindowOperatorMigrationTest.java:494-507 does, and written again;
 * bytes: the engine's body parsed by tests/heap_reader.py (every byte consumed), written again by
   tests/heap_tuple_ref.py (byte for byte equal), and every unfired window's reduced tuple compared with an
   arrival-order fold in numpy over the accepted records. The streams hold small integers and multiples of 0.5, so every
   sum is exact in float and double and the comparison is ==;
 * restore with rescaling against the oracle's uninterrupted run, reductions and String-keyed aggregates. String keys
   go through dictionary ids and wire.jstring_hash again after the restore, so restored and new records of a key meet
   only if the restore computed the same String.hashCode() and encoded the same char bytes;
 * the refusals, each with its reason in fwa_last_error.
"""
import os
import struct

import numpy as np
import pytest

import heap_reader as H
import heap_tuple_ref as W
from flink_amd import _abi as A
from helpers import reduce_aggs, reduce_field_values
from test_reduce_gpu import _close, _stream

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "flink_snapshots",
                       "win-op-migration-test-reduce-event-time-flink1.18-snapshot")
TYPES = ("I32", "F64", "I64", "F32")                       # fields f1..f4 = value columns 0..3
RD = {"I32": H.ser_int, "I64": H.ser_long, "F64": W.ser_double, "F32": W.ser_float}
WR = {"I32": W.w_int, "I64": W.w_long, "F64": W.w_double, "F32": W.w_float}
NP = {"I32": np.int32, "I64": np.int64, "F64": np.float64, "F32": np.float32}
SESSION_KIND_TYPE = {"I32": 0, "F64": 1, "I64": 2, "F32": 3}


@pytest.fixture(scope="module")
def eng():
    from flink_amd import engine
    engine.lib()
    return engine


def key_text(i):
    """The String of key number i: the empty string, 1-, 2- and 3-byte chars"""
    return "" if i == 0 else ("ключ%d", "键%d", "k€y%d", "key%d", "key%d", "key%d", "key%d")[i % 7] % i


class Keys:
    """The key column of a stream as Long keys, or as Strings behind a one-field STRING dictionary (ids beside
    String.hashCode(), computed on the device by wire.jstring_hash)."""

    def __init__(self, keys, strings, maxp=128):
        self.strings, self.maxp = strings, maxp
        self.uniq, self.idx = np.unique(keys, return_inverse=True)
        self.long = keys
        self.texts = [key_text(i) for i in range(len(self.uniq))]

    @property
    def key_kind(self):
        return A.KEY_PREHASHED if self.strings else A.KEY_JAVA_LONG

    def new_dict(self):
        if not self.strings:
            return None
        from flink_amd.keydict import KeyDictionary
        return KeyDictionary(["STRING"], max_parallelism=self.maxp, capacity=4096)

    def ids_and_hash(self, kd):
        """(engine key per record, hashCode per record or None, engine key -> key number)"""
        if not self.strings:
            return self.long, None, {int(k): i for i, k in enumerate(self.uniq)}
        import torch
        from flink_amd import wire
        raw = [wire.jstring_bytes(t) for t in self.texts]
        offs = np.zeros(len(raw) + 1, np.int32)
        offs[1:] = np.cumsum([len(b) for b in raw])
        data = np.frombuffer(b"".join(raw), np.uint8).copy()
        h = wire.jstring_hash(torch.from_numpy(offs).cuda(), torch.from_numpy(data).cuda()).cpu().numpy()
        assert [int(x) for x in h] == [W.java_string_hash(t) for t in self.texts]
        ids = kd.encode([raw]).cpu().numpy()
        return ids[self.idx], h[self.idx].astype(np.int32), {int(k): i for i, k in enumerate(ids)}


def bits(v, t):
    if t == "F64":
        return int(np.float64(v).view(np.uint64))
    if t == "F32":
        return int(np.float32(v).view(np.uint32))
    return int(v)


def stream4(seed, n, nkeys, span):
    keys, ts, cols = _stream(seed, n, nkeys, span, True)
    return keys, ts, cols + [(cols[1] * 3).astype(np.float32)]


def fold(op, pos, by_last, rows):
    """HeapReducingState.add over `rows` (tuples of the fields f1..fn, arrival order) with SumAggregator /
    ComparableAggregator (ComparableAggregator.java:83-107)."""
    acc = list(rows[0])
    p = pos - 1
    for r in rows[1:]:
        if op == "sum":
            acc[p] = type(acc[p])(acc[p] + r[p])
        elif op == "min":
            acc[p] = min(acc[p], r[p])
        elif op == "max":
            acc[p] = max(acc[p], r[p])
        else:
            better = r[p] < acc[p] if op == "min_by" else r[p] > acc[p]
            if better or (by_last and r[p] == acc[p]):
                acc = list(r)
    return acc


def layouts(strings, sess, field_types, key_pos):
    kr, kw = (H.ser_string, W.w_string) if strings else (H.ser_long, W.w_long)
    tr = [RD[t] for t in field_types]
    tw = [WR[t] for t in field_types]
    tr.insert(key_pos, kr)
    tw.insert(key_pos, kw)
    rl = {0: ("kv", H.ser_time_window, kr, H.ser_tuple(*tr))}
    wl = {0: ("kv", W.w_time_window, kw, W.w_tuple(*tw))}
    nxt = 1
    if sess:
        rl[1] = ("kv", H.ser_void, kr, H.ser_list(H.ser_tuple(H.ser_time_window, H.ser_time_window)))
        wl[1] = ("kv", W.w_void, kw, W.w_list(W.w_tuple(W.w_time_window, W.w_time_window)))
        nxt = 2
    for sid in (nxt, nxt + 1):
        rl[sid] = ("pq", kr, H.ser_time_window)
        wl[sid] = ("pq", kw, W.w_time_window)
    return rl, wl


def parse_and_rewrite(body, offs, rl, wl, first_kg=0):
    """heap_reader over the whole body (each section read to its last byte, the sections back to back from 0 to the
    end), then the parsed entries written again in the same order: the same bytes."""
    assert offs[0] == 0 and list(offs) == sorted(offs)
    secs = H.read_key_groups(body, [int(o) for o in offs], first_kg, rl)
    for s in secs.values():
        assert list(s) == sorted(rl), "every state section, in id order"
    again, offs2 = W.write_key_groups(secs, wl)
    assert offs2 == [int(o) for o in offs]
    assert again == body
    return secs


# ------------------------------------------------------------------------------------------------
# the reference's checkpoint, without an adapter

def test_reference_reduce_snapshot_restores_as_it_stands(eng):
    from flink_amd.keydict import KeyDictionary
    first, offs, data = H.read_operator_snapshot(open(FIXTURE, "rb").read())[0]
    assert first == 0 and len(offs) == 1
    section = data[offs[0]:]
    rl, wl = layouts(True, False, ["I32"], 0)
    ref = H.read_key_groups(data, offs, first, rl)[0]
    kd = KeyDictionary(["STRING"], max_parallelism=1, capacity=64)
    cfg = A.make_config(window_kind="TUMBLE", size_ms=3000, aggs=[("SUM_I32", 0)], reduce=True, key_kind=A.KEY_PREHASHED,
                        max_parallelism=1, key_capacity=64)
    g = eng.WindowAggregator(cfg, options={"heap_key_pos": 0})
    assert g.get_option("heap_key_pos") == 0
    g.restore_heap([section], [1999], keydict=kd)
    body, boffs, wm = g.snapshot_heap(keydict=kd)
    assert wm == 1999 and list(boffs) == [0]
    mine = parse_and_rewrite(body, boffs, rl, wl)[0]
    assert sorted(mine[0]) == sorted(ref[0]) and len(ref[0]) == 3
    assert mine[1] == ref[1] == []
    assert sorted(mine[2]) == sorted(ref[2]) and len(ref[2]) == 3
    out = {}
    for w in (2999, 3999, 4999, 5999):                                   # WindowOperatorMigrationTest.java:494-507
        r = g.advance_watermark(w)
        names = kd.decode(r["key"], with_nulls=False)[0] if len(r["key"]) else []
        out[w] = sorted(zip(names, np.asarray(r["agg0"]).tolist(), np.asarray(r["win_end"]).tolist()))
    assert out == {2999: [("key1", 3, 3000), ("key2", 3, 3000)], 3999: [], 4999: [], 5999: [("key2", 2, 6000)]}
    g.close()
    kd.close()


# ------------------------------------------------------------------------------------------------
# bytes

TUMBLE_CASES = [  # op, pos, by_last, String keys, key position, allowed lateness
    ("sum", 1, False, False, 0, 0), ("sum", 2, False, True, 2, 1500), ("sum", 4, False, False, 4, 0),
    ("sum", 3, False, True, 1, 0), ("min", 3, False, True, 0, 0), ("max", 4, False, False, 1, 1500),
    ("min_by", 2, False, True, 4, 0), ("min_by", 1, True, False, 2, 1500), ("max_by", 3, False, False, 0, 0),
    ("max_by", 4, True, True, 3, 1500)]


@pytest.mark.parametrize("op,pos,by_last,strings,key_pos,late", TUMBLE_CASES,
                         ids=["%s%d_%s_%s_pos%d_late%d" % (c[0], c[1], "last" if c[2] else "first", "str" if c[3] else "long",
                                                           c[4], c[5]) for c in TUMBLE_CASES])
def test_tumble_reduction_bytes(eng, op, pos, by_last, strings, key_pos, late):
    size = 1000
    keys, ts, cols = stream4(11 + pos, 20_000, 300, 30_000)
    K = Keys(keys, strings)
    kd = K.new_dict()
    ek, eh, num_of = K.ids_and_hash(kd)
    cfg = A.make_config(window_kind="TUMBLE", size_ms=size, allowed_lateness_ms=late, aggs=reduce_aggs(op, pos, TYPES),
                        reduce=True, by_last=by_last, key_kind=K.key_kind, key_capacity=4096)
    g = eng.WindowAggregator(cfg, options={"heap_key_pos": key_pos})
    nb, cut, mx, wm = 8, 4, -2**63, A.LONG_MIN
    accepted = np.zeros(len(keys), bool)
    wstart = ts - ts % size
    for b in range(cut):
        sl = slice(b * len(keys) // nb, (b + 1) * len(keys) // nb)
        accepted[sl] = wstart[sl] + size - 1 + late > wm               # WindowOperator.isWindowLate at arrival
        dropped = g.push(ek[sl], ts[sl], [c[sl] for c in cols], key_hash=None if eh is None else eh[sl])
        assert dropped == int((~accepted[sl]).sum())
        mx = max(mx, int(ts[sl].max()))
        wm = mx - 801
        g.advance_watermark(wm)
    body, offs, swm = g.snapshot_heap(keydict=kd)
    g.close()
    assert swm == wm and len(offs) == 128
    rl, wl = layouts(strings, False, TYPES, key_pos)
    secs = parse_and_rewrite(body, offs, rl, wl)
    # expected state: the fold of each (key, window)'s accepted records, for windows not yet cleaned up
    order = np.lexsort((np.arange(len(keys)), wstart, K.idx))
    order = order[accepted[order]]
    exp = {}
    fields = [c.astype(NP[t]) for c, t in zip(cols, TYPES)]
    at = 0
    while at < len(order):
        i = order[at]
        end = at
        while end < len(order) and K.idx[order[end]] == K.idx[i] and wstart[order[end]] == wstart[i]:
            end += 1
        if wstart[i] + size - 1 + late > wm:
            rows = [tuple(f[j] for f in fields) for j in order[at:end]]
            exp[(int(K.idx[i]), int(wstart[i]))] = [bits(v, t) for v, t in zip(fold(op, pos, by_last, rows), TYPES)]
        at = end
    text_num = {t: i for i, t in enumerate(K.texts)}
    got, unfired = {}, 0
    for kg, s in secs.items():
        timers = set()
        for (st, en), key, tup in s[0]:
            num = text_num[key] if strings else num_of[key]
            assert en == st + size and tup[key_pos] == key
            assert (num, st) not in got
            got[(num, st)] = list(tup[:key_pos] + tup[key_pos + 1:])
            timers.add((en - 1 + late, key, (st, en)))                   # the cleanup timer, always
            if en - 1 > wm:
                timers.add((en - 1, key, (st, en)))                      # the trigger's, until the window fires
        assert s[1] == []
        assert set(s[2]) == timers and len(s[2]) == len(timers)
    assert sorted(got) == sorted(exp)
    for k, tup in got.items():
        if k[1] + size - 1 > wm:                                        # unfired: the arrival-order fold, bit for bit
            unfired += 1
            assert tup == exp[k], (k, tup, exp[k])
    assert unfired > 100
    if kd is not None:
        kd.close()


SESSION_CASES = [("SUM_I32", False, 0), ("MIN_F64", True, 1), ("MAXBY_I64", False, 1), ("SUM_F32", True, 0),
                 ("MAX_I32", True, 0), ("MINBY_F32", False, 1)]


@pytest.mark.parametrize("kind,strings,key_pos", SESSION_CASES, ids=["%s_%s_pos%d" % (c[0], "str" if c[1] else "long", c[2])
                                                                      for c in SESSION_CASES])
def test_session_reduction_bytes(eng, kind, strings, key_pos):
    """Tuple2<key, f1> session reductions, checkpointed before the first watermark (every record accepted, every session
    in flight): window-contents under each session's state window, the merging-window-set, the timers."""
    gap = 500
    t = kind.rsplit("_", 1)[1]
    keys, ts, cols = stream4(41 + key_pos, 20_000, 300, 30_000)
    K = Keys(keys, strings)
    kd = K.new_dict()
    ek, eh, num_of = K.ids_and_hash(kd)
    cfg = A.make_config(window_kind="SESSION", gap_ms=gap, size_ms=0, aggs=[(kind, SESSION_KIND_TYPE[t])], reduce=True,
                        key_kind=K.key_kind, key_capacity=4096)
    g = eng.WindowAggregator(cfg, options={"heap_key_pos": key_pos})
    n = len(keys) // 2
    for sl in (slice(0, n // 2), slice(n // 2, n)):
        assert g.push(ek[sl], ts[sl], [c[sl] for c in cols], key_hash=None if eh is None else eh[sl]) == 0
    body, offs, swm = g.snapshot_heap(keydict=kd)
    g.close()
    assert swm == A.LONG_MIN
    rl, wl = layouts(strings, True, [t], key_pos)
    secs = parse_and_rewrite(body, offs, rl, wl)
    col = cols[SESSION_KIND_TYPE[t]][:n].astype(NP[t])
    exp = {}
    order = np.lexsort((ts[:n], K.idx[:n]))
    at = 0
    while at < len(order):                                               # EventTimeSessionWindows + MergingWindowSet
        end = at + 1
        while end < len(order) and K.idx[order[end]] == K.idx[order[at]] and ts[order[end]] <= ts[order[end - 1]] + gap:   # (TimeWindow.intersects)
            end += 1
        v = col[order[at:end]]
        r = v.sum(dtype=NP[t]) if kind.startswith("SUM") else (v.min() if kind.startswith("MIN") else v.max())
        exp[(int(K.idx[order[at]]), int(ts[order[at]]), int(ts[order[end - 1]]) + gap)] = bits(r, t)
        at = end
    text_num = {x: i for i, x in enumerate(K.texts)}
    got, nsets = {}, 0
    for kg, s in secs.items():
        state = set()
        for (st, en), key, tup in s[0]:
            assert tup[key_pos] == key
            got[(text_num[key] if strings else num_of[key], st, en)] = tup[1 - key_pos]
            state.add((key, (st, en)))
        mapped = {(key, sw) for _, key, pairs in s[1] for aw, sw in pairs}
        assert all(aw == sw for _, _, pairs in s[1] for aw, sw in pairs) and mapped == state
        assert s[2] == [] and {(k, ns) for tt, k, ns in s[3] if tt == ns[1] - 1} == state and len(s[3]) == len(state)
        nsets += len(s[1])
    assert got == exp and nsets == len({k[0] for k in exp}) and len(exp) > 1000
    if kd is not None:
        kd.close()


# ------------------------------------------------------------------------------------------------
# restore and rescale

def run_rescale(eng, kw, K, keys, ts, cols, key_pos, rows_of, close, check_bytes=None):
    """Checkpoint a handle over all key groups mid-stream in the heap layout, restore it into one subtask and into two
    with a new key-group split, push the rest: the rows of every later watermark equal the oracle's uninterrupted run."""
    from oracle.oracle import Oracle
    ocfg = A.make_config(**kw)                                           # the oracle runs on the key numbers
    nb, cut, mx = 8, 4, -2**63
    okeys = K.idx.astype(np.int64)
    o = Oracle(ocfg)
    exp, wms = [], []
    for b in range(nb + 1):
        sl = slice(b * len(keys) // nb, (b + 1) * len(keys) // nb) if b < nb else slice(0, 0)
        o.push(okeys[sl], ts[sl], [c[sl] for c in cols])
        if b < nb:
            mx = max(mx, int(ts[sl].max()))
        wms.append(mx - 801 if b < nb else A.LONG_MAX)
        exp.append(rows_of(o.advance_watermark(wms[-1]), None))
    o.close()
    opts = {} if key_pos is None else {"heap_key_pos": key_pos}
    kd = K.new_dict()
    ek, eh, num_of = K.ids_and_hash(kd)
    g = eng.WindowAggregator(A.make_config(key_kind=K.key_kind, **kw), options=opts)
    for b in range(cut):
        sl = slice(b * len(keys) // nb, (b + 1) * len(keys) // nb)
        g.push(ek[sl], ts[sl], [c[sl] for c in cols], key_hash=None if eh is None else eh[sl])
        close(rows_of(g.advance_watermark(wms[b]), num_of), exp[b])
    body, offs, swm = g.snapshot_heap(keydict=kd)
    g.close()
    if kd is not None:
        kd.close()
    if check_bytes:
        check_bytes(body, offs)
    for layout in ([(0, 127)], [(0, 31), (32, 127)]):
        kd2 = K.new_dict()                                               # a new job: its own dictionary
        subs = []
        for lo, hi in layout:
            h = eng.WindowAggregator(A.make_config(key_kind=K.key_kind, kg_start=lo, kg_end=hi, **kw), options=opts)
            h.restore_heap([body], [swm], keydict=kd2)
            subs.append((h, lo, hi))
        ek2, eh2, num2 = K.ids_and_hash(kd2)
        if kd2 is not None:
            assert kd2.size() == len(K.texts)                            # restored keys met their own strings
        kgs = np.asarray(eng.key_groups(ek2, 128, 1, K.key_kind, eh2)[0])
        for b in range(cut, nb + 1):
            sl = slice(b * len(keys) // nb, (b + 1) * len(keys) // nb) if b < nb else slice(0, 0)
            got = []
            for h, lo, hi in subs:
                m = (kgs[sl] >= lo) & (kgs[sl] <= hi)
                h.push(ek2[sl][m], ts[sl][m], [c[sl][m] for c in cols], key_hash=None if eh2 is None else eh2[sl][m])
                got += rows_of(h.advance_watermark(wms[b]), num2)
            close(sorted(got), exp[b])
        for h, _, _ in subs:
            h.close()
        if kd2 is not None:
            kd2.close()


def renumber(rows, num_of):
    return rows if num_of is None else sorted((num_of[r[0]],) + r[1:] for r in rows)


RESCALE_TUMBLE = [("sum", 2, False, True, 2, 0), ("min_by", 3, True, False, 0, 1500), ("max", 1, False, True, 4, 1500),
                  ("max_by", 4, False, True, 1, 0), ("sum", 4, False, False, 3, 1500)]


@pytest.mark.parametrize("op,pos,by_last,strings,key_pos,late", RESCALE_TUMBLE,
                         ids=["%s%d_%s_%s_late%d" % (c[0], c[1], "last" if c[2] else "first", "str" if c[3] else "long", c[5])
                              for c in RESCALE_TUMBLE])
def test_tumble_reduction_restore_rescale(eng, op, pos, by_last, strings, key_pos, late):
    kw = dict(window_kind="TUMBLE", size_ms=1000, allowed_lateness_ms=late, aggs=reduce_aggs(op, pos, TYPES), reduce=True,
              by_last=by_last, key_capacity=4096)
    names = A.agg_names(A.make_config(**kw))
    keys, ts, cols = stream4(71 + pos, 20_000, 300, 30_000)
    run_rescale(eng, kw, Keys(keys, strings), keys, ts, cols, key_pos,
                lambda r, m: renumber(reduce_field_values(r, names, TYPES), m), lambda a, b: _close(a, b, names))


RESCALE_SESSION = [("SUM_I64", False, 0, 0), ("MIN_I32", True, 1, 1500), ("MAXBY_F64", False, 1, 1500), ("SUM_F32", True, 0, 0)]


@pytest.mark.parametrize("kind,strings,key_pos,late", RESCALE_SESSION,
                         ids=["%s_%s_late%d" % (c[0], "str" if c[1] else "long", c[3]) for c in RESCALE_SESSION])
def test_session_reduction_restore_rescale(eng, kind, strings, key_pos, late):
    t = kind.rsplit("_", 1)[1]
    kw = dict(window_kind="SESSION", gap_ms=500, size_ms=0, allowed_lateness_ms=late, aggs=[(kind, SESSION_KIND_TYPE[t])],
              reduce=True, key_capacity=4096)
    names = A.agg_names(A.make_config(**kw))
    keys, ts, cols = stream4(81 + key_pos, 20_000, 300, 30_000)
    run_rescale(eng, kw, Keys(keys, strings), keys, ts, cols, key_pos,
                lambda r, m: renumber(reduce_field_values(r, names, [t]), m), lambda a, b: _close(a, b, names))


@pytest.mark.parametrize("win", [dict(window_kind="TUMBLE", size_ms=1000, allowed_lateness_ms=1500),
                                 dict(window_kind="SLIDE", size_ms=3000, slide_ms=1000, offset_ms=300),
                                 dict(window_kind="SESSION", gap_ms=500, size_ms=0)], ids=["tumble", "slide", "session"])
def test_string_keyed_aggregates_restore_rescale(eng, win):
    """COUNT + SUM_I64 + MAX_F64 of a String-keyed DataStream job: only the key bytes are new in the body."""
    kw = dict(aggs=[("COUNT", 0), ("SUM_I64", 2), ("MAX_F64", 1)], key_capacity=4096, **win)
    keys, ts, cols = _stream(91, 20_000, 300, 30_000, True)

    def rows_of(r, m):
        rows = sorted(zip(np.asarray(r["key"]).tolist(), np.asarray(r["win_start"]).tolist(), np.asarray(r["win_end"]).tolist(),
                          np.asarray(r["agg0"]).tolist(), np.asarray(r["agg1"]).tolist(), np.asarray(r["agg2"]).tolist()))
        return renumber(rows, m)

    def close(a, b):
        assert a == b

    sess = win["window_kind"] == "SESSION"

    def check_bytes(body, offs):
        kr, kw_ = H.ser_string, W.w_string
        acc_r, acc_w = H.ser_tuple(*[H.ser_ulong] * 4), W.w_tuple(*[W.w_double] * 4)   # COUNT(*) + 3 ACC fields, 8 bytes
        rl, wl = layouts(True, sess, [], 0)
        rl[0], wl[0] = ("kv", H.ser_time_window, kr, acc_r), ("kv", W.w_time_window, kw_, acc_w)
        secs = parse_and_rewrite(body, offs, rl, wl)
        assert sum(len(s[0]) for s in secs.values()) > 100

    run_rescale(eng, kw, Keys(keys, True), keys, ts, cols, None, rows_of, close, check_bytes)


# ------------------------------------------------------------------------------------------------
# refusals

def refused(eng, call, code, *words):
    with pytest.raises(eng.EngineError) as ei:
        call()
    assert A.STATUS[ei.value.code] == code, str(ei.value)
    for w in words:
        assert w in str(ei.value), str(ei.value)


def test_refusals_name_their_reason(eng):
    from flink_amd.keydict import KeyDictionary
    red = dict(aggs=[("SUM_I64", 0), ("FIRST_64", 1)], reduce=True, key_capacity=64)
    g = eng.WindowAggregator(A.make_config(**red))
    assert g.get_option("heap_key_pos") == -1
    refused(eng, g.snapshot_heap, "E_UNSUPPORTED", "FWA_OPT_HEAP_KEY_POS")          # not declared
    refused(eng, lambda: g.restore_heap([struct.pack(">i", 0)], [0]), "E_UNSUPPORTED", "FWA_OPT_HEAP_KEY_POS")
    refused(eng, lambda: g.set_option("heap_key_pos", 3), "E_ARG", "FWA_OPT_HEAP_KEY_POS")
    refused(eng, lambda: g.set_option("heap_key_pos", -1), "E_ARG", "FWA_OPT_HEAP_KEY_POS")
    g.set_option("heap_key_pos", 2)
    assert g.get_option("heap_key_pos") == 2
    g.snapshot_heap()
    g.close()
    g = eng.WindowAggregator(A.make_config(window_kind="SLIDE", size_ms=3000, slide_ms=1000, **red), options={"heap_key_pos": 0})
    refused(eng, g.snapshot_heap, "E_UNSUPPORTED", "SLIDE reduction", "slice")
    g.close()
    for kw in (dict(aggs=[("SUM_F32", 0)], reduce=True), dict(aggs=[("COUNT", 0), ("SUM_F32", 0)])):
        g = eng.WindowAggregator(A.make_config(f32_fold=True, key_capacity=64, **kw))
        if kw.get("reduce"):
            g.set_option("heap_key_pos", 0)
        refused(eng, g.snapshot_heap, "E_UNSUPPORTED", "FWA_CFG_F32_FOLD")
        g.close()
    agg = dict(aggs=[("COUNT", 0), ("SUM_I64", 0)], key_capacity=64)
    g = eng.WindowAggregator(A.make_config(key_kind=A.KEY_PREHASHED, **agg))
    refused(eng, g.snapshot_heap, "E_UNSUPPORTED", "without a key dictionary")
    for types in (["STRING", "BIGINT"], ["BIGINT"]):
        kd = KeyDictionary(types, max_parallelism=128, capacity=64)
        refused(eng, lambda: g.snapshot_heap(keydict=kd), "E_UNSUPPORTED", "exactly one STRING field")
        refused(eng, lambda: g.restore_heap([struct.pack(">i", 0)], [0], keydict=kd), "E_UNSUPPORTED", "exactly one STRING field")
        kd.close()
    g.close()
    kd = KeyDictionary(["STRING"], max_parallelism=128, capacity=64)
    g = eng.WindowAggregator(A.make_config(**agg))                               # JAVA_LONG keys beside a dictionary
    refused(eng, lambda: g.snapshot_heap(keydict=kd), "E_UNSUPPORTED", "not dictionary ids")
    g.close()
    # malformed String keys: the null string, char 0 coded in two bytes, a length past the section
    lay = ("kv", W.w_time_window, lambda raw: raw, W.w_tuple(W.w_long, W.w_long, W.w_long))
    pq = ("pq", lambda raw: raw, W.w_time_window)
    for raw in (b"\x00", b"\x02\x80\x00", b"\x02\x80\x80\x80\x01", b"\x7fabc"):
        body = W.write_key_group(0, [(0, lay, [((0, 10_000), raw, (1, 1, 5))]), (1, pq, []), (2, pq, [])])
        g = eng.WindowAggregator(A.make_config(key_kind=A.KEY_PREHASHED, max_parallelism=1, **agg))
        refused(eng, lambda: g.restore_heap([body], [0], keydict=kd), "E_ARG", "heap body")
        g.close()
    good = W.write_key_group(0, [(0, lay, [((0, 10_000), W.w_string("né中"), (1, 1, 5))]), (1, pq, []), (2, pq, [])])
    g = eng.WindowAggregator(A.make_config(key_kind=A.KEY_PREHASHED, max_parallelism=1, **agg))
    g.restore_heap([good], [0], keydict=kd)                                      # (the same body with a sound key is taken)
    r = g.advance_watermark(A.LONG_MAX)
    assert np.asarray(r["agg1"]).tolist() == [5]
    g.close()
    kd.close()
