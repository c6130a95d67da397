"""GPU wire decoder on BinaryRowData rows with STRING fields (FWA_FIELD_STRING) against the sequential reference
decoder of tests/wire_strings_ref.py, bit for bit: key / ts / value columns where the schema has them, NULL flags,
events, `consumed`, and per STRING field the Arrow offsets, bytes and NULL flags of fwa_wire_strings_of; host bytes and
a device tensor both. Then the refusals (with byte positions, and the decoder usable afterwards), the unchanged
fixed-length schemas, and a VARCHAR-keyed Table job end to end: channel bytes -> NetworkInput -> key dictionary ids ->
window engine, fired rows decoded back to their strings and compared with the window oracle."""
import struct
from collections import Counter

import numpy as np
import pytest

from flink_amd import _abi as A
from flink_amd import wire
from oracle import oracle as O
from oracle import wire_encode as W

import wire_strings_ref as R
from test_keydict_strings_gpu import WORDS

pytestmark = pytest.mark.gpu

UTV = ["STRING", "LONG", "LONG"]                 # VARCHAR user, TIMESTAMP(3) rowtime, BIGINT v


class Sch:
    def __init__(self, fields, key_field=-1, ts_field=-1, cols=()):
        self.fields, self.key_field, self.ts_field, self.cols = fields, key_field, ts_field, list(cols)
        self.schema = wire.make_schema(fields, key_field=key_field, ts_field=ts_field, cols=cols, fmt="ROWDATA")
        self.sf = [f for f, t in enumerate(fields) if t == "STRING"]

    def ref(self, data):
        return R.decode(self.fields, data, self.key_field, self.ts_field, self.cols)


UTV_S = dict(fields=UTV, key_field=-1, ts_field=1, cols=[2])


def check(dec, sch, data, device=False, ref=None):
    import torch
    if ref is None:
        rc, ref = sch.ref(data)
        assert rc == 0
    x = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if device and len(data) else data
    got = dec.decode(x)
    assert (got.n_records, got.n_events, got.consumed) == (ref["n_records"], ref["n_events"], ref["consumed"])
    assert np.array_equal(got.ts.cpu().numpy(), ref["ts"])
    if sch.key_field >= 0:
        assert np.array_equal(got.key.cpu().numpy(), ref["key"])
        assert np.array_equal(got.key_null.cpu().numpy(), ref["key_null"])
    else:
        assert got.key is None and got.key_null is None
    for a, b, an, bn in zip(got.cols, ref["cols"], got.col_null, ref["col_null"]):
        assert np.array_equal(a.cpu().numpy().view(np.uint8), b.view(np.uint8))
        assert np.array_equal(an.cpu().numpy(), bn)
    assert np.array_equal(got.evt_pos, ref["evt_pos"]) and np.array_equal(got.evt_tag, ref["evt_tag"])
    assert np.array_equal(got.evt_val, ref["evt_val"])
    for f in sch.sf:
        o, b, z = got.strings(f)
        ro, rb, rz = ref["strings"][f]
        o = o.cpu().numpy()
        assert o.dtype == np.int32 and np.array_equal(o, ro)
        assert np.array_equal(b.cpu().numpy()[:ro[-1]], rb)
        assert np.array_equal(z.cpu().numpy(), rz)
    return got, ref


def words(rng, n, lo=8, hi=40, null_p=0.0):
    """n values: WORDS now and then, else random printable strings of lo..hi bytes; None with probability null_p."""
    out = []
    for i in range(n):
        if rng.random() < null_p:
            out.append(None)
        elif i % 9 == 0:
            out.append(WORDS[(i // 9) % len(WORDS)])
        else:
            out.append(bytes(rng.integers(0x20, 0x7F, int(rng.integers(lo, hi + 1)), dtype=np.uint8)).decode())
    return out


def utv_stream(rng, n, n_events=None, with_ts=False, strs=None):
    strs = words(rng, n) if strs is None else strs
    rt = rng.integers(0, 1 << 45, n)
    v = rng.integers(-(1 << 40), 1 << 40, n)
    rows = [(s, int(a), int(b)) for s, a, b in zip(strs, rt, v)]
    n_events = max(1, n // 400) if n_events is None else n_events
    events = []
    for p, t in zip(np.sort(rng.integers(0, n + 1, n_events)).tolist(), rng.choice([2, 3, 4, 5], n_events).tolist()):
        vals = (int(rng.integers(-(1 << 62), 1 << 62)), -1, int(rng.integers(0, 1 << 40)), int(rng.integers(0, 100)))
        events.append((p, t, (vals[0] & 1,) if t == 5 else ((-1,) if t == 4 else vals)))
    ts = rng.integers(-(1 << 40), 1 << 40, n) if with_ts else None
    return R.encode_stream(UTV, rows, ts, events)


@pytest.mark.parametrize("n", [0, 1, 2, 60, 3000, 50_000])
def test_stream_sizes_vs_reference(n):
    """One chunk, two compose levels (> 26 chunks at S = 253) and three (> 676 chunks)."""
    rng = np.random.default_rng(n)
    sch = Sch(**UTV_S)
    dec = wire.WireDecoder(sch.schema)
    data, _ = utv_stream(rng, n, n_events=3 if n < 60 else None)
    chunks = len(data) // 4096 + 1
    assert {60: chunks <= 2, 3000: chunks > 26, 50_000: chunks > 676}.get(n, True)
    _, ref = check(dec, sch, data)
    check(dec, sch, data, device=True, ref=ref)
    dec.close()


@pytest.mark.parametrize("n", [60, 3000])
def test_tail_cuts(n):
    rng = np.random.default_rng(100 + n)
    sch = Sch(**UTV_S)
    dec = wire.WireDecoder(sch.schema)
    strs = words(rng, n)
    strs[-1] = "v" * 40                                            # a cut of 10 bytes lands in its variable part
    data, starts = utv_stream(rng, n, strs=strs)
    data = data[:starts[-1] + 4 + 5 + 32 + 40]                     # the stream ends with that record
    for cut in (1, 4, 5, 8, 10, 4095, 4096, 4097):
        if cut < len(data):
            _, ref = check(dec, sch, data[:len(data) - cut], device=cut in (8, 4096))
            assert ref["consumed"] < len(data) - cut or cut > 40
    dec.close()


def _lengths_rows(rng, n):
    lens = [0, 7, 8, 40, 208]                                      # 208: 5 + 32 + 208 = 245, the longest padded row
    return [("s" * lens[i % 5], int(rng.integers(0, 1 << 40)), i) for i in range(n)]


CONTENT = {
    "lengths": (UTV_S, _lengths_rows),
    "utf8": (UTV_S, lambda rng, n: [(WORDS[i % len(WORDS)], i * 7, -i) for i in range(n)]),
    "nulls": (UTV_S, lambda rng, n: [(s, i, i) for i, s in enumerate(words(rng, n, 0, 40, null_p=0.3))]),
    "two_strings": (dict(fields=["STRING", "LONG", "STRING", "INT"], key_field=-1, ts_field=1, cols=[3]),
                    lambda rng, n: [(a, i, b, int(rng.integers(-2**31, 2**31))) for i, (a, b) in
                                    enumerate(zip(words(rng, n, 0, 30, 0.1), words(rng, n, 0, 30, 0.1)))]),
    "payload_beside_long_key": (dict(fields=["LONG", "STRING", "LONG", "DOUBLE"], key_field=0, ts_field=2, cols=[3]),
                                lambda rng, n: [(None if i % 17 == 0 else int(rng.integers(-2**62, 2**62)), s, i,
                                                 None if i % 5 == 0 else float(rng.standard_normal()))
                                                for i, s in enumerate(words(rng, n, 0, 40, 0.1))]),
    "all_inline": (UTV_S, lambda rng, n: [(s, i, i) for i, s in enumerate(words(rng, n, 0, 7))]),
    "alternating": (UTV_S, lambda rng, n: [("ab" if i % 2 else "a-long-user-name-%06d" % i, i, i) for i in range(n)]),
}


@pytest.mark.parametrize("case", list(CONTENT))
@pytest.mark.parametrize("with_ts", [False, True])
def test_content_cases(case, with_ts):
    rng = np.random.default_rng(len(case))
    kw, gen = CONTENT[case]
    sch = Sch(**kw)
    dec = wire.WireDecoder(sch.schema)
    n = 2500
    rows = gen(rng, n)
    if case == "lengths" and with_ts:
        rows = [(s[:200], a, b) for s, a, b in rows]              # 13 + 32 + 200 = 245 with the timestamp
    events = [(int(p), 2, (int(p) * 1000,)) for p in np.sort(rng.integers(0, n + 1, 6))]
    data, _ = R.encode_stream(sch.fields, rows, rng.integers(0, 1 << 40, n) if with_ts else None, events)
    _, ref = check(dec, sch, data)
    check(dec, sch, data, device=True, ref=ref)
    if case == "nulls":
        assert 0 < ref["strings"][0][2].sum() < n
    if case == "payload_beside_long_key":
        assert ref["key_null"].sum() > 0 and ref["col_null"][0].sum() > 0
    dec.close()


def test_unpadded_rows_and_short_values_in_the_variable_part():
    """The row size need not be a multiple of 8 (L = 249 exactly is accepted), and a value of 7 bytes or fewer may sit in
    the variable part: the slot's own top bit decides."""
    sch = Sch(**UTV_S)
    dec = wire.WireDecoder(sch.schema)
    elems = []
    for i in range(400):
        ln = [212, 9, 3, 0, 33][i % 5]
        row = bytearray(R.row_bytes(UTV, ("q" * max(ln, 8), i, -i)))
        row[8:16] = struct.pack("<Q", (32 << 32) | ln)            # 3 and 0 bytes: in the variable part all the same
        elems.append(R.frame(bytes(row[:32 + ln])))               # no padding after the value
        if i % 5 == 0:
            assert len(elems[-1]) == 4 + 249
    data = b"".join(elems) + W.encode_event(2, (5,))
    _, ref = check(dec, sch, data)
    check(dec, sch, data, device=True, ref=ref)
    assert np.diff(ref["strings"][0][0])[:5].tolist() == [212, 9, 3, 0, 33]
    dec.close()


def test_false_chains_inside_strings():
    """Values made of whole encoded watermark and latency-marker elements, next to small integers: every element start
    inside a value begins a valid-looking chain, and where the value ends on the row's end (72 bytes, no padding) that
    chain runs on into the true one. Only the chain from offset 0 may be decoded."""
    rng = np.random.default_rng(7)
    sch = Sch(**UTV_S)
    dec = wire.WireDecoder(sch.schema)
    wm, lm = W.encode_event(2, (33,)), W.encode_event(3, (33, 0, 9, 1))
    vals = [wm * 3 + lm, wm + lm, lm + wm * 3, wm * 2]
    assert len(vals[0]) == 72 and len(vals[1]) == 46
    n = 4000
    rows = [(vals[int(rng.integers(0, 4))], 0x21, int(rng.integers(0, 64))) for _ in range(n)]
    data, _ = R.encode_stream(UTV, rows, None, [(100, 2, (0x2100000000,)), (2500, 3, (1, 2, 3, 4)), (2500, 2, (33,))])
    _, ref = check(dec, sch, data)
    assert ref["n_events"] == 3
    check(dec, sch, data, device=True, ref=ref)
    data2, _ = R.encode_stream(UTV, rows, np.full(n, 0x0000000902000000, np.int64), [(7, 4, (0,))])
    check(dec, sch, data2)
    dec.close()


def _bad_elements():
    fixed = 32
    long_row = R.row_bytes(UTV, ("x" * 216, 1, 2))                # L = 5 + 32 + 216 = 253 >= 250
    ok_row = bytearray(R.row_bytes(UTV, ("x" * 16, 1, 2)))

    def slot(v):
        r = bytearray(ok_row)
        r[8:16] = struct.pack("<Q", v)
        return R.frame(bytes(r))
    size_bad = bytearray(R.frame(bytes(ok_row)))
    size_bad[5 + 3] ^= 8                                          # the row's size int no longer equals L - 5
    return {
        "element_of_253_bytes": (R.frame(long_row), R.E_UNSUPPORTED),
        "element_of_250_bytes": (R.frame(long_row[:32 + 213]), R.E_UNSUPPORTED),
        "size_int_differs_from_L": (bytes(size_bad), R.E_CORRUPT),
        "slot_past_the_row": (slot((fixed << 32) | 17), R.E_CORRUPT),
        "slot_inside_the_fixed_part": (slot(((fixed - 8) << 32) | 8), R.E_CORRUPT),
        "inline_length_9": (slot((0x89 << 56) | 0x41), R.E_CORRUPT),
    }


@pytest.mark.parametrize("case", list(_bad_elements()))
def test_refusals_report_code_and_position(case):
    rng = np.random.default_rng(5)
    sch = Sch(**UTV_S)
    dec = wire.WireDecoder(sch.schema)
    good, starts = utv_stream(rng, 3000)
    elem, code = _bad_elements()[case]
    at = starts[2000]
    data = good[:at] + elem + good[at:]
    rc, ref = sch.ref(data)
    assert (rc, ref["err_pos"]) == (code, at)
    for device in (False, True):
        import torch
        x = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if device else data
        with pytest.raises(Exception) as ei:
            dec.decode(x)
        assert ei.value.code == code and ("byte %d" % at) in str(ei.value), str(ei.value)
        if code == R.E_UNSUPPORTED:
            assert "249" in str(ei.value)
        with pytest.raises(Exception) as ei:                        # no strings of a failed decode
            dec.strings_of(0, 0)
        assert ei.value.code == -8
        check(dec, sch, good)                                       # the decoder is usable afterwards
    dec.close()


def test_strings_of_state_and_argument_errors():
    sch = Sch(**UTV_S)
    dec = wire.WireDecoder(sch.schema)
    with pytest.raises(Exception) as ei:
        dec.strings_of(0, 0)
    assert ei.value.code == -8                                      # FWA_E_STATE: nothing decoded yet
    data, _ = utv_stream(np.random.default_rng(1), 10)
    got = dec.decode(data)
    for f in (1, 2, 3, -1):
        with pytest.raises(Exception) as ei:
            got.strings(f)
        assert ei.value.code == -1                                  # FWA_E_ARG: a LONG field / no field
    o, b, z = got.strings(0)
    assert o[0].item() == 0 and len(o) == 11 and len(z) == 10
    dec.close()


def test_fixed_length_schemas_decode_as_before():
    from test_wire_gpu import C5, T3, _check, _stream
    rng = np.random.default_rng(2)
    s = wire.make_schema(T3, key_field=0, ts_field=-1, cols=[1, 2])
    dec = wire.WireDecoder(s)
    data = _stream(rng, 40_000, n_events=50)
    _check(dec, s, data)
    _check(dec, s, data[:len(data) - 5], device=True)
    dec.close()
    s = wire.make_schema(C5, key_field=0, ts_field=1, cols=[2, 3], fmt="ROWDATA")
    dec = wire.WireDecoder(s)
    data = _stream(rng, 40_000, fields=C5, fmt="ROWDATA", with_ts=False, n_events=30, nulls=True)
    _check(dec, s, data)
    _check(dec, s, data, device=True)
    with pytest.raises(Exception) as ei:
        dec.strings_of(0, 0)
    assert ei.value.code == -1
    dec.close()


@pytest.mark.parametrize("two_part_key", [False, True])
def test_varchar_keyed_table_job_end_to_end(two_part_key):
    """(VARCHAR user, TIMESTAMP(3) rowtime, BIGINT v) rows in 32 KiB buffers -> NetworkInput(keydict) -> Table TUMBLE
    COUNT / SUM on FWA_KEY_GROUP_PREFIXED ids; fired rows back to their strings, per watermark, against the oracle on
    surrogate integer ids. The second case keys by (user, v) with NULL users."""
    from flink_amd.engine import WindowAggregator
    from flink_amd.keydict import KeyDictionary
    from oracle.oracle import Oracle
    rng = np.random.default_rng(21 + two_part_key)
    n = 40_000
    names = words(rng, 300, 0, 30) + [w for w in WORDS]
    names = sorted(set(names))
    pick = rng.integers(0, len(names), n)
    users = [names[i] for i in pick]
    if two_part_key:
        users = [None if rng.random() < 0.05 else u for u in users]
    ts = (np.arange(n) * 3 + rng.integers(0, 2000, n)).astype(np.int64)
    vals = rng.integers(0, 3, n).astype(np.int64) if two_part_key else rng.integers(0, 1 << 31, n).astype(np.int64)
    events = []
    for p in range(4000, n, 4000):
        wm = int(ts[:p].max()) - 1500
        events.append((p, 2, (wm,)))
        if p == 12_000:
            events.append((p, 4, (-1,)))                          # idle: the next watermark is ignored
        if p == 16_000:
            events.append((p, 4, (0,)))
        if p == 28_000:
            events.append((p, 2, (wm - 100_000,)))                # non-advancing
    data, _ = R.encode_stream(UTV, [(u, int(t), int(v)) for u, t, v in zip(users, ts, vals)], None, events)
    base = dict(window_kind="TUMBLE", semantics="TABLE", size_ms=5000, aggs=[("COUNT", 0), ("SUM_I64", 0)],
                key_kind=A.KEY_GROUP_PREFIXED, key_capacity=1 << 13)
    eng = WindowAggregator(A.make_config(**base))
    kd = KeyDictionary(["STRING", "BIGINT"] if two_part_key else ["STRING"], max_parallelism=128, capacity=1 << 14)
    parts = [("str", 0), ("col", 0)] if two_part_key else [("str", 0)]
    inp = wire.NetworkInput(wire.make_schema(UTV, key_field=-1, ts_field=1, cols=[2], fmt="ROWDATA"), eng,
                            keydict=kd, key_parts=parts)

    def decoded(r):
        if not len(r["key"]):
            return Counter()
        kc, kn = kd.decode(r["key"])
        keys = [tuple(None if z[i] else (c[i] if isinstance(c[i], str) else int(c[i])) for c, z in zip(kc, kn))
                for i in range(len(r["key"]))]
        return Counter(zip(keys, r["win_end"].tolist(), r["agg0"].tolist(), r["agg1"].tolist()))
    got = []
    for buf in W.split_buffers(data):
        got += [decoded(r) for r in inp.feed(buf)]
    got.append(decoded(eng.advance_watermark(A.LONG_MAX)))
    # the oracle on surrogate ids (key group 0: every key group is owned), valve semantics restated
    rows_key = [(u, int(v)) if two_part_key else (u,) for u, v in zip(users, vals)]
    sid = {}
    ids = np.array([sid.setdefault(k, len(sid)) for k in rows_key], np.int64)
    back = {v: k for k, v in sid.items()}
    o = Oracle(A.make_config(**base))

    def expected(r):
        return Counter(zip([back[k] for k in r["key"].tolist()], r["win_end"].tolist(), r["agg0"].tolist(),
                           r["agg1"].tolist()))
    exp, at, cur, idle, late = [], 0, A.LONG_MIN, False, 0
    for pos, tag, v in events + [(n, None, None)]:
        if pos > at:
            late += o.push(ids[at:pos], ts[at:pos], [vals[at:pos]])
            at = pos
        if tag == 2 and not idle and v[0] > cur:
            cur = v[0]
            exp.append(expected(o.advance_watermark(cur)))
        elif tag == 4:
            idle = v[0] == -1
    exp.append(expected(o.advance_watermark(A.LONG_MAX)))
    assert len(got) == len(exp) == 9
    for i, (g, e) in enumerate(zip(got, exp)):
        assert g == e, "watermark %d: only GPU %s, only oracle %s" % (i, list((g - e).items())[:3], list((e - g).items())[:3])
    assert sum(len(e) for e in exp) > 1000 and kd.size() == len(sid)
    assert inp.records_in == n and inp.late_dropped == late and inp.carry == b""
    inp.close()
    eng.close()
    kd.close()
