"""java.lang.String fields of TUPLE values on the GPU (FWA_FIELD_JSTRING) against the sequential reference of
tests/wire_jstring_ref.py, bit for bit: the decoder (columns, timestamps, events with positions, `consumed`, and per
JSTRING field the Arrow offsets, char bytes and NULL flags of fwa_wire_strings_of; host bytes and a device tensor), its
refusals with byte positions, fwa_jstring_hash against String.hashCode(), the encoder's bytes, the round trip, and a
String-keyed DataStream job from channel bytes to channel bytes."""
import functools
from collections import Counter

import numpy as np
import pytest

from flink_amd import _abi as A
from flink_amd import wire

import wire_jstring_ref as J

pytestmark = pytest.mark.gpu

SMILE = "\U0001F600"
SCHEMAS = {
    "sl": (["JSTRING", "LONG"], [1]),
    "lsid": (["LONG", "JSTRING", "INT", "DOUBLE"], [0, 2, 3]),
    "ssf": (["JSTRING", "JSTRING", "FLOAT"], [2]),
}
FIXED_BYTES = {"LONG": 8, "DOUBLE": 8, "INT": 4, "FLOAT": 4}


class Sch:
    def __init__(self, fields, cols, ts_field=-1):
        self.fields, self.cols, self.ts_field = fields, list(cols), ts_field
        self.schema = wire.make_schema(fields, key_field=-1, ts_field=ts_field, cols=cols)
        self.sf = [f for f, t in enumerate(fields) if t == "JSTRING"]
        fixed = sum(FIXED_BYTES.get(t, 0) for t in fields)
        # char bytes a value may have so that a record with a timestamp stays within the 249-byte ceiling
        self.budget = min(200, (249 - 9 - fixed - 2 * len(self.sf)) // len(self.sf))

    def ref(self, data):
        return J.decode(self.fields, data, self.ts_field, self.cols)


def check(dec, sch, data, device=False, ref=None):
    import torch
    if ref is None:
        rc, ref = sch.ref(data)
        assert rc == 0
    x = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if device and len(data) else data
    got = dec.decode(x)
    assert (got.n_records, got.n_events, got.consumed) == (ref["n_records"], ref["n_events"], ref["consumed"])
    assert got.key is None and got.key_null is None and got.col_null is None
    assert np.array_equal(got.ts.cpu().numpy(), ref["ts"])
    for a, b in zip(got.cols, ref["cols"]):
        assert np.array_equal(a.cpu().numpy().view(np.uint8), b.view(np.uint8))
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


def value(rng, nbytes, ascii_only=False):
    """A String whose char bytes number at most nbytes (exactly nbytes when ascii_only): 1-, 2- and 3-byte chars, lone
    surrogates among them."""
    if ascii_only:
        return bytes(rng.integers(0x20, 0x7F, nbytes, dtype=np.uint8)).decode()
    out, left = [], nbytes
    while left > 0:
        r = rng.random()
        if r < 0.7 or left < 2:
            out.append(chr(int(rng.integers(0, 0x80))))
            left -= 1
        elif r < 0.9 or left < 3:
            out.append(chr(int(rng.integers(0x80, 0x4000))))
            left -= 2
        else:
            out.append(chr(int(rng.integers(0x4000, 0x10000))))
            left -= 3
    return "".join(out)


def fixed_value(rng, t, i):
    if t == "LONG":
        return int(rng.integers(-(1 << 62), 1 << 62)) if i % 3 else i      # small values: runs of zero bytes
    if t == "INT":
        return int(rng.integers(-(1 << 31), 1 << 31))
    return float(np.float32(rng.standard_normal()))


def make_rows(rng, sch, n, lens, null_p=0.0, ascii_only=False):
    """lens(i, k): the char bytes of JSTRING field k of record i."""
    rows = []
    for i in range(n):
        r, k = [], 0
        for t in sch.fields:
            if t == "JSTRING":
                r.append(None if rng.random() < null_p else value(rng, min(sch.budget, lens(i, k)), ascii_only))
                k += 1
            else:
                r.append(fixed_value(rng, t, i))
        rows.append(tuple(r))
    return rows


def some_events(rng, n, k):
    events = []
    for p, t in zip(np.sort(rng.integers(0, n + 1, k)).tolist(), rng.choice([2, 3, 4, 5], k).tolist()):
        vals = (int(rng.integers(-(1 << 62), 1 << 62)), -1, int(rng.integers(0, 1 << 40)), int(rng.integers(0, 100)))
        events.append((p, t, (vals[0] & 1,) if t == 5 else ((-1,) if t == 4 else vals)))
    return events


def stream(rng, sch, n, lens, with_ts, n_events=None, **kw):
    rows = make_rows(rng, sch, n, lens, **kw)
    ts = rng.integers(-(1 << 40), 1 << 40, n) if with_ts else None
    ev = some_events(rng, n, max(1, n // 300) if n_events is None else n_events)
    data, starts = J.encode_stream(sch.fields, rows, ts, ev)
    return data, starts, rows


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097, 20000])
@pytest.mark.parametrize("with_ts", [False, True])
@pytest.mark.parametrize("name", list(SCHEMAS))
def test_decoder_sizes_vs_reference(name, with_ts, n):
    """Short values (0..12 char bytes): records of about 30 bytes; 20000 of them pass 64 chunks of 4 KiB, which adds the
    second composition level. Host bytes and a device tensor."""
    rng = np.random.default_rng(n + 7 * with_ts + len(name))
    sch = Sch(*SCHEMAS[name])
    dec = wire.WireDecoder(sch.schema)
    data, _, _ = stream(rng, sch, n, lambda i, k: int(rng.integers(0, 13)), with_ts, null_p=0.05)
    if n == 20000:
        assert len(data) // 4096 + 1 > 64
    _, ref = check(dec, sch, data)
    assert ref["n_records"] == n
    check(dec, sch, data, device=True, ref=ref)
    dec.close()


PATTERNS = {
    "one_length": lambda rng: (lambda i, k: 11),                    # the speculative walk
    "alternating": lambda rng: (lambda i, k: 3 if i % 2 else 40),   # the listed walk
    "random_0_200": lambda rng: (lambda i, k: int(rng.integers(0, 201))),
}


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("with_ts", [False, True])
@pytest.mark.parametrize("name", list(SCHEMAS))
def test_decoder_length_patterns(name, with_ts, pattern):
    rng = np.random.default_rng(len(pattern) + 3 * with_ts + len(name))
    sch = Sch(*SCHEMAS[name])
    dec = wire.WireDecoder(sch.schema)
    ascii_only = pattern != "random_0_200"                          # exact byte lengths for the first two
    data, _, _ = stream(rng, sch, 1500, PATTERNS[pattern](rng), with_ts, ascii_only=ascii_only,
                        null_p=0.1 if pattern == "random_0_200" else 0.0)
    _, ref = check(dec, sch, data)
    check(dec, sch, data, device=True, ref=ref)
    if pattern == "random_0_200":
        z = ref["strings"][sch.sf[0]][2]
        assert 0 < z.sum() < 1500
    dec.close()


def test_decoder_edge_values():
    """126 and 127 chars (a one- and a two-byte length), empty and null values, 2- and 3-byte chars, U+0000, lone
    surrogates, a surrogate pair; an element of exactly 249 bytes."""
    sch = Sch(["JSTRING", "LONG"], [1])
    dec = wire.WireDecoder(sch.schema)
    vals = ["a" * 126, "b" * 127, "", None, "é€", SMILE, "\uffff", "\x00", "\x00\x00", "\ud800", "x\udc00", "\u0080\u3fff\u4000",
            "c" * 238, "polygenelubricants", "Aa", "BB", "\x7f" * 5, "\u07ff" * 60, "\u4e2d" * 70]
    rows = [(v, i - 3) for i, v in enumerate(vals)] * 7
    for ts in (None, np.arange(len(rows)) * 5):
        if ts is not None:
            rows = [r for r in rows if r[0] is None or len(r[0]) < 230]     # "c" * 238 needs the room of the timestamp
        data, starts = J.encode_stream(sch.fields, rows, ts, [(2, 2, (77,)), (len(rows), 4, (0,))])
        _, ref = check(dec, sch, data)
        check(dec, sch, data, device=True, ref=ref)
        o, b, z = ref["strings"][0]
        assert [None if z[i] else J.text_of(bytes(b[o[i]:o[i + 1]])) for i in range(len(rows))] == [r[0] for r in rows]
    fit = J.frame(J.value_bytes(sch.fields, ("c" * 238, 1)))        # tag + 2 + 238 + 8 = 249
    assert len(fit) == 4 + 249
    _, ref = check(dec, sch, fit * 40)
    assert ref["n_records"] == 40
    ts_fit = J.frame(J.value_bytes(sch.fields, ("d" * 230, 1)), ts=5)   # tag + 8 + 2 + 230 + 8 = 249
    assert len(ts_fit) == 4 + 249
    check(dec, sch, (fit + ts_fit) * 20, device=True)
    dec.close()


def test_ts_field_and_unread_fields():
    """The rowtime taken from a LONG field behind a String, a column read twice, a field read by no column."""
    rng = np.random.default_rng(3)
    sch = Sch(["INT", "JSTRING", "LONG", "JSTRING", "DOUBLE"], [2, 0, 2], ts_field=2)
    dec = wire.WireDecoder(sch.schema)
    data, _, _ = stream(rng, sch, 700, lambda i, k: int(rng.integers(0, 60)), True)
    _, ref = check(dec, sch, data)
    assert np.array_equal(ref["ts"], ref["cols"][0].view(np.int64))
    dec.close()


def decode_in_pieces(sch, data, cuts):
    """Feed data cut at `cuts` to one decoder, carrying partial elements over; the concatenated result."""
    dec = wire.WireDecoder(sch.schema)
    ts, cols, events = [], [[] for _ in sch.cols], []
    strs = {f: ([], [], []) for f in sch.sf}
    carry, at, nrec = b"", 0, 0
    for c in sorted(set(cuts) | {len(data)}):
        buf = carry + data[at:c]
        at = c
        got = dec.decode(buf)
        ts.append(got.ts.cpu().numpy().copy())
        for j in range(len(sch.cols)):
            cols[j].append(got.cols[j].cpu().numpy().copy())
        for f in sch.sf:
            o, b, z = got.strings(f)
            o = o.cpu().numpy()
            strs[f][0].append(np.diff(o))
            strs[f][1].append(b.cpu().numpy()[:o[-1]].copy())
            strs[f][2].append(z.cpu().numpy().copy())
        events += [(nrec + p, t, tuple(v)) for p, t, v in zip(got.evt_pos.tolist(), got.evt_tag.tolist(), got.evt_val.tolist())]
        nrec += got.n_records
        carry = buf[got.consumed:]
    dec.close()
    assert carry == b""
    return dict(ts=np.concatenate(ts), cols=[np.concatenate(c) for c in cols], events=events, n=nrec,
                strs={f: tuple(np.concatenate(x) for x in v) for f, v in strs.items()})


def same_as_whole(sch, data, pieces):
    rc, ref = sch.ref(data)
    assert rc == 0 and ref["consumed"] == len(data) and pieces["n"] == ref["n_records"]
    assert np.array_equal(pieces["ts"], ref["ts"])
    for a, b in zip(pieces["cols"], ref["cols"]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert pieces["events"] == [(p, t, tuple(v)) for p, t, v in zip(ref["evt_pos"].tolist(), ref["evt_tag"].tolist(), ref["evt_val"].tolist())]
    for f in sch.sf:
        ro, rb, rz = ref["strings"][f]
        assert np.array_equal(pieces["strs"][f][0], np.diff(ro)) and np.array_equal(pieces["strs"][f][1], rb)
        assert np.array_equal(pieces["strs"][f][2], rz)
    return ref


def test_stream_fed_in_pieces():
    """Cuts at arbitrary byte positions, one inside a two-byte length varint and one inside a 3-byte char among them."""
    rng = np.random.default_rng(12)
    sch = Sch(["JSTRING", "LONG"], [1])
    rows = make_rows(rng, sch, 1200, lambda i, k: int(rng.integers(0, 80)))
    rows[400] = ("v" * 130, 1)                                      # len + 1 = 131: 83 01
    rows[800] = ("\u4e2d\u6587", 2)
    ts = rng.integers(0, 1 << 40, len(rows))
    data, starts = J.encode_stream(sch.fields, rows, ts, some_events(rng, len(rows), 9))
    in_varint = starts[400] + 4 + 9 + 1
    in_char = starts[800] + 4 + 9 + 1 + 2
    assert data[in_varint - 1:in_varint + 1] == b"\x83\x01" and data[in_char - 2] >= 0x80 and data[in_char - 1] >= 0x80
    cuts = [in_varint, in_char, starts[5] + 2, starts[6] + 4, starts[7] + 5, starts[900] + 12] + rng.integers(1, len(data), 6).tolist()
    same_as_whole(sch, data, decode_in_pieces(sch, data, cuts))


@pytest.mark.parametrize("name", ["sl", "ls"])
def test_false_chains_inside_values(name):
    """Values made of U+0000..U+007F chars whose bytes spell whole valid-looking elements (records of this schema,
    watermarks, latency markers; 00 00 00 0d 00 ... among them) at every phase of the chunk grid; with the String as the
    last field a false chain runs on into the true one. Only the chain from byte 0 may be decoded."""
    rng = np.random.default_rng(7 + len(name))
    fields = ["JSTRING", "LONG"] if name == "sl" else ["LONG", "JSTRING"]
    sch = Sch(fields, [fields.index("LONG")])
    dec = wire.WireDecoder(sch.schema)
    small = ("ab", 5) if name == "sl" else (5, "ab")
    fakes = [J.frame(J.value_bytes(fields, small), ts=7), J.frame(J.value_bytes(fields, small)),
             J.encode_event(2, (33,)), J.encode_event(3, (33, 0, 9, 1)), bytes.fromhex("00 00 00 0d 00") + bytes(12)]
    assert all(max(f) < 0x80 for f in fakes)
    vals = [fakes[0] * 3, fakes[1] * 5 + fakes[2], fakes[2] * 4 + fakes[3], fakes[4] * 3 + fakes[0], fakes[3] + fakes[1] * 2]
    n = 3000
    rows = []
    for i in range(n):
        v = ("x" * int(rng.integers(0, 4)) + vals[int(rng.integers(0, len(vals)))].decode("latin-1"))
        rows.append((v, 0x21) if name == "sl" else (int(rng.integers(0, 64)), v))
    data, _ = J.encode_stream(fields, rows, None, [(100, 2, (0x2100000000,)), (2000, 3, (1, 2, 3, 4)), (2000, 2, (33,))])
    _, ref = check(dec, sch, data)
    assert ref["n_events"] == 3 and ref["n_records"] == n
    check(dec, sch, data, device=True, ref=ref)
    data2, _ = J.encode_stream(fields, rows[:1500], np.full(1500, 0x0000000d00000000, np.int64), [(7, 4, (0,))])
    check(dec, sch, data2)
    dec.close()


BAD = {
    "length_claims_more_chars": (b"\x09ab", J.E_CORRUPT),
    "length_past_the_element": (b"\x7fab", J.E_CORRUPT),
    "fewer_chars_than_the_element_holds": (b"\x02ab", J.E_CORRUPT),
    "four_group_char": (b"\x02\x80\x80\x80\x01", J.E_CORRUPT),
    "third_group_of_04": (b"\x02\x80\x80\x04", J.E_CORRUPT),
    "char_80_00": (b"\x02\x80\x00", J.E_CORRUPT),
    "length_80_00": (b"\x80\x00", J.E_CORRUPT),
    "element_of_250_bytes": ("c" * 239, J.E_UNSUPPORTED),
}


@pytest.mark.parametrize("case", list(BAD))
def test_refusals_report_code_and_position(case):
    import torch
    rng = np.random.default_rng(5)
    sch = Sch(["JSTRING", "LONG"], [1])
    dec = wire.WireDecoder(sch.schema)
    good, starts, _ = stream(rng, sch, 2000, lambda i, k: int(rng.integers(0, 40)), False)
    raw, code = BAD[case]
    elem = J.frame(J.value_bytes(sch.fields, (raw, 1)))
    if code == J.E_UNSUPPORTED:
        assert len(elem) == 4 + 250
    at = starts[1300]
    data = good[:at] + elem + good[at:]
    rc, ref = sch.ref(data)
    assert (rc, ref["err_pos"]) == (code, at)
    for device in (False, True):
        x = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if device else data
        with pytest.raises(Exception) as ei:
            dec.decode(x)
        assert ei.value.code == code and ("byte %d" % at) in str(ei.value), str(ei.value)
        if code == J.E_UNSUPPORTED:
            assert "249" in str(ei.value)
        with pytest.raises(Exception) as ei:                        # no strings of a failed decode
            dec.strings_of(0, 0)
        assert ei.value.code == -8
    check(dec, sch, good)                                           # the decoder is usable afterwards
    dec.close()


# ---- String.hashCode() ----
def arrow(vals):
    """Arrow offsets / char bytes / NULL flags of a list of str-or-None (a NULL keeps garbage bytes in the column)."""
    parts = [b"NULL-GARBAGE"[:1 + i % 12] if v is None else J.char_bytes(v) for i, v in enumerate(vals)]
    offs = np.zeros(len(vals) + 1, np.int32)
    offs[1:] = np.cumsum([len(p) for p in parts])
    data = np.frombuffer(b"".join(parts) or b"\0", np.uint8).copy()
    return offs, data, np.array([v is None for v in vals], np.uint8)


def gpu_hash(vals, skip=0, with_nulls=False):
    import torch
    o, b, z = arrow(vals)
    got = wire.jstring_hash(torch.from_numpy(o).cuda()[skip:], torch.from_numpy(b).cuda(),
                            torch.from_numpy(z).cuda()[skip:] if with_nulls else None)
    assert got.dtype == torch.int32 and got.is_cuda
    return got.cpu().numpy().tolist()


TABLE = ["key1", "", "é€", SMILE, "\uffff", "a" * 127, "polygenelubricants", "Aa", "BB"]


def test_jstring_hash_table_and_lengths():
    assert gpu_hash(TABLE) == [3288498, 0, 15587, 1772899, 65535, -1374877567, -2147483648, 2112, 2112]
    rng = np.random.default_rng(2)
    vals = [value(rng, ln) for ln in (0, 1, 63, 64, 65, 200)] + [value(rng, ln, True) for ln in (0, 1, 63, 64, 65, 200)]
    vals += ["\u4e2d" * 3000, "z" * 9000]                           # values longer than one staged tile
    assert gpu_hash(vals) == [J.java_hash(v) for v in vals]


@pytest.mark.parametrize("n", [0, 1, 65, 4097])
def test_jstring_hash_sizes_offsets_nulls(n):
    rng = np.random.default_rng(40 + n)
    vals = [None if rng.random() < 0.1 else value(rng, int(rng.integers(0, 50))) for _ in range(n)]
    exp = [0 if v is None else J.java_hash(v) for v in vals]
    plain = [v or "" for v in vals]
    assert gpu_hash(plain) == [J.java_hash(v) for v in plain]
    assert gpu_hash(vals, with_nulls=True) == exp
    if n > 5:
        assert gpu_hash(vals, skip=5, with_nulls=True) == exp[5:]   # offsets that do not start at 0
        assert gpu_hash(plain, skip=n - 1) == [J.java_hash(plain[-1])]


# ---- the encoder ----
WM = (2, (1_700_000_000_123,))
ENC_SCHEMAS = {
    "key_agg": (["JSTRING", "LONG"], [("JSTRING", ("KEYCOL", 0, "STRING")), ("LONG", ("AGG", 0, "SUM_I64"))]),
    "agg_key_int_end": (["LONG", "JSTRING", "INT", "LONG"],
                        [("LONG", ("AGG", 0, "SUM_I64")), ("JSTRING", ("KEYCOL", 0, "STRING")),
                         ("INT", ("AGG", 1, "MIN_I32")), ("LONG", "WIN_END")]),
}


def make_out(n, win_end, aggs, nulls=(), device=True):
    import torch
    keep = []

    def ptr(x):
        x = np.array(x)
        if device:
            t = torch.from_numpy(x).cuda()
            keep.append(t)
            return t.data_ptr() or None
        keep.append(x)
        return x.ctypes.data
    out = A.Out()
    out.n_rows, out.on_device, out.num_aggs = n, 1 if device else 0, len(aggs)
    out.win_end = ptr(win_end)
    for j, a in enumerate(aggs):
        out.agg[j] = ptr(a)
        if j < len(nulls):
            out.agg_null[j] = ptr(nulls[j])
    return out, keep


@functools.lru_cache(maxsize=None)
def enc_case(name, n, with_ts, special=False):
    """Columns and the reference bytes (computed once per case, shared, never changed)."""
    rng = np.random.default_rng(500 + n + len(name) + with_ts)
    if special:                                                    # the length prefix grows to three bytes; one direct tile
        keys = [value(rng, int(rng.integers(0, 30))) for _ in range(n)]
        keys[3], keys[70], keys[n // 2] = "x" * 16382, "é" * 16383, value(rng, 70_000)
    else:
        keys = [value(rng, int(rng.integers(0, 301))) for _ in range(n)]
    a0 = rng.integers(-(1 << 62), 1 << 62, n)
    a1 = rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32)
    we = rng.integers(0, 1 << 44, n)
    fields, schema = ENC_SCHEMAS[name]
    rows = [(keys[i], int(a0[i])) if name == "key_agg" else (int(a0[i]), keys[i], int(a1[i]), int(we[i])) for i in range(n)]
    ref, starts = J.encode_stream(fields, rows, we - 1 if with_ts else None, [(n, WM[0], WM[1])])
    return dict(schema=schema, fields=fields, keys=keys, aggs=[a0, a1], we=we, ref=ref, starts=starts, rows=rows)


def encode(case, n, with_ts, device=True, host=False, key_nulls=False, events=(WM,)):
    import torch
    enc = wire.WireEncoder(wire.make_out_schema(case["schema"], record_ts="WIN_TIME" if with_ts else None))
    out, keep = make_out(n, case["we"], case["aggs"], device=device)
    o, b, z = arrow(case["keys"])
    cols = [(torch.from_numpy(o).cuda(), torch.from_numpy(b).cuda())]
    try:
        got = enc.encode(out, keycols=(cols, [torch.from_numpy(z).cuda()] if key_nulls else None), events=events, host=host)
        got = got if host else bytes(got.cpu().numpy())
        st = enc.stats()
        assert (st.calls, st.rows_in, st.bytes_out) == (1, n, len(got))
    finally:
        enc.close()
    return got


def same(got, ref):
    if got == ref:
        return
    assert len(got) == len(ref), "%d bytes, reference %d" % (len(got), len(ref))
    at = int(np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(ref, np.uint8))[0])
    raise AssertionError("first difference at byte %d: %s, reference %s" % (at, got[at:at + 16].hex(), ref[at:at + 16].hex()))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
@pytest.mark.parametrize("with_ts", [False, True])
@pytest.mark.parametrize("name", list(ENC_SCHEMAS))
def test_encoder_bytes_vs_reference(name, with_ts, n):
    """Value lengths 0..300 char bytes: runs of 64 rows that fit the LDS tile and runs that do not."""
    case = enc_case(name, n, with_ts)
    same(encode(case, n, with_ts), case["ref"])


@pytest.mark.parametrize("name", list(ENC_SCHEMAS))
def test_encoder_long_values(name):
    """16382 and 16383 chars, where the length prefix grows to three bytes, and one 70000-byte value: direct tiles."""
    case = enc_case(name, 200, True, special=True)
    assert case["ref"].count(b"\xff\x7f" + b"x" * 8) == 1 and case["ref"].count(b"\x80\x80\x01\xe9\x01") == 1
    same(encode(case, 200, True), case["ref"])


def test_encoder_events_host_rows_host_bytes():
    events = [(3, (1_700_000_000_000, -5, 1 << 62, 7)), (4, (-1,)), (2, (-(1 << 63),)), (5, (1,))]
    ev = b"".join(J.encode_event(t, v) for t, v in events)
    for n in (65, 4097):
        case = enc_case("agg_key_int_end", n, True)
        same(encode(case, n, True, events=[WM] + events), case["ref"] + ev)
        same(encode(case, n, True, device=False, host=True), case["ref"])
        same(encode(case, n, True, device=False, host=False), case["ref"])
        same(encode(case, n, True, device=True, host=True), case["ref"])
    assert encode(enc_case("key_agg", 0, False), 0, False, events=events) == ev


def test_encoder_refusals():
    def refused(fields, fmt, code, text):
        with pytest.raises(Exception) as ei:
            wire.WireEncoder(wire.make_out_schema(fields, fmt=fmt))
        assert ei.value.code == code and text in str(ei.value), str(ei.value)
    key = ("JSTRING", ("KEYCOL", 0, "STRING"))
    refused([key, ("LONG", "KEY")], "ROWDATA", -1, "TUPLE values only")
    refused([("JSTRING", "KEY")], "TUPLE", -1, "an int64 source cannot be written as JSTRING")
    refused([("JSTRING", ("AGG", 0, "SUM_F64"))], "TUPLE", -1, "a double source cannot be written as JSTRING")
    refused([("JSTRING", ("KEYCOL", 0, "BIGINT"))], "TUPLE", -1, "an int64 source cannot be written as JSTRING")
    refused([("LONG", "KEY"), ("STRING", ("KEYCOL", 0, "STRING"))], "TUPLE", -1, "STRING fields are written in ROWDATA rows only")
    case = enc_case("key_agg", 65, False)
    with pytest.raises(Exception) as ei:                            # NULL flags on the source
        encode(case, 65, False, key_nulls=True)
    assert ei.value.code == -1 and "TupleSerializer cannot write null fields" in str(ei.value)
    enc = wire.WireEncoder(wire.make_out_schema(case["schema"]))
    out, keep = make_out(65, case["we"], case["aggs"])
    with pytest.raises(Exception) as ei:
        enc.encode(out)
    assert ei.value.code == -1 and "keycols" in str(ei.value)
    enc.close()


@pytest.mark.parametrize("name", list(ENC_SCHEMAS))
def test_round_trip_through_the_decoder(name):
    """Encoder output whose elements stay within 249 bytes, fed to the GPU decoder in arbitrary cuts."""
    import torch
    rng = np.random.default_rng(77)
    n = 3000
    fields, schema = ENC_SCHEMAS[name]
    keys = [value(rng, int(rng.integers(0, 180))) for _ in range(n)]
    a0 = rng.integers(-(1 << 62), 1 << 62, n)
    a1 = rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32)
    we = rng.integers(0, 1 << 44, n)
    enc = wire.WireEncoder(wire.make_out_schema(schema, record_ts="WIN_TIME"))
    out, keep = make_out(n, we, [a0, a1])
    o, b, _ = arrow(keys)
    data = bytes(enc.encode(out, keycols=([(torch.from_numpy(o).cuda(), torch.from_numpy(b).cuda())], None),
                            events=[WM]).cpu().numpy())
    enc.close()
    sch = Sch(fields, [f for f, t in enumerate(fields) if t != "JSTRING"])
    res = decode_in_pieces(sch, data, rng.integers(1, len(data), 7).tolist())
    sf = sch.sf[0]
    assert res["n"] == n and np.array_equal(res["ts"], we - 1) and res["events"] == [(n, 2, (WM[1][0], 0, 0, 0))]
    assert np.array_equal(res["strs"][sf][0], np.diff(o)) and np.array_equal(res["strs"][sf][1], b[:o[-1]])
    assert not res["strs"][sf][2].any()
    if name == "key_agg":
        assert np.array_equal(res["cols"][0].view(np.int64), a0)
    else:
        assert np.array_equal(res["cols"][0].view(np.int64), a0) and np.array_equal(res["cols"][1].view(np.int64), a1.astype(np.int64))
        assert np.array_equal(res["cols"][2].view(np.int64), we)


# ---- a String-keyed DataStream job, bytes to bytes ----
JOB = dict(window_kind="TUMBLE", semantics="DATASTREAM", size_ms=2000, aggs=[("COUNT", 0), ("SUM_I64", 0)],
           key_kind=A.KEY_PREHASHED, max_parallelism=128, key_capacity=1 << 11)


@functools.lru_cache(maxsize=None)
def job_input():
    rng = np.random.default_rng(31)
    n = 5000
    names = ["Aa", "BB", "polygenelubricants", "é€", SMILE, "\u4e2d\u6587-key", "", "key1", "key2"]
    # (through the char bytes and back: a high and a low surrogate that came to stand side by side are one code point)
    names += sorted({J.text_of(J.char_bytes(value(rng, int(rng.integers(1, 30))))) for _ in range(300)} - set(names))[:291]
    keys = [names[i] for i in rng.integers(0, len(names), n)]
    ts = (np.arange(n) * 3 + rng.integers(0, 1500, n)).astype(np.int64)
    v = rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)
    events = [(p, 2, (int(ts[:p].max()) - 300,)) for p in range(500, n, 500)]
    data, _ = J.encode_stream(["JSTRING", "LONG"], list(zip(keys, v.tolist())), ts, events)
    return dict(n=n, names=names, keys=keys, ts=ts, v=v, events=events, data=data)


class Piped:
    """The handle as NetworkInput sees it, its watermark step routed through the NetworkOutput behind it."""

    def __init__(self, eng, net):
        self.cfg, self.push, self.net = eng.cfg, eng.push, net

    def advance_watermark(self, wm):
        return bytes(self.net.emit(wm).cpu().numpy())


def test_string_keyed_job_from_bytes_to_bytes():
    """Tuple2<String, Long> records with timestamps and watermarks -> NetworkInput(key_string=0) -> DATASTREAM TUMBLE
    COUNT + SUM on a PREHASHED handle -> NetworkOutput writing Tuple3<String, Long, Long> under the record timestamp
    win_end - 1. Per watermark the bytes, decoded by the reference, equal as a multiset the oracle's rows (host-assigned
    ids, key_hash = java_hash); late drops are equal."""
    from flink_amd.engine import WindowAggregator
    from flink_amd.keydict import KeyDictionary
    from oracle.oracle import Oracle
    job = job_input()
    n, keys, ts, v = job["n"], job["keys"], job["ts"], job["v"]
    eng = WindowAggregator(A.make_config(output_on_device=1, **JOB))
    kd = KeyDictionary(["STRING"], max_parallelism=128, capacity=1 << 11)
    out_fields = ["JSTRING", "LONG", "LONG"]
    net = wire.NetworkOutput(wire.make_out_schema([("JSTRING", ("KEYCOL", 0, "STRING")), ("LONG", ("AGG", 0, "COUNT")),
                                                   ("LONG", ("AGG", 1, "SUM_I64"))], record_ts="WIN_TIME"), eng, keydict=kd)
    inp = wire.NetworkInput(wire.make_schema(["JSTRING", "LONG"], key_field=-1, cols=[1]), Piped(eng, net),
                            keydict=kd, key_string=0)
    got = []
    for at in range(0, len(job["data"]), 32 * 1024):
        got += inp.feed(job["data"][at:at + 32 * 1024])
    got.append(bytes(net.emit(A.LONG_MAX).cpu().numpy()))
    # the oracle on host-assigned ids beside String.hashCode()
    sid = {}
    ids = np.array([sid.setdefault(k, len(sid)) for k in keys], np.int64)
    hs = np.array([J.java_hash(k) for k in keys], np.int32)
    back = {i: k for k, i in sid.items()}
    o = Oracle(A.make_config(**JOB))
    exp, at, late, wms = [], 0, 0, []
    for pos, _, val in job["events"] + [(n, 2, (A.LONG_MAX,))]:
        late += o.push(ids[at:pos], ts[at:pos], [v[at:pos]], key_hash=hs[at:pos])
        at = pos
        r = o.advance_watermark(val[0])
        wms.append(val[0])
        exp.append(Counter(zip([back[k] for k in r["key"].tolist()], r["agg0"].tolist(), r["agg1"].tolist(),
                               (r["win_end"] - 1).tolist())))
    assert len(got) == len(exp) == 10
    for data, e, wm in zip(got, exp, wms):
        assert data[-13:] == J.encode_event(2, (wm,))
        rc, d = J.decode(out_fields, data, cols=[1, 2])
        assert rc == 0 and d["consumed"] == len(data) and d["n_events"] == 1 and d["evt_pos"].tolist() == [sum(e.values())]
        so, sb, sz = d["strings"][0]
        assert not sz.any()
        rows = Counter((J.text_of(bytes(sb[so[i]:so[i + 1]])), int(d["cols"][0].view(np.int64)[i]),
                        int(d["cols"][1].view(np.int64)[i]), int(d["ts"][i])) for i in range(d["n_records"]))
        assert rows == e, "watermark %d: only GPU %s, only oracle %s" % (wm, list((rows - e).items())[:3], list((e - rows).items())[:3])
    assert sum(sum(e.values()) for e in exp) > 500 and kd.size() == len(sid) == len(job["names"])
    assert inp.records_in == n and inp.late_dropped == late and late > 0 and inp.carry == b""
    assert net.rows_out == sum(sum(e.values()) for e in exp)
    for x in (inp, net, eng, kd):
        x.close()


def murmur_key_group(code, max_parallelism):
    """KeyGroupRangeAssignment.computeKeyGroupForKeyHash: MathUtils.murmurHash(key.hashCode()) % maxParallelism."""
    m = 0xFFFFFFFF
    rotl = lambda x, r: ((x << r) | (x >> (32 - r))) & m
    c = (code & m) * 0xCC9E2D51 & m
    c = rotl(c, 15) * 0x1B873593 & m
    c = (rotl(c, 13) * 5 + 0xE6546B64) & m
    c ^= 4
    c ^= c >> 16
    c = c * 0x85EBCA6B & m
    c ^= c >> 13
    c = c * 0xC2B2AE35 & m
    c ^= c >> 16
    c = c - (1 << 32) if c >> 31 else c
    c = c if c >= 0 else (-c if c != -(1 << 31) else 0)
    return c % max_parallelism


def test_key_group_check_reads_the_device_hash():
    """A handle owning key groups 0..63 of 128 accepts exactly the records whose murmur(String.hashCode()) falls there;
    every other record is FWA_E_KEYGROUP. A null key is refused like KeyGroupRangeAssignment.assignToKeyGroup does."""
    from flink_amd import engine
    from flink_amd.keydict import KeyDictionary
    job = job_input()
    names = job["names"]
    hs = np.array([J.java_hash(k) for k in names], np.int32)
    kg, _ = engine.key_groups(np.arange(len(names), dtype=np.int64), 128, 1, key_kind=A.KEY_PREHASHED, key_hash=hs)
    kg = np.asarray(kg)
    assert kg.tolist() == [murmur_key_group(int(h), 128) for h in hs]
    assert 0 < (kg <= 63).sum() < len(names)
    assert kg[names.index("Aa")] == kg[names.index("BB")]           # one hash, two keys
    eng = engine.WindowAggregator(A.make_config(kg_start=0, kg_end=63, **JOB))
    kd = KeyDictionary(["STRING"], max_parallelism=128, capacity=1 << 11)
    schema = wire.make_schema(["JSTRING", "LONG"], key_field=-1, cols=[1])
    inp = wire.NetworkInput(schema, eng, keydict=kd, key_string=0)
    accepted = 0
    for i, name in enumerate(names):
        data, _ = J.encode_stream(["JSTRING", "LONG"], [(name, 1), (name, 2)], [10, 20])
        if kg[i] <= 63:
            inp.feed(data)
            accepted += 2
        else:
            with pytest.raises(Exception) as ei:
                inp.feed(data)
            assert A.STATUS[ei.value.code] == "E_KEYGROUP", (name, str(ei.value))
        assert inp.records_in == accepted
    own = [k for k, g in zip(names, kg) if g <= 63]
    data, _ = J.encode_stream(["JSTRING", "LONG"], [(k, 3) for k in own], [30] * len(own))
    inp.feed(data)                                                 # a run of owned keys only is taken whole
    r = eng.advance_watermark(A.LONG_MAX)
    assert len(r["key"]) == len(own) and sorted(r["agg0"].tolist()) == [3] * len(own)
    data, _ = J.encode_stream(["JSTRING", "LONG"], [(own[0], 1), (None, 2)], [10, 20])
    with pytest.raises(Exception) as ei:
        inp.feed(data)
    assert ei.value.code == -1 and "Assigned key must not be null" in str(ei.value)
    for x in (inp, eng, kd):
        x.close()
