"""DECIMAL(38) on the wire, on the GPU (FWA_FIELD_DECIMAL): fwa_wire_encode and fwa_wire_decode against the pure-Python
reference tests/wire_decimal_ref.py, byte for byte / bit for bit and in order. The encoder's columns are hand-made tensors
wrapped in an fwa_out, so nothing but the encoder stands between them and the bytes; the decoder's streams are
reference-written, with both NULL forms, non-minimal lengths, STRING fields beside the DECIMALs and events in between.
Then corrupt slots, the round trip, the schema checks on a machine with a device, and a Table job with DECIMAL(38)
aggregates from channel bytes to channel bytes."""
import ctypes as C
import functools
from collections import Counter

import numpy as np
import pytest

from flink_amd import _abi as A
from flink_amd import wire
from oracle import wire_encode as W

import test_wire_decimal_cpu as CPU
import wire_decimal_ref as D

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 4097]
WM = (2, (1_700_000_000_123,))
NULL_MODES = ["quarter", "all", "none", "noflags"]
OUT_FIELDS = ["LONG", "DECIMAL", "LONG", "DECIMAL", "LONG", "LONG"]
OUT_SCHEMA = [("LONG", "KEY"), ("DECIMAL", ("AGG", 0, "SUM_DEC128")), ("LONG", ("AGG", 1, "COUNT")),
              ("DECIMAL", ("AGG", 2, "AVG_DEC")), ("LONG", "WIN_START"), ("LONG", "WIN_END")]


def decimals(rng, n, shift=0):
    """n unscaled values: the boundary values first (rotated by `shift`), then random 128-bit values of every length."""
    vals = D.boundary_values()
    vals = vals[shift % len(vals):] + vals[:shift % len(vals)]
    out = vals[:n]
    while len(out) < n:
        v = int.from_bytes(rng.bytes(16), "little", signed=True)
        out.append(v >> int(rng.integers(0, 128)))
    return out


def make_out(n, key=None, win_start=None, win_end=None, aggs=(), nulls=(), device=True):
    """An fwa_out over numpy columns (copied to the device unless device=False) and the objects it points into."""
    import torch
    keep = []

    def ptr(x):
        if x is None:
            return None
        x = np.array(x)                                            # a contiguous copy: the shared columns stay read-only
        if device:
            t = torch.from_numpy(x.view(np.uint8) if x.dtype == bool else x).cuda()
            keep.append(t)
            return t.data_ptr() or None
        keep.append(x)
        return x.ctypes.data
    out = A.Out()
    out.n_rows, out.on_device, out.num_aggs = n, 1 if device else 0, len(aggs)
    out.key, out.win_start, out.win_end = ptr(key), ptr(win_start), ptr(win_end)
    for j, a in enumerate(aggs):
        out.agg[j] = ptr(a)
        out.agg_null[j] = ptr(nulls[j]) if j < len(nulls) else None
    return out, keep


def _flags(mode, rng, n):
    if mode == "quarter":
        return rng.random(n) < 0.25
    return np.ones(n, bool) if mode == "all" else np.zeros(n, bool)


@functools.lru_cache(maxsize=None)
def out_case(n, mode):
    """Columns and reference bytes of the encoder's case 1 (computed once per size and NULL mode, shared, never changed)."""
    rng = np.random.default_rng(5000 + n)
    key = rng.integers(-(1 << 63), 1 << 63, n)
    ws = rng.integers(-(1 << 40), 1 << 45, n)
    we = ws + 1000
    d0, d2 = decimals(rng, n), decimals(rng, n, shift=17)
    cnt = rng.integers(1, 1 << 40, n)
    z0, z2 = _flags(mode, rng, n), _flags(mode, rng, n)
    rows = [(int(key[i]), None if z0[i] else d0[i], int(cnt[i]), None if z2[i] else d2[i], int(ws[i]), int(we[i]))
            for i in range(n)]
    ref, starts = D.encode_stream(OUT_FIELDS, rows, None, [(n, WM[0], WM[1])])
    assert len(ref) == (4 + 1 + 4 + 8 + 48) * n + 16 * int((~z0).sum() + (~z2).sum()) + 13
    aggs = [A.dec128_column(d0), cnt, A.dec128_column(d2)]         # non-zero garbage stays under the NULL flags
    nulls = [None, None, None] if mode == "noflags" else [z0, None, z2]
    for v in [key, ws, we] + aggs:
        v.setflags(write=False)
    return dict(key=key, ws=ws, we=we, aggs=aggs, nulls=nulls, d=[d0, d2], z=[z0, z2], rows=rows, ref=ref)


def _encode(case, n, schema=OUT_SCHEMA, device=True, host=False, events=(WM,), keycols=None):
    enc = wire.WireEncoder(wire.make_out_schema(schema, fmt="ROWDATA"))
    out, keep = make_out(n, case["key"], case["ws"], case["we"], case["aggs"], case["nulls"], device=device)
    got = enc.encode(out, keycols=keycols, events=events, host=host)
    got = got if host else bytes(got.cpu().numpy())
    st = enc.stats()
    assert (st.calls, st.rows_in, st.bytes_out) == (1, n, len(got))
    enc.close()
    return got


def _same(got, ref):
    if got == ref:
        return
    assert len(got) == len(ref), "%d bytes, reference %d" % (len(got), len(ref))
    at = int(np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(ref, np.uint8))[0])
    raise AssertionError("first difference at byte %d: %s, reference %s" % (at, got[at:at + 16].hex(), ref[at:at + 16].hex()))


# ---- 1. encode ----
@pytest.mark.parametrize("mode", NULL_MODES)
@pytest.mark.parametrize("n", SIZES)
def test_encode_decimal_results(n, mode):
    case = out_case(n, mode)
    got = _encode(case, n)
    _same(got, case["ref"])
    if n == 0:
        assert got == W.encode_event(*WM)


@pytest.mark.parametrize("n", [65, 4097])
def test_encode_host_rows_and_host_bytes(n):
    case = out_case(n, "quarter")
    _same(_encode(case, n, device=False, host=True), case["ref"])
    _same(_encode(case, n, device=False, host=False), case["ref"])
    _same(_encode(case, n, device=True, host=True), case["ref"])


# ---- 2. STRING key columns beside the DECIMALs ----
STR_FIELDS = ["STRING", "DECIMAL", "STRING", "LONG", "DECIMAL", "LONG"]
STR_SCHEMA = [("STRING", ("KEYCOL", 0, "STRING")), ("DECIMAL", ("AGG", 0, "SUM_DEC128")), ("STRING", ("KEYCOL", 1, "STRING")),
              ("LONG", ("AGG", 1, "COUNT")), ("DECIMAL", ("AGG", 2, "AVG_DEC")), ("LONG", "WIN_END")]
LENS = [0, 1, 7, 8, 9, 16, 17, 40]


def _arrow(vals, garbage=b"GARBAGE-UNDER-A-NULL"):
    """Arrow offsets / bytes / NULL flags of a list of bytes-or-None; a NULL keeps garbage bytes in the column."""
    parts = [garbage[:1 + i % len(garbage)] if v is None else v for i, v in enumerate(vals)]
    offs = np.zeros(len(vals) + 1, np.int32)
    offs[1:] = np.cumsum([len(p) for p in parts])
    data = np.frombuffer(b"".join(parts) or b"\0", np.uint8).copy()
    return offs, data, np.array([v is None for v in vals], np.uint8)


@pytest.mark.parametrize("big", [False, True], ids=["staged", "direct"])
def test_encode_strings_beside_decimals(big):
    """big: one 70 000-byte value makes its tile of 64 rows too long for LDS, so that tile's DECIMAL parts are written
    by the direct path; the 65th row's tile stays staged."""
    import torch
    n = 65
    base = out_case(n, "quarter")
    rng = np.random.default_rng(6000 + big)
    strs = []
    for k in range(2):
        col = []
        for i in range(n):
            ln = LENS[int(rng.integers(0, len(LENS)))]
            col.append(None if rng.random() < 0.15 else bytes(rng.integers(0x20, 0x7F, ln, dtype=np.uint8)))
        strs.append(col)
    if big:
        strs[0][10] = bytes(rng.integers(0, 256, 70_000, dtype=np.uint8))
    rows = [(strs[0][i], r[1], strs[1][i], r[2], r[3], r[5]) for i, r in enumerate(base["rows"])]
    ref, starts = D.encode_stream(STR_FIELDS, rows, None, [(n, WM[0], WM[1])])
    assert (max(np.diff(starts + [len(ref) - 13])) > 70_000) == big
    cols, nulls = [], []
    for col in strs:
        o, b, z = _arrow(col)
        cols.append((torch.from_numpy(o).cuda(), torch.from_numpy(b).cuda()))
        nulls.append(torch.from_numpy(z).cuda())
    _same(_encode(base, n, schema=STR_SCHEMA, keycols=(cols, nulls)), ref)


# ---- 3. decode ----
IN_FIELDS = ["LONG", "DECIMAL", "STRING", "DECIMAL", "LONG"]
IN_STRINGS = [None, "", "seven77", "eight888", "a-string-of-20-bytes", "x" * 40]


@functools.lru_cache(maxsize=None)
def in_case(n):
    """A reference-written stream of n records [LONG key, DECIMAL, STRING, DECIMAL, LONG] with record timestamps: both
    NULL forms and minimal / non-minimal lengths from record to record, events in between."""
    rng = np.random.default_rng(7000 + n)
    d1, d3 = decimals(rng, n), decimals(rng, n, shift=29)
    rows = []
    for i in range(n):
        s = IN_STRINGS[int(rng.integers(0, len(IN_STRINGS)))]
        rows.append((int(rng.integers(-(1 << 62), 1 << 62)), None if rng.random() < 0.2 else d1[i], s,
                     None if rng.random() < 0.2 else d3[i], None if i % 9 == 4 else i * 3))
    ts = rng.integers(0, 1 << 44, n)
    events = [(0, 4, (0,))] + [(p, 2, (1000 + p,)) for p in range(50, n, 211)] + [(n // 2, 3, (1, 2, 3, 4)), (n, 2, (1 << 50,)),
                                                                                 (n, 5, (1,))]
    events.sort(key=lambda e: e[0])
    data, starts = D.encode_stream(IN_FIELDS, rows, ts, events, null_form=lambda i: ("setnull", "write")[(i // 3) % 2],
                                   dec_len=lambda i: (None, 16, None, 9)[i % 4])
    return dict(rows=rows, ts=ts, data=data, starts=starts)


def _decode_pieces(schema, data, cuts, fields, cols, str_fields=()):
    """Feed data[.. cuts[0]], data[cuts[0] .. cuts[1]], ... to one WireDecoder, carrying the tail after `consumed` over;
    every piece is checked against the reference decoder on the same buffer, and the whole is returned."""
    dec = wire.WireDecoder(schema)
    res = dict(key=[], ts=[], cols=[[] for _ in cols], col_null=[[] for _ in cols], events=[],
               strs={f: ([], [], []) for f in str_fields})
    carry, at, nrec = b"", 0, 0
    for c in sorted(set(list(cuts) + [len(data)])):
        buf = carry + data[at:c]
        at = c
        got = dec.decode(buf)
        rc, want = D.decode(fields, buf, key_field=schema.key_field, ts_field=schema.ts_field, cols=cols)
        assert rc == 0 and got.consumed == want["consumed"] and got.n_records == want["n_records"], \
            "piece ending at %d: consumed %d records %d, reference %d / %d" % (c, got.consumed, got.n_records, want["consumed"], want["n_records"])
        if got.key is not None:
            res["key"].append(got.key.cpu().numpy().copy())
        res["ts"].append(got.ts.cpu().numpy().copy())
        for j in range(len(cols)):
            res["cols"][j].append(got.cols[j].cpu().numpy().copy())
            res["col_null"][j].append(got.col_null[j].cpu().numpy().copy())
        for f in str_fields:
            o, b, z = got.strings(f)
            o = o.cpu().numpy()
            res["strs"][f][0].append(np.diff(o))
            res["strs"][f][1].append(b.cpu().numpy()[:o[-1]].copy())
            res["strs"][f][2].append(z.cpu().numpy().copy())
        res["events"] += [(nrec + p, t, v) for p, t, v in zip(got.evt_pos.tolist(), got.evt_tag.tolist(), got.evt_val.tolist())]
        nrec += got.n_records
        carry = buf[got.consumed:]
    dec.close()
    assert carry == b""
    res["key"], res["ts"] = (np.concatenate(res[k]) if res[k] else None for k in ("key", "ts"))
    res["cols"] = [np.concatenate(c) for c in res["cols"]]
    res["col_null"] = [np.concatenate(c) for c in res["col_null"]]
    res["strs"] = {f: tuple(np.concatenate(x) for x in v) for f, v in res["strs"].items()}
    return res, nrec


def _assert_decoded(res, nrec, want, fields, cols):
    """Bit-exact against the reference decode of the whole stream."""
    assert nrec == want["n_records"]
    if want["key"] is not None:
        assert np.array_equal(res["key"], want["key"])
    assert np.array_equal(res["ts"], want["ts"])
    for j, f in enumerate(cols):
        assert np.array_equal(res["col_null"][j], want["col_null"][j]), "NULL flags of column %d" % j
        if fields[f] == "DECIMAL":
            assert res["cols"][j].shape == (nrec, 2) and res["cols"][j].dtype == np.int64
            exp = A.dec128_column(want["cols"][j]).reshape(-1, 2)
            bad = np.flatnonzero((res["cols"][j] != exp).any(axis=1))
            assert bad.size == 0, "column %d record %d: %s, reference %d" % (
                j, bad[0], A.dec128_values(res["cols"][j][bad[0]].tobytes())[0], want["cols"][j][bad[0]])
        else:
            assert np.array_equal(res["cols"][j].view(np.uint64), want["cols"][j])
    assert res["events"] == list(zip(want["evt_pos"].tolist(), want["evt_tag"].tolist(), want["evt_val"].tolist()))


def _cuts(case, n):
    """Inside a variable-length part (the 16 bytes of a record's first DECIMAL), just past the 4096-byte chunk boundaries
    and inside the length prefix of the elements that cross them, and an element boundary."""
    data, starts = case["data"], case["starts"]
    cuts = []
    withvar = [i for i, r in enumerate(case["rows"]) if r[1] is not None]
    for i in withvar[len(withvar) // 3::max(1, len(withvar) // 3)][:2]:
        end = starts[i + 1] if i + 1 < n else len(data)
        cuts.append(min(end, starts[i] + 4 + 13 + 4 + 48 + 16) - 3)   # in the 16 bytes of the first DECIMAL
    for edge in (4096, 8192):
        if len(data) > edge + 300:
            i = int(np.searchsorted(starts, edge, side="right")) - 1
            cuts += [edge + 1, starts[i] + 2]
    if n > 10:
        cuts.append(starts[n // 5])
    return [c for c in cuts if 0 < c < len(data)]


@pytest.mark.parametrize("n", SIZES)
def test_decode_decimal_columns(n):
    case = in_case(n)
    data = case["data"]
    for cols, key_field in [([1, 3, 4], 0), ([3], 0), ([4, 1, 0], -1)]:      # all read; field 1 unread; beside a STRING key
        s = wire.make_schema(IN_FIELDS, key_field=key_field, ts_field=-1, cols=cols, fmt="ROWDATA")
        rc, want = D.decode(IN_FIELDS, data, key_field=key_field, cols=cols)
        assert rc == 0 and want["consumed"] == len(data) and want["n_records"] == n
        res, nrec = _decode_pieces(s, data, [], IN_FIELDS, cols, str_fields=[2])
        _assert_decoded(res, nrec, want, IN_FIELDS, cols)
        lens, sb, sz = res["strs"][2]
        wo, wb, wz = want["strings"][2]
        assert np.array_equal(lens, np.diff(wo)) and bytes(sb) == bytes(wb) and np.array_equal(sz, wz)
        if n > 1 and cols == [1, 3, 4]:
            res, nrec = _decode_pieces(s, data, _cuts(case, n), IN_FIELDS, cols)
            _assert_decoded(res, nrec, want, IN_FIELDS, cols)
    want_ts = case["ts"]
    assert np.array_equal(res["ts"], want_ts)


def test_decode_rows_without_strings_and_a_rowtime_field():
    """DECIMAL fields alone make the rows vary in length (the setNullAt form); ts from a field, device bytes."""
    import torch
    fields = ["LONG", "LONG", "DECIMAL", "DECIMAL"]
    rng = np.random.default_rng(11)
    n = 700
    d = decimals(rng, 2 * n)
    rows = [(i % 13, 5 * i, None if i % 3 == 0 else d[i], None if i % 5 == 0 else d[n + i]) for i in range(n)]
    data, starts = D.encode_stream(fields, rows, None, [(n, 2, (9,))])
    s = wire.make_schema(fields, key_field=0, ts_field=1, cols=[2, 3], fmt="ROWDATA")
    dec = wire.WireDecoder(s)
    got = dec.decode(torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda())
    assert got.n_records == n and got.consumed == len(data)
    assert got.ts.cpu().tolist() == [r[1] for r in rows] and got.key.cpu().tolist() == [r[0] for r in rows]
    for j, f in enumerate([2, 3]):
        assert got.cols[j].shape == (n, 2)
        assert list(A.dec128_values(got.cols[j].cpu().numpy().tobytes())) == [0 if r[f] is None else r[f] for r in rows]
        assert got.col_null[j].cpu().tolist() == [int(r[f] is None) for r in rows]
    empty = dec.decode(b"")
    assert empty.n_records == 0 and tuple(empty.cols[0].shape) == (0, 2)
    dec.close()


# ---- 4. corrupt slots ----
@pytest.mark.parametrize("which", sorted(CPU.BAD_SLOTS))
def test_corrupt_decimal_slot(which):
    rows = [r for r in CPU._rows(900) if r[1] is not None and r[3] is not None][:200]
    data, starts = D.encode_stream(CPU.FIELDS, rows, None, [(200, 2, (5,))])
    i = 150
    assert starts[i] > 2 * 4096                                    # not in the first chunk
    size = len(D.row_bytes(CPU.FIELDS, rows[i]))
    bad = CPU.corrupt_slot(data, starts[i], CPU.FIELDS, 3, CPU.BAD_SLOTS[which](size))
    rc, ref = D.decode(CPU.FIELDS, bad, key_field=0, cols=[1, 3])
    assert rc == D.E_CORRUPT and ref["err_pos"] == starts[i]
    s = wire.make_schema(CPU.FIELDS, key_field=0, cols=[1, 3], fmt="ROWDATA")
    dec = wire.WireDecoder(s)
    with pytest.raises(Exception) as ei:
        dec.decode(bad)
    assert ei.value.code == D.E_CORRUPT and "DECIMAL slot" in str(ei.value) and ("byte %d" % starts[i]) in str(ei.value), str(ei.value)
    got = dec.decode(data)                                         # the decoder stays usable
    assert got.n_records == 200 and got.consumed == len(data)
    assert list(A.dec128_values(got.cols[1].cpu().numpy().tobytes())) == [r[3] for r in rows]
    dec.close()
    # the same slot under a NULL bit, or in a field no column reads, is not looked at
    s1 = wire.make_schema(CPU.FIELDS, key_field=0, cols=[1], fmt="ROWDATA")
    dec = wire.WireDecoder(s1)
    got = dec.decode(bad)
    assert got.n_records == 200 and list(A.dec128_values(got.cols[0].cpu().numpy().tobytes())) == [r[1] for r in rows]
    dec.close()
    nb = bytearray(bad)
    nb[starts[i] + 9 + 1] |= 1 << 3                                # null bit of field 3: bit 11
    dec = wire.WireDecoder(s)
    got = dec.decode(bytes(nb))
    assert got.n_records == 200
    assert got.col_null[1].cpu().tolist() == [int(j == i) for j in range(200)]
    assert list(A.dec128_values(got.cols[1].cpu().numpy().tobytes())) == [0 if j == i else r[3] for j, r in enumerate(rows)]
    dec.close()


# ---- 5. round trip ----
@pytest.mark.parametrize("mode", ["quarter", "noflags"])
def test_round_trip(mode):
    n = 4097
    case = out_case(n, mode)
    data = _encode(case, n)
    s = wire.make_schema(OUT_FIELDS, key_field=0, ts_field=5, cols=[1, 2, 3, 4], fmt="ROWDATA")
    rng = np.random.default_rng(3)
    cuts = rng.integers(1, len(data), 7).tolist()
    res, nrec = _decode_pieces(s, data, cuts, OUT_FIELDS, [1, 2, 3, 4])
    assert nrec == n and np.array_equal(res["key"], case["key"]) and np.array_equal(res["ts"], case["we"])
    nulls = [z if mode == "quarter" else np.zeros(n, bool) for z in case["z"]]
    for j, (d, z) in zip((0, 2), zip(case["d"], nulls)):
        assert np.array_equal(res["col_null"][j].astype(bool), z)
        assert list(A.dec128_values(res["cols"][j].tobytes())) == [0 if z[i] else d[i] for i in range(n)]
    assert np.array_equal(res["cols"][1], case["aggs"][1]) and np.array_equal(res["cols"][3], case["ws"])
    assert not res["col_null"][1].any() and not res["col_null"][3].any()
    assert res["events"] == [(n, 2, [WM[1][0], 0, 0, 0])]


# ---- 6. the schema checks with a device behind them ----
def test_refusals_and_acceptances_on_the_device_path():
    S = ["LONG", "DECIMAL", "LONG", "STRING"]
    assert CPU._create(wire.make_schema(S, key_field=0, ts_field=2, cols=[1], fmt="ROWDATA")) == 0
    assert CPU._create(wire.make_schema(S, key_field=0, ts_field=2, cols=[], fmt="ROWDATA")) == 0
    assert CPU._create(wire.make_schema(S, key_field=-1, cols=[1, 0], fmt="ROWDATA")) == 0
    assert CPU._enc_create(OUT_SCHEMA) == (0, "")
    for kind in A.DEC_KINDS:
        assert CPU._enc_create([("DECIMAL", ("AGG", 3, kind)), ("STRING", ("KEYCOL", 0, "STRING"))]) == (0, "")
    CPU.test_decoder_create_refusals_and_acceptances()
    CPU.test_encoder_create_refusals_and_acceptances()
    CPU.test_make_out_schema_pairs_decimal_with_decimal_aggregates()
    # at encode: a DECIMAL aggregate the rows do not carry
    enc = wire.WireEncoder(wire.make_out_schema([("LONG", "KEY"), ("DECIMAL", ("AGG", 3, "SUM_DEC"))], fmt="ROWDATA"))
    case = out_case(65, "quarter")
    out, keep = make_out(65, case["key"], case["ws"], case["we"], case["aggs"], case["nulls"])
    with pytest.raises(Exception) as ei:
        enc.encode(out)
    assert ei.value.code == -1 and "aggregate 3 is not in the rows" in str(ei.value)
    enc.close()


# ---- 7. end to end ----
class _Fired:
    """The engine as NetworkOutput sees it, keeping the rows of every watermark step as the engine returned them."""

    def __init__(self, eng):
        self.eng, self.steps = eng, []

    def advance_watermark_raw(self, wm):
        out = self.eng.advance_watermark_raw(wm)
        self.steps.append(self.eng._rows(out))
        return out


class _Through:
    """The engine as NetworkInput sees it: a watermark of the input channel is the output channel's emit."""

    def __init__(self, eng, net):
        self.eng, self.net, self.cfg, self.sent = eng, net, eng.cfg, []

    def push(self, *a, **kw):
        return self.eng.push(*a, **kw)

    def advance_watermark(self, wm):
        self.sent.append((wm, bytes(self.net.emit(wm).cpu().numpy())))
        return len(self.sent)


@pytest.mark.parametrize("on_device", [1, 0], ids=["device-rows", "host-rows"])
def test_table_job_with_decimal_aggregates_from_bytes_to_bytes(on_device):
    """Table TUMBLE, COUNT / SUM / AVG over a nullable DECIMAL(38, 2) column: a reference-encoded channel stream ->
    NetworkInput -> engine -> NetworkOutput.emit. The emitted bytes are the reference encoding of the rows the engine
    returned, and decoded by the reference they are the oracle's rows (per watermark, as a multiset); a SUM that leaves
    38 digits is a NULL among them."""
    from flink_amd.engine import WindowAggregator
    from oracle.oracle import Oracle
    rng = np.random.default_rng(21)
    n = 400
    key = rng.integers(0, 40, n).astype(np.int64)
    ts = (np.arange(n) * 10 + rng.integers(0, 300, n)).astype(np.int64)
    vals = [int(x) * 10 ** 12 + int(y) for x, y in zip(rng.integers(-10 ** 15, 10 ** 15, n), rng.integers(0, 10 ** 12, n))]
    isnull = rng.random(n) < 0.2
    for i in (100, 101):                                           # two records of one key and window: 1.2e38 overflows
        key[i], ts[i], vals[i], isnull[i] = 99, 1500, 6 * 10 ** 37, False
    for i in (102, 103):                                           # a key whose only records are NULL: SUM and AVG NULL
        key[i], ts[i], isnull[i] = 98, 1600, True
    in_fields = ["LONG", "LONG", "DECIMAL"]
    rows = [(int(key[i]), int(ts[i]), None if isnull[i] else vals[i]) for i in range(n)]
    wms = [(150, 1400), (300, 2900), (n, A.LONG_MAX)]
    stream, starts = D.encode_stream(in_fields, rows, None, [(p, 2, (wm,)) for p, wm in wms],
                                     null_form=lambda i: ("setnull", "write")[i % 2], dec_len=lambda i: (None, 16)[(i // 2) % 2])
    base = dict(window_kind="TUMBLE", semantics="TABLE", size_ms=1000, key_capacity=1 << 10, nullable_cols=(0,),
                aggs=[("COUNT", 0), ("SUM_DEC128", 0, 2), ("AVG_DEC128", 0, 2)])
    eng = WindowAggregator(A.make_config(output_on_device=on_device, **base))
    out_fields = ["LONG", "LONG", "DECIMAL", "DECIMAL", "LONG", "LONG"]
    fired = _Fired(eng)
    net = wire.NetworkOutput(wire.make_out_schema(
        [("LONG", "KEY"), ("LONG", ("AGG", 0, "COUNT")), ("DECIMAL", ("AGG", 1, "SUM_DEC128")),
         ("DECIMAL", ("AGG", 2, "AVG_DEC128")), ("LONG", "WIN_START"), ("LONG", "WIN_END")], fmt="ROWDATA"), fired)
    through = _Through(eng, net)
    inp = wire.NetworkInput(wire.make_schema(in_fields, key_field=0, ts_field=1, cols=[2], fmt="ROWDATA"), through)
    cuts = [starts[40] + 30, 4096 + 7, starts[250] + 50, len(stream)]
    at = 0
    for c in cuts:
        inp.feed(stream[at:c])
        at = c
    assert inp.carry == b"" and inp.records_in == n and len(through.sent) == 3 and inp.late_dropped == 0
    o = Oracle(A.make_config(**base))
    col, zf = A.dec128_column(vals), isnull.astype(np.uint8)
    a, total, saw_null = 0, 0, 0
    for (p, wm), (got_wm, data), r in zip(wms, through.sent, fired.steps):
        assert got_wm == wm
        assert o.push(key[a:p], ts[a:p], [col[a:p]], nulls=[zf[a:p]]) == 0
        a = p
        ro = o.advance_watermark(wm)

        def tuples(x):
            m = len(x["key"])
            nul = [x.get("null%d" % j) for j in range(3)]
            return [(int(x["key"][i]), int(x["agg0"][i])) +
                    tuple(None if nul[j] is not None and nul[j][i] else int(x["agg%d" % j][i]) for j in (1, 2)) +
                    (int(x["win_start"][i]), int(x["win_end"][i])) for i in range(m)]
        mine = tuples(r)
        ref, _ = D.encode_stream(out_fields, mine, None, [(len(mine), 2, (wm,))])
        _same(data, ref)                                           # the bytes are the rows the engine returned, in order
        back, events = D.decode_rows(out_fields, data)
        assert events == [(len(mine), 2, [wm, 0, 0, 0])]
        exp = Counter(tuples(ro))
        assert Counter(back) == exp, "watermark %d: only GPU %s, only oracle %s" % (
            wm, list((Counter(back) - exp).items())[:3], list((exp - Counter(back)).items())[:3])
        total += len(back)
        saw_null += sum(1 for t in back if t[2] is None)
        if wm == 2900:
            assert (99, 2, None, None, 1000, 2000) in exp          # 6e37 + 6e37: outside DECIMAL(38, 2)
            assert any(t[0] == 98 and t[2] is None and t[3] is None for t in exp)      # nothing but NULLs
    assert total > 100 and net.rows_out == total and saw_null >= 2
    assert bytes(net.emit(A.LONG_MAX).cpu().numpy()) == W.encode_event(2, (A.LONG_MAX,))      # the zero-row path
    for x in (net, inp, eng):
        x.close()
    o.close()
