"""GPU wire encoder (fwa_wire_encode) against the reference encoders, byte for byte and in order: oracle.wire_encode for
fixed-length TUPLE / ROWDATA values, tests/wire_strings_ref.py for rows with STRING fields. The columns are hand-made
tensors wrapped in an fwa_out, so nothing but the encoder stands between them and the bytes. Then host rows / host bytes,
the non-record elements, the round trip through the GPU decoder, the refusals, and two jobs end to end through
NetworkOutput: a dictionary-keyed Table job, and two DataStream operators joined by nothing but bytes."""
import ctypes as C
import functools
from collections import Counter

import numpy as np
import pytest

from flink_amd import _abi as A
from flink_amd import wire
from oracle import wire_encode as W

import wire_strings_ref as R

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 4097, 100_003]
WM = (2, (1_700_000_000_123,))
WM_BYTES = W.encode_event(*WM)


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


def _specials64(rng, n):
    bits = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    sp = np.array([0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000001, 0x7FF0000000000001,
                   0xFFFFFFFFFFFFFFFF, 0, 1], np.uint64)          # -0.0, +-Inf, quiet / signalling NaN payloads, ...
    bits[:min(n, len(sp))] = sp[:n]
    return bits.view(np.float64)


def _specials32(rng, n):
    bits = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    sp = np.array([0x80000000, 0x7F800000, 0xFF800000, 0x7FC00001, 0x7F800001, 0xFFFFFFFF, 0, 1], np.uint32)
    bits[:min(n, len(sp))] = sp[:n]
    return bits.view(np.float32)


@functools.lru_cache(maxsize=None)
def tuple_case(which, n):
    """Columns, schema arguments and the reference bytes of case 1 (computed once per size, shared, never changed)."""
    rng = np.random.default_rng(1000 + n)
    key = rng.integers(-(1 << 63), 1 << 63, n)
    ws = rng.integers(-(1 << 40), 1 << 45, n)
    we = ws + 1000
    if which == 45:
        aggs = [rng.integers(-(1 << 62), 1 << 62, n), _specials64(rng, n), _specials32(rng, n),
                rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32)]
        kinds = ["SUM_I64", "SUM_F64", "SUM_F32", "SUM_I32"]
        wire_fields = ["LONG", "LONG", "DOUBLE", "FLOAT", "INT"]
        schema = [("LONG", "KEY")] + [(t, ("AGG", j, k)) for j, (t, k) in enumerate(zip(wire_fields[1:], kinds))]
        values = [key] + aggs
    else:
        aggs = [rng.integers(0, 1 << 40, n)]
        wire_fields = ["LONG", "LONG", "LONG"]
        schema = [("LONG", "KEY"), ("LONG", ("AGG", 0, "COUNT")), ("LONG", "WIN_START")]
        values = [key, aggs[0], ws]
    ref = W.encode_records(wire_fields, values, we - 1, "TUPLE") + WM_BYTES
    assert len(ref) == which * n + 13
    for v in [key, ws, we] + aggs:
        v.setflags(write=False)
    return dict(schema=schema, wire_fields=wire_fields, key=key, ws=ws, we=we, aggs=aggs, values=values, ref=ref)


@functools.lru_cache(maxsize=None)
def rowdata_case(n):
    rng = np.random.default_rng(2000 + n)
    key = rng.integers(-(1 << 63), 1 << 63, n)
    ws = rng.integers(-(1 << 40), 1 << 45, n)
    we = ws + 5000
    aggs = [rng.integers(-(1 << 62), 1 << 62, n) | 1, _specials64(rng, n), rng.integers(1, 1 << 31, n).astype(np.int32)]
    aggs[1] = np.where(aggs[1].view(np.uint64) == 0, 1.5, aggs[1])           # non-zero garbage under every NULL flag
    nulls = [np.zeros(n, bool), np.ones(n, bool), np.arange(n) % 3 == 0]
    wire_fields = ["LONG", "LONG", "DOUBLE", "INT", "LONG", "LONG", "LONG"]
    schema = [("LONG", "KEY"), ("LONG", ("AGG", 0, "SUM_I64")), ("DOUBLE", ("AGG", 1, "MAX_F64")),
              ("INT", ("AGG", 2, "MIN_I32")), ("LONG", "WIN_START"), ("LONG", "WIN_END"), ("LONG", "WIN_TIME")]
    values = [key] + aggs + [ws, we, we - 1]
    ref = W.encode_records(wire_fields, values, None, "ROWDATA", nulls=[None] + nulls + [None] * 3) + WM_BYTES
    assert len(ref) == 73 * n + 13
    return dict(schema=schema, wire_fields=wire_fields, key=key, ws=ws, we=we, aggs=aggs, nulls=nulls, values=values, ref=ref)


def _encode(case, fmt, record_ts, n, device=True, host=False, events=(WM,)):
    enc = wire.WireEncoder(wire.make_out_schema(case["schema"], fmt=fmt, record_ts=record_ts))
    out, keep = make_out(n, case["key"], case["ws"], case["we"], case["aggs"], case.get("nulls", ()), device=device)
    got = enc.encode(out, events=events, host=host)
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


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("esize", [45, 37])
def test_fixed_tuple_with_timestamps(esize, n):
    case = tuple_case(esize, n)
    got = _encode(case, "TUPLE", "WIN_TIME", n)
    _same(got, case["ref"])
    if n == 0:
        assert got == WM_BYTES and len(got) == 13


@pytest.mark.parametrize("n", SIZES)
def test_fixed_rowdata_with_nulls(n):
    case = rowdata_case(n)
    _same(_encode(case, "ROWDATA", None, n), case["ref"])


# ---- STRING fields ----
LENS = [0, 1, 6, 7, 8, 9, 15, 16, 17, 40]


def _arrow(vals, garbage=b"GARBAGE-UNDER-A-NULL"):
    """Arrow offsets / bytes / NULL flags of a list of bytes-or-None; a NULL keeps garbage bytes in the column."""
    parts = [garbage[:1 + i % len(garbage)] if v is None else v for i, v in enumerate(vals)]
    offs = np.zeros(len(vals) + 1, np.int32)
    offs[1:] = np.cumsum([len(p) for p in parts])
    data = np.frombuffer(b"".join(parts) or b"\0", np.uint8).copy()
    return offs, data, np.array([v is None for v in vals], np.uint8)


@functools.lru_cache(maxsize=None)
def string_case(two, n, big=False):
    rng = np.random.default_rng(3000 + n + two)

    def strs(salt):
        out = []
        for i in range(n):
            if rng.random() < 0.1:
                out.append(None)
            else:
                ln = LENS[int(rng.integers(0, len(LENS)))]
                out.append(bytes(rng.integers(0x20, 0x7F, ln, dtype=np.uint8)))
        return out
    s0 = strs(0)
    if big:
        s0[n // 2] = bytes(rng.integers(0, 256, 70_000, dtype=np.uint8))
    s1 = strs(1) if two else None
    k = rng.integers(-(1 << 62), 1 << 62, n)
    kz = rng.random(n) < 0.1
    a0 = rng.integers(-(1 << 50), 1 << 50, n) | 1
    a0z = np.arange(n) % 4 == 1
    a1 = rng.standard_normal(n)
    we = rng.integers(0, 1 << 44, n)
    fields = ["STRING", "LONG"] + (["STRING"] if two else []) + ["LONG", "DOUBLE", "LONG"]
    schema = [("STRING", ("KEYCOL", 0, "STRING")), ("LONG", ("KEYCOL", 1, "BIGINT"))]
    schema += [("STRING", ("KEYCOL", 2, "STRING"))] if two else []
    schema += [("LONG", ("AGG", 0, "SUM_I64")), ("DOUBLE", ("AGG", 1, "SUM_F64")), ("LONG", "WIN_END")]
    rows = []
    for i in range(n):
        r = [s0[i], None if kz[i] else int(k[i])] + ([s1[i]] if two else [])
        rows.append(tuple(r + [None if a0z[i] else int(a0[i]), float(a1[i]), int(we[i])]))
    ref, starts = R.encode_stream(fields, rows, None, [(n, WM[0], WM[1])])
    return dict(schema=schema, fields=fields, s0=s0, s1=s1, k=k, kz=kz, aggs=[a0, a1], nulls=[a0z], we=we, rows=rows,
                ref=ref, starts=starts)


def _encode_strings(case, n):
    import torch
    enc = wire.WireEncoder(wire.make_out_schema(case["schema"], fmt="ROWDATA"))
    out, keep = make_out(n, None, None, case["we"], case["aggs"], case["nulls"])
    cols, nulls = [], []
    for vals in [case["s0"], None, case["s1"]]:
        if vals is None:
            if len(cols) == 1:
                cols.append(torch.from_numpy(case["k"]).cuda())
                nulls.append(torch.from_numpy(case["kz"].view(np.uint8)).cuda())
            continue
        o, b, z = _arrow(vals)
        cols.append((torch.from_numpy(o).cuda(), torch.from_numpy(b).cuda()))
        nulls.append(torch.from_numpy(z).cuda())
    got = bytes(enc.encode(out, keycols=(cols, nulls), events=[WM]).cpu().numpy())
    st = enc.stats()
    assert st.rows_in == n and st.bytes_out == len(got)
    enc.close()
    return got


@pytest.mark.parametrize("n", [1, 64, 65, 5000])
@pytest.mark.parametrize("two", [False, True])
def test_string_fields(two, n):
    case = string_case(two, n)
    _same(_encode_strings(case, n), case["ref"])


def test_a_value_longer_than_the_lds_tile():
    """One 70 000-byte value among short ones: its tile is written directly, the others stay staged."""
    case = string_case(False, 200, big=True)
    assert max(np.diff(case["starts"] + [len(case["ref"]) - 13])) > 70_000
    _same(_encode_strings(case, 200), case["ref"])


def test_host_rows_and_host_bytes():
    for n in (65, 4097):
        case = tuple_case(45, n)
        _same(_encode(case, "TUPLE", "WIN_TIME", n, device=False, host=True), case["ref"])
        _same(_encode(case, "TUPLE", "WIN_TIME", n, device=False, host=False), case["ref"])
        _same(_encode(case, "TUPLE", "WIN_TIME", n, device=True, host=True), case["ref"])


EVENTS = [(3, (1_700_000_000_000, -5, 1 << 62, 7)), (4, (-1,)), (2, (-(1 << 63),)), (5, (1,)), (4, (0,)), (5, (0,)),
          (3, (-1, -1, -1, -1)), (2, ((1 << 63) - 1,))]


def test_events_alone_and_behind_rows():
    ev_ref = b"".join(W.encode_event(t, v) for t, v in EVENTS)
    case = tuple_case(37, 65)
    assert _encode(case, "TUPLE", "WIN_TIME", 0, events=EVENTS) == ev_ref
    assert _encode(case, "TUPLE", "WIN_TIME", 0, events=EVENTS, host=True) == ev_ref
    assert _encode(case, "TUPLE", "WIN_TIME", 0, events=()) == b""
    _same(_encode(case, "TUPLE", "WIN_TIME", 65, events=EVENTS), case["ref"][:-13] + ev_ref)
    rcase = rowdata_case(63)
    _same(_encode(rcase, "ROWDATA", None, 63, events=EVENTS[:3]), rcase["ref"][:-13] + b"".join(W.encode_event(t, v) for t, v in EVENTS[:3]))
    with pytest.raises(Exception) as ei:
        _encode(case, "TUPLE", "WIN_TIME", 0, events=[(1, (0,))])
    assert ei.value.code == -1 and "tag 1" in str(ei.value)


# ---- round trip through the GPU decoder ----
def _decode_in_pieces(schema, data, seed, str_fields=()):
    """Cut the stream at arbitrary positions, feed the pieces to one WireDecoder (carrying partial elements over) and
    concatenate what comes back."""
    rng = np.random.default_rng(seed)
    cuts = sorted(set(rng.integers(1, max(2, len(data)), 6).tolist() + [len(data)]))
    dec = wire.WireDecoder(schema)
    res = dict(key=[], ts=[], cols=[[] for _ in range(schema.num_cols)], col_null=[[] for _ in range(schema.num_cols)],
               events=[], strs={f: ([], [], []) for f in str_fields})
    carry, at, nrec = b"", 0, 0
    for c in cuts:
        buf = carry + data[at:c]
        at = c
        got = dec.decode(buf)
        n = got.n_records
        if got.key is not None:
            res["key"].append(got.key.cpu().numpy())
        res["ts"].append(got.ts.cpu().numpy())
        for j in range(schema.num_cols):
            res["cols"][j].append(got.cols[j].cpu().numpy().copy())
            if got.col_null is not None:
                res["col_null"][j].append(got.col_null[j].cpu().numpy().copy())
        for f in str_fields:
            o, b, z = got.strings(f)
            o = o.cpu().numpy()
            res["strs"][f][0].append(np.diff(o))
            res["strs"][f][1].append(b.cpu().numpy()[:o[-1]].copy())
            res["strs"][f][2].append(z.cpu().numpy().copy())
        res["events"] += [(nrec + p, t, v) for p, t, v in zip(got.evt_pos.tolist(), got.evt_tag.tolist(), got.evt_val.tolist())]
        nrec += n
        carry = buf[got.consumed:]
    dec.close()
    assert carry == b""
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0)
    res["key"], res["ts"] = cat(res["key"]), cat(res["ts"])
    res["cols"] = [cat(c) for c in res["cols"]]
    res["col_null"] = [cat(c) for c in res["col_null"]]
    res["strs"] = {f: tuple(cat(x) for x in v) for f, v in res["strs"].items()}
    return res, nrec


@pytest.mark.parametrize("n", [65, 4097])
def test_round_trip_fixed(n):
    case = tuple_case(45, n)
    got = _encode(case, "TUPLE", "WIN_TIME", n)
    s = wire.make_schema(case["wire_fields"], key_field=0, ts_field=-1, cols=[1, 2, 3, 4])
    res, nrec = _decode_in_pieces(s, got, n)
    assert nrec == n and np.array_equal(res["key"], case["key"]) and np.array_equal(res["ts"], case["we"] - 1)
    want = [case["aggs"][0], case["aggs"][1], case["aggs"][2], case["aggs"][3].astype(np.int64)]
    for a, b in zip(res["cols"], want):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert res["events"] == [(n, 2, [WM[1][0], 0, 0, 0])]

    case = rowdata_case(n)
    got = _encode(case, "ROWDATA", None, n)
    s = wire.make_schema(case["wire_fields"], key_field=0, ts_field=5, cols=[1, 2, 3, 4, 6], fmt="ROWDATA")
    res, nrec = _decode_in_pieces(s, got, n + 1)
    assert nrec == n and np.array_equal(res["key"], case["key"]) and np.array_equal(res["ts"], case["we"])
    nulls = case["nulls"] + [np.zeros(n, bool)] * 2
    want = [case["aggs"][0], case["aggs"][1], case["aggs"][2].astype(np.int64), case["ws"], case["we"] - 1]
    for a, z, b, bz in zip(res["cols"], res["col_null"], want, nulls):
        assert np.array_equal(z.astype(bool), bz)
        assert np.array_equal(a.view(np.uint8), np.where(bz, np.zeros(1, b.dtype), b).view(np.uint8))
    assert res["events"] == [(n, 2, [WM[1][0], 0, 0, 0])]


@pytest.mark.parametrize("two", [False, True])
def test_round_trip_strings(two):
    n = 5000
    case = string_case(two, n)
    got = _encode_strings(case, n)
    fields = case["fields"]
    cols = [f for f, t in enumerate(fields) if t != "STRING"]
    sf = [f for f, t in enumerate(fields) if t == "STRING"]
    s = wire.make_schema(fields, key_field=-1, ts_field=-1, cols=cols, fmt="ROWDATA")
    res, nrec = _decode_in_pieces(s, got, 7 + two, str_fields=sf)
    assert nrec == n and np.all(res["ts"] == A.LONG_MIN)
    for f, vals in zip(sf, [case["s0"], case["s1"]]):
        lens, data, z = res["strs"][f]
        assert z.tolist() == [int(v is None) for v in vals]
        assert lens.tolist() == [0 if v is None else len(v) for v in vals]
        assert bytes(data) == b"".join(v for v in vals if v is not None)
    kz, a0z = case["kz"], case["nulls"][0]
    want = [(np.where(kz, 0, case["k"]), kz), (np.where(a0z, 0, case["aggs"][0]), a0z),
            (case["aggs"][1], np.zeros(n, bool)), (case["we"], np.zeros(n, bool))]
    for a, z, (b, bz) in zip(res["cols"], res["col_null"], want):
        assert np.array_equal(z.astype(bool), bz) and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert res["events"] == [(n, 2, [WM[1][0], 0, 0, 0])]


# ---- refusals ----
def test_refusals_and_their_messages():
    def refused(fields, fmt, code, msg):
        with pytest.raises(Exception) as ei:
            wire.WireEncoder(wire.make_out_schema(fields, fmt=fmt))
        assert ei.value.code == code and msg in str(ei.value), str(ei.value)
    refused([("LONG", "KEY"), ("STRING", ("KEYCOL", 0, "STRING"))], "TUPLE", -1, "STRING fields are written in ROWDATA rows only")
    refused([("LONG", ("AGG", 0, "SUM_F64"))], "TUPLE", -1, "a double source cannot be written as LONG")
    refused([("LONG", "KEY"), ("LONG", ("AGG", 1, "SUM_DEC"))], "ROWDATA", -7, "DECIMAL")
    for arity in (0, 17):
        s = wire.make_out_schema([("LONG", "KEY")])
        s.arity = arity
        with pytest.raises(Exception) as ei:
            wire.WireEncoder(s)
        assert ei.value.code == -1 and ("arity %d out of range" % arity) in str(ei.value)
    # at encode: a TUPLE value cannot carry NULLs; KEYCOL sources need the key columns
    case = rowdata_case(65)
    enc = wire.WireEncoder(wire.make_out_schema([("LONG", "KEY"), ("INT", ("AGG", 2, "MIN_I32"))], fmt="TUPLE"))
    out, keep = make_out(65, case["key"], case["ws"], case["we"], case["aggs"], case["nulls"])
    with pytest.raises(Exception) as ei:
        enc.encode(out)
    assert ei.value.code == -1 and "TupleSerializer cannot write null fields" in str(ei.value)
    out2, keep2 = make_out(65, case["key"], case["ws"], case["we"], case["aggs"], ())
    got = bytes(enc.encode(out2).cpu().numpy())                    # the encoder is usable afterwards
    assert got == W.encode_records(["LONG", "INT"], [case["key"], case["aggs"][2]], None, "TUPLE")
    enc.close()
    enc = wire.WireEncoder(wire.make_out_schema([("LONG", ("KEYCOL", 0, "BIGINT")), ("LONG", "WIN_END")], fmt="ROWDATA"))
    with pytest.raises(Exception) as ei:
        enc.encode(out2)
    assert ei.value.code == -1 and "needs the key columns" in str(ei.value)
    enc.close()
    from flink_amd.engine import WindowAggregator
    eng = WindowAggregator(A.make_config(window_kind="TUMBLE", size_ms=1000, aggs=[("SUM_I64", 0)], key_capacity=1 << 10))
    with pytest.raises(Exception) as ei:
        wire.NetworkOutput(wire.make_out_schema([("LONG", ("KEYCOL", 0, "BIGINT"))], fmt="ROWDATA"), eng)
    assert ei.value.code == -1 and "key dictionary" in str(ei.value)
    eng.close()


# ---- end to end ----
def test_table_job_through_network_output():
    """TUMBLE keyed by (VARCHAR user, BIGINT k) through a key dictionary, SUM / COUNT / nullable MAX: per watermark the
    bytes of NetworkOutput.emit split into the oracle's rows (as a multiset: the emission order among windows of equal
    end is unspecified), the watermark element last; then the other elements as elements of their own."""
    from flink_amd.engine import WindowAggregator
    from flink_amd.keydict import KeyDictionary
    from oracle.oracle import Oracle
    rng = np.random.default_rng(8)
    n = 6000
    names = [None] + ["u%d" % i for i in range(5)] + ["user-with-a-longer-name-%03d" % i for i in range(40)]
    users = [names[i] for i in rng.integers(0, len(names), n)]
    k = rng.integers(0, 6, n).astype(np.int64)
    ts = (np.arange(n) * 3 + rng.integers(0, 1500, n)).astype(np.int64)
    v = rng.integers(-1000, 1000, n).astype(np.int64)
    m = rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)
    mz = rng.random(n) < 0.7
    base = dict(window_kind="TUMBLE", semantics="TABLE", size_ms=2000, aggs=[("SUM_I64", 0), ("COUNT", 0), ("MAX_I64", 1)],
                key_kind=A.KEY_GROUP_PREFIXED, key_capacity=1 << 12, nullable_cols=(1,))
    eng = WindowAggregator(A.make_config(output_on_device=1, **base))
    kd = KeyDictionary(["STRING", "BIGINT"], max_parallelism=128, capacity=1 << 12)
    fields = ["STRING", "LONG", "LONG", "LONG", "LONG", "LONG", "LONG"]
    schema = wire.make_out_schema([("STRING", ("KEYCOL", 0, "STRING")), ("LONG", ("KEYCOL", 1, "BIGINT")),
                                   ("LONG", ("AGG", 0, "SUM_I64")), ("LONG", ("AGG", 1, "COUNT")),
                                   ("LONG", ("AGG", 2, "MAX_I64")), ("LONG", "WIN_START"), ("LONG", "WIN_END")], fmt="ROWDATA")
    net = wire.NetworkOutput(schema, eng, keydict=kd)
    sid = {}
    ids_o = np.array([sid.setdefault(key, len(sid)) for key in zip(users, k.tolist())], np.int64)
    back = {i: key for key, i in sid.items()}
    o = Oracle(A.make_config(**base))
    unz = np.array([u is None for u in users], np.uint8)
    total = 0
    steps = list(range(1500, n + 1, 1500))
    for si, p in enumerate(steps):
        sl = slice(p - 1500, p)
        ids = kd.encode([users[sl], k[sl]], [unz[sl], None]).cpu().numpy()
        eng.push(ids, ts[sl], [v[sl], m[sl]], nulls=[None, mz[sl].astype(np.uint8)])
        o.push(ids_o[sl], ts[sl], [v[sl], m[sl]], nulls=[None, mz[sl].astype(np.uint8)])
        wm = A.LONG_MAX if si == len(steps) - 1 else int(ts[:p].max()) - 1600
        data = bytes(net.emit(wm).cpu().numpy())
        ro = o.advance_watermark(wm)
        assert data[-13:] == W.encode_event(2, (wm,))
        rc, got = R.decode(fields, data, cols=[1, 2, 3, 4, 5, 6])
        assert rc == 0 and got["consumed"] == len(data) and got["n_events"] == 1 and got["evt_pos"].tolist() == [len(ro["key"])]
        so, sb, sz = got["strings"][0]
        rows = Counter()
        for i in range(got["n_records"]):
            user = None if sz[i] else bytes(sb[so[i]:so[i + 1]]).decode()
            c = [None if got["col_null"][j][i] else int(got["cols"][j].view(np.int64)[i]) for j in range(6)]
            rows[(user,) + tuple(c)] += 1
        exp = Counter()
        for i in range(len(ro["key"])):
            user, kk = back[int(ro["key"][i])]
            mx = None if ("null2" in ro and ro["null2"][i]) else int(ro["agg2"][i])
            exp[(user, kk, int(ro["agg0"][i]), int(ro["agg1"][i]), mx, int(ro["win_start"][i]), int(ro["win_end"][i]))] += 1
        assert rows == exp, "watermark %d: only GPU %s, only oracle %s" % (wm, list((rows - exp).items())[:3], list((exp - rows).items())[:3])
        total += len(ro["key"])
    assert total > 300 and net.rows_out == total
    assert any(r[4] is None for r in exp) and any(r[0] is None for r in exp)
    assert bytes(net.emit_watermark_status(-1).cpu().numpy()) == W.encode_event(4, (-1,))
    assert bytes(net.emit_latency_marker(5, 6, 7, 8).cpu().numpy()) == W.encode_event(3, (5, 6, 7, 8))
    assert bytes(net.emit_record_attributes(True).cpu().numpy()) == W.encode_event(5, (1,))
    net.close()
    eng.close()
    kd.close()


def test_two_operators_joined_by_bytes():
    """DataStream TUMBLE 1 s SUM -> NetworkOutput (TUPLE, record timestamp win_end - 1) -> NetworkInput -> TUMBLE 5 s SUM
    of the sums: nothing but channel bytes in HBM between the two engines. Against the oracle run as the same two stages."""
    from flink_amd.engine import WindowAggregator
    from oracle.oracle import Oracle
    rng = np.random.default_rng(9)
    n = 8000
    key = rng.integers(0, 200, n).astype(np.int64)
    ts = (np.arange(n) * 2 + rng.integers(0, 900, n)).astype(np.int64)
    v = rng.integers(-(1 << 30), 1 << 30, n).astype(np.int64)
    c1 = dict(window_kind="TUMBLE", semantics="DATASTREAM", size_ms=1000, aggs=[("SUM_I64", 0)], key_capacity=1 << 10)
    c2 = dict(c1, size_ms=5000)
    g1, g2 = WindowAggregator(A.make_config(output_on_device=1, **c1)), WindowAggregator(A.make_config(**c2))
    o1, o2 = Oracle(A.make_config(**c1)), Oracle(A.make_config(**c2))
    net = wire.NetworkOutput(wire.make_out_schema([("LONG", "KEY"), ("LONG", ("AGG", 0, "SUM_I64"))], record_ts="WIN_TIME"), g1)
    inp = wire.NetworkInput(wire.make_schema(["LONG", "LONG"], key_field=0, ts_field=-1, cols=[1]), g2)
    steps = list(range(2000, n + 1, 2000))
    fired = 0
    for si, p in enumerate(steps):
        sl = slice(p - 2000, p)
        g1.push(key[sl], ts[sl], [v[sl]])
        o1.push(key[sl], ts[sl], [v[sl]])
        wm = A.LONG_MAX if si == len(steps) - 1 else int(ts[:p].max()) - 1000
        got = inp.feed(net.emit(wm))                               # a device tensor: the bytes never leave HBM
        r1 = o1.advance_watermark(wm)
        assert o2.push(r1["key"], r1["win_end"] - 1, [r1["agg0"]]) == 0
        r2 = o2.advance_watermark(wm)
        assert len(got) == 1 and inp.carry == b""
        a = sorted(zip(got[0]["key"].tolist(), got[0]["win_start"].tolist(), got[0]["win_end"].tolist(), got[0]["agg0"].tolist()))
        b = sorted(zip(r2["key"].tolist(), r2["win_start"].tolist(), r2["win_end"].tolist(), r2["agg0"].tolist()))
        assert a == b
        fired += len(b)
    assert fired > 400 and inp.late_dropped == 0 and inp.records_in == net.rows_out > 1000
    for x in (net, inp, g1, g2):
        x.close()
