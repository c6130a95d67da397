"""CPU checks around DECIMAL(38) on the wire (FWA_FIELD_DECIMAL): the reference encoder / decoder the GPU is judged by
(tests/wire_decimal_ref.py) against hand-derived byte literals, against wire_strings_ref for rows without DECIMALs and
against the heap snapshot reader's accumulator-row parser; then the schema checks of fwa_wire_create /
fwa_wire_enc_create / make_out_schema, which are made before a device is touched."""
import ctypes as C
import struct

import numpy as np
import pytest

from flink_amd import _abi as A
from flink_amd import wire

import heap_reader as H
import wire_decimal_ref as D
import wire_strings_ref as R

P38 = 10 ** 38 - 1


boundary_values = D.boundary_values


def test_field_value():
    assert wire.FIELDS["DECIMAL"] == 6 and 5 not in wire.FIELDS.values()


def test_unscaled_lengths_step_where_biginteger_steps():
    for k in range(1, 17):
        assert D.unscaled_len((1 << (8 * k - 1)) - 1) == k
        assert D.unscaled_len(-(1 << (8 * k - 1))) == k
        if k < 16:
            assert D.unscaled_len(1 << (8 * k - 1)) == k + 1
            assert D.unscaled_len(-(1 << (8 * k - 1)) - 1) == k + 1
    assert D.unscaled_len(0) == 1 and D.unscaled_len(P38) == 16 and D.unscaled_len(-P38) == 16
    assert len(boundary_values()) == 7 + 4 * 16 - 2


def test_one_field_rows_are_the_hand_derived_bytes():
    one = D.row_bytes(["DECIMAL"], (1,))
    assert len(one) == 32
    assert one[:8] == bytes(8)                                     # RowKind INSERT, no null bit
    assert one[8:16] == bytes.fromhex("01 00 00 00 10 00 00 00")   # offset 16 << 32 | length 1, little-endian
    assert one[16:] == b"\x01" + bytes(15)
    for v, hexs in [(-1, "ff"), (128, "00 80"), (-129, "ff 7f"), (0, "00"), (127, "7f"), (-128, "80"),
                    (P38, "4b 3b 4c a8 5a 86 c4 7a 09 8a 22 3f ff ff ff ff")]:
        b = bytes.fromhex(hexs)
        row = D.row_bytes(["DECIMAL"], (v,))
        assert len(row) == 32 and row[:8] == bytes(8)
        assert row[8:16] == struct.pack("<II", len(b), 16)
        assert row[16:] == b + bytes(16 - len(b)), (v, row[16:].hex())


def test_null_in_each_form():
    a = D.row_bytes(["DECIMAL"], (None,), null_form="setnull")
    assert len(a) == 16 and a == b"\x00\x01" + bytes(14)           # bit 8 = field 0, a zero slot, nothing reserved
    b = D.row_bytes(["DECIMAL"], (None,), null_form="write")
    assert len(b) == 32 and b == b"\x00\x01" + bytes(6) + bytes.fromhex("00 00 00 00 10 00 00 00") + bytes(16)
    # the cursor moves in the write form: the next field's part comes 16 bytes later
    c = D.row_bytes(["DECIMAL", "DECIMAL"], (None, 5), null_form="write")
    d = D.row_bytes(["DECIMAL", "DECIMAL"], (None, 5), null_form="setnull")
    assert len(c) == 24 + 32 and c[16:24] == struct.pack("<II", 1, 40) and c[40] == 5
    assert len(d) == 24 + 16 and d[16:24] == struct.pack("<II", 1, 24) and d[24] == 5 and d[8:16] == bytes(8)


def test_parts_come_in_field_order():
    fields = ["STRING", "DECIMAL", "STRING", "LONG"]
    row = D.row_bytes(fields, ("a-string-of-20-bytes", -129, "short", 7))
    fixed = 8 + 8 * 4
    assert len(row) == fixed + 24 + 16
    assert row[8:16] == struct.pack("<II", 20, 40)                 # the long STRING: offset 40, 20 bytes in 24
    assert row[40:64] == b"a-string-of-20-bytes" + bytes(4)
    assert row[16:24] == struct.pack("<II", 2, 64)                 # the DECIMAL behind it: offset 64, 2 bytes in 16
    assert row[64:80] == b"\xff\x7f" + bytes(14)
    assert row[24:32] == b"short\x00\x00\x85"                      # inline, nothing in the variable-length part
    assert row[32:40] == struct.pack("<q", 7)
    # DECIMAL first: the STRING's part follows its 16 bytes
    row = D.row_bytes(["DECIMAL", "STRING"], (1, "nine-long"))
    assert row[8:16] == struct.pack("<II", 1, 24) and row[16:24] == struct.pack("<II", 9, 40) and len(row) == 24 + 16 + 16


def test_rows_without_decimals_are_the_string_references_rows():
    fields = ["STRING", "LONG", "INT", "DOUBLE", "FLOAT", "STRING"]
    for row in [("abc", -5, 7, 1.5, -2.25, "a-longer-string-value"), (None, None, None, None, None, None),
                ("exactly8", 1 << 62, -(1 << 31), float("inf"), 0.0, "")]:
        assert D.row_bytes(fields, row) == R.row_bytes(fields, row)
    rows = [("k%d" % i, i, i, i / 3, float(i), None) for i in range(20)]
    ev = [(3, 2, (55,)), (20, 4, (-1,))]
    assert D.encode_stream(fields, rows, None, ev) == R.encode_stream(fields, rows, None, ev)
    assert D.encode_stream(fields, rows, list(range(20)), ev) == R.encode_stream(fields, rows, list(range(20)), ev)


def test_reference_rows_parse_with_the_heap_snapshot_reader():
    """tests/heap_reader.ser_binrow_dec reads the accumulator rows heap_snapshot.cpp writes; it asserts the minimal
    length and the zero padding. Rows: [LONG, DECIMAL, LONG, DECIMAL]."""
    vals = boundary_values()
    rd = H.ser_binrow_dec(4, (1, 3))
    for i, v in enumerate(vals):
        w = None if i % 5 == 0 else vals[-1 - i]
        row = D.row_bytes(["LONG", "DECIMAL", "LONG", "DECIMAL"], (i, v, None if i % 3 == 0 else -i, w))
        kind, nulls, f = rd(H.Reader(struct.pack(">i", len(row)) + row))
        assert kind == 0 and nulls == [False, False, i % 3 == 0, w is None]
        assert f[0] == i and f[1] == v and (w is None or f[3] == w)
        if i % 3:
            assert f[2] == (-i) & ((1 << 64) - 1)


FIELDS = ["LONG", "DECIMAL", "STRING", "DECIMAL", "LONG"]


def _rows(n, seed=1):
    rng = np.random.default_rng(seed)
    vals = boundary_values()
    rows = []
    for i in range(n):
        a = vals[i % len(vals)]
        b = int(rng.integers(-(1 << 62), 1 << 62)) * int(rng.integers(1, 1 << 62))
        s = [None, "", "seven77", "eight888", "a-string-of-20-bytes"][i % 5]
        rows.append((i - 3, None if i % 4 == 1 else a, s, None if i % 7 == 2 else b, None if i % 6 == 0 else i * i))
    return rows


def _check_decoded(got, rows, cols):
    assert got["n_records"] == len(rows)
    for j, f in enumerate(cols):
        assert got["col_null"][j].tolist() == [int(r[f] is None) for r in rows]
        want = [0 if r[f] is None else r[f] for r in rows]
        if FIELDS[f] == "DECIMAL":
            assert got["cols"][j] == want
        else:
            assert got["cols"][j].view(np.int64).tolist() == want


@pytest.mark.parametrize("null_form", ["setnull", "write", "mixed"])
@pytest.mark.parametrize("dec_len", [None, 16, "mixed"])
def test_decoder_reference_reads_both_null_forms_and_any_length(null_form, dec_len):
    rows = _rows(150)
    nf = (lambda i: ("setnull", "write")[i % 2]) if null_form == "mixed" else null_form
    dl = (lambda i: (None, 9, 16, 3)[i % 4]) if dec_len == "mixed" else dec_len
    ev = [(0, 2, (1,)), (77, 4, (0,)), (150, 2, (99,))]
    data, starts = D.encode_stream(FIELDS, rows, None, ev, null_form=nf, dec_len=dl)
    rc, got = D.decode(FIELDS, data, key_field=0, cols=[1, 3, 4])
    assert rc == 0 and got["consumed"] == len(data)
    _check_decoded(got, rows, [1, 3, 4])
    assert got["key"].tolist() == [r[0] for r in rows]
    assert got["evt_pos"].tolist() == [0, 77, 150] and got["evt_tag"].tolist() == [2, 4, 2]
    o, b, z = got["strings"][2]
    assert z.tolist() == [int(r[2] is None) for r in rows]
    assert bytes(b) == b"".join(r[2].encode() for r in rows if r[2] is not None)
    # an unread DECIMAL field is skipped; decode_rows gives the tuples back
    rc, got = D.decode(FIELDS, data, key_field=0, cols=[3])
    assert rc == 0
    _check_decoded(got, rows, [3])
    back, events = D.decode_rows(FIELDS, data)
    assert back == [tuple(v.encode() if isinstance(v, str) else v for v in r) for r in rows]
    assert [(p, t) for p, t, _ in events] == [(0, 2), (77, 4), (150, 2)]
    # a cut inside a variable-length part ends the decode at the element before it
    cut = starts[100] + 40
    rc, got = D.decode(FIELDS, data[:cut], key_field=0, cols=[1])
    assert rc == 0 and got["consumed"] == starts[100] and got["n_records"] == 100


def corrupt_slot(data, start, fields, f, slot):
    """The stream with the slot of field f of the record element at `start` replaced (TAG_REC_WITHOUT_TIMESTAMP)."""
    at = start + 4 + 1 + 4 + D.W.nullbits_width(len(fields)) + 8 * f
    return data[:at] + struct.pack("<Q", slot) + data[at + 8:]


BAD_SLOTS = {                                                      # for a row of FIELDS: fixed part 48 bytes
    "len0": lambda size: (48 << 32) | 0,
    "len17": lambda size: (48 << 32) | 17,
    "off_in_fixed_part": lambda size: (47 << 32) | 1,
    "past_the_row": lambda size: ((size - 3) << 32) | 4,
    "offset_far_away": lambda size: (0x7FFFFFFF << 32) | 1,
}


@pytest.mark.parametrize("which", sorted(BAD_SLOTS))
def test_decoder_reference_refuses_bad_slots(which):
    rows = [r for r in _rows(40) if r[1] is not None and r[3] is not None][:12]
    data, starts = D.encode_stream(FIELDS, rows, None, [(12, 2, (5,))])
    i = 7
    size = len(D.row_bytes(FIELDS, rows[i]))
    bad = corrupt_slot(data, starts[i], FIELDS, 3, BAD_SLOTS[which](size))
    rc, got = D.decode(FIELDS, bad, key_field=0, cols=[1, 3])
    assert rc == D.E_CORRUPT and got["err_pos"] == starts[i]
    rc, got = D.decode(FIELDS, bad, key_field=0, cols=[1])        # no column reads the field: skipped, not checked
    assert rc == 0 and got["n_records"] == 12


def test_decoder_reference_accepts_what_the_reader_accepts():
    rows = [(1, 5, None, -7, 2), (2, None, None, None, 3)]
    data, starts = D.encode_stream(FIELDS, rows, None)
    # a NULL field with a garbage slot: the null bit is read first, the slot never
    for slot in (0xFFFFFFFFFFFFFFFF, 17, (5 << 32) | 1, (48 << 32) | 0):
        rc, got = D.decode(FIELDS, corrupt_slot(data, starts[1], FIELDS, 3, slot), key_field=0, cols=[1, 3])
        assert rc == 0 and got["cols"][1] == [-7, 0] and got["col_null"][1].tolist() == [0, 1]
    # 00 .. 01 in 16 bytes is 1; a value whose 16 reserved bytes would pass the row's end is still read
    row = bytearray(D.row_bytes(["DECIMAL"], (1,), dec_len=16))
    assert row[16:] == bytes(15) + b"\x01" and row[8:16] == struct.pack("<II", 16, 16)
    rc, got = D.decode(["DECIMAL", ], R.frame(bytes(row)), cols=[0])
    assert rc == 0 and got["cols"][0] == [1]
    short = bytes(row[:8]) + struct.pack("<II", 2, 16) + b"\xff\x7f"      # an 18-byte row: 2 value bytes, no padding
    rc, got = D.decode(["DECIMAL"], R.frame(short), cols=[0])
    assert rc == 0 and got["cols"][0] == [-129]


# ---- the schema checks, made before a device is touched ----
E_ARG, E_DEVICE, E_UNSUPPORTED = -1, -6, -7


def _create(schema):
    """fwa_wire_create's status; a decoder that came to life (a machine with a GPU) is destroyed again."""
    from flink_amd.engine import lib
    L = wire._bind(lib())
    h = C.c_void_p()
    rc = L.fwa_wire_create(C.byref(schema), C.byref(h))
    if rc == 0:
        L.fwa_wire_destroy(h)
    else:
        assert not h.value
    return rc


def test_decoder_create_refusals_and_acceptances():
    S = ["LONG", "DECIMAL", "LONG", "STRING"]
    passed = (0, E_DEVICE)                                         # the schema is fine: a device, or the lack of one
    assert _create(wire.make_schema(S, key_field=0, ts_field=2, cols=[1], fmt="ROWDATA")) in passed
    assert _create(wire.make_schema(S, key_field=0, ts_field=2, cols=[], fmt="ROWDATA")) in passed      # unread: skipped
    assert _create(wire.make_schema(S, key_field=-1, cols=[1, 0], fmt="ROWDATA")) in passed           # beside a STRING key
    assert _create(wire.make_schema(S[:3], key_field=0, cols=[1, 1], fmt="ROWDATA")) in passed
    assert _create(wire.make_schema(S, key_field=1, ts_field=2, fmt="ROWDATA")) == E_ARG               # as key_field
    assert _create(wire.make_schema(S, key_field=0, ts_field=1, fmt="ROWDATA")) == E_ARG               # as ts_field
    assert _create(wire.make_schema(S[:3], key_field=-1, cols=[1], fmt="ROWDATA")) == E_ARG            # -1 needs a STRING
    assert _create(wire.make_schema(S[:3], key_field=0, cols=[1], fmt="TUPLE")) == E_UNSUPPORTED       # BigDecSerializer
    assert _create(wire.make_schema(S[:3], key_field=0, fmt="TUPLE")) == E_UNSUPPORTED
    s = wire.make_schema(S, key_field=0, cols=[1], fmt="ROWDATA")
    for t in (5, 7):
        s.field[2] = t
        assert _create(s) == E_UNSUPPORTED                                                           # 5 stays unassigned


def _enc_create(fields, fmt="ROWDATA"):
    """(status, message) of fwa_wire_enc_create behind WireEncoder."""
    try:
        wire.WireEncoder(wire.make_out_schema(fields, fmt=fmt)).close()
    except Exception as e:                                         # EngineError
        return e.code, str(e)
    return 0, ""


def test_encoder_create_refusals_and_acceptances():
    row = [("LONG", "KEY"), ("DECIMAL", ("AGG", 0, "SUM_DEC128")), ("LONG", ("AGG", 1, "COUNT")),
           ("DECIMAL", ("AGG", 2, "AVG_DEC")), ("LONG", "WIN_START"), ("LONG", "WIN_END")]
    assert _enc_create(row)[0] in (0, E_DEVICE)
    for kind in A.DEC_KINDS:
        assert _enc_create([("DECIMAL", ("AGG", 3, kind)), ("STRING", ("KEYCOL", 0, "STRING"))])[0] in (0, E_DEVICE)
        code, msg = _enc_create([("LONG", "KEY"), ("LONG", ("AGG", 0, kind))])
        assert code == E_UNSUPPORTED and "DECIMAL" in msg and "FWA_FIELD_DECIMAL only" in msg
        code, msg = _enc_create([("DOUBLE", ("AGG", 0, kind))], fmt="TUPLE")
        assert code == E_UNSUPPORTED and "DECIMAL" in msg
        code, msg = _enc_create([("LONG", "KEY"), ("DECIMAL", ("AGG", 0, kind))], fmt="TUPLE")
        assert code == E_ARG and "ROWDATA rows only" in msg
    # a DECIMAL wire type over another source: make_out_schema refuses the pair, and so does the library
    s = wire.make_out_schema(row, fmt="ROWDATA")
    for src, kind, what in [(wire.SOURCES["KEY"], 0, "an int64"), (wire.SOURCES["WIN_END"], 0, "an int64"),
                            (wire.SOURCES["AGG"], A.AGG_KINDS["SUM_F64"], "a double"),
                            (wire.SOURCES["AGG"], A.AGG_KINDS["SUM_I32"], "an int32"),
                            (wire.SOURCES["KEYCOL"], wire.KEY_FIELD["STRING"], "a STRING")]:
        s.src[1], s.src_kind[1] = src, kind
        with pytest.raises(Exception) as ei:
            wire.WireEncoder(s)
        assert ei.value.code == E_ARG and (what + " source cannot be written as DECIMAL") in str(ei.value), str(ei.value)
    s = wire.make_out_schema(row, fmt="ROWDATA")
    s.field[2] = 5
    with pytest.raises(Exception) as ei:
        wire.WireEncoder(s)
    assert ei.value.code == E_ARG and "unknown field type" in str(ei.value)


def test_make_out_schema_pairs_decimal_with_decimal_aggregates():
    s = wire.make_out_schema([("DECIMAL", ("AGG", 2, "AVG_DEC128")), ("LONG", "KEY")], fmt="ROWDATA")
    assert (s.field[0], s.src[0], s.src_index[0], s.src_kind[0]) == (6, 5, 2, 17)
    for kind in A.DEC_KINDS:
        assert wire.make_out_schema([("DECIMAL", ("AGG", 0, kind))], fmt="ROWDATA").src_kind[0] == A.AGG_KINDS[kind]
    for src in ["KEY", "WIN_END", ("AGG", 0, "SUM_I64"), ("AGG", 0, "COUNT"), ("KEYCOL", 0, "STRING"), ("AGG", 0)]:
        with pytest.raises(ValueError, match="wire type"):
            wire.make_out_schema([("DECIMAL", src)], fmt="ROWDATA")
    with pytest.raises(ValueError, match="DECIMAL aggregate"):
        wire.make_out_schema([("DECIMAL", "KEY")])
    assert wire.make_schema(["LONG", "DECIMAL"], key_field=0, cols=[1], fmt="ROWDATA").field[1] == 6
