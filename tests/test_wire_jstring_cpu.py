"""CPU checks around java.lang.String fields on the wire (FWA_FIELD_JSTRING): the reference sender / receiver the GPU is
judged by (tests/wire_jstring_ref.py) and flink_amd.wire's host helpers against hand-derived byte and hashCode() literals
and against the reference's own bytes (a TupleSerializer(StringSerializer, IntSerializer) state value in a Flink 1.18
checkpoint); then the schema checks of fwa_wire_create / fwa_wire_enc_create, made before a device is touched, and
NetworkInput's argument errors."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from flink_amd import _abi as A
from flink_amd import wire
from flink_amd.engine import EngineError

import heap_reader as H
import wire_jstring_ref as J
import wire_strings_ref as R

E_ARG, E_DEVICE, E_UNSUPPORTED, E_CORRUPT = -1, -6, -7, -9

SMILE = "\U0001F600"
TABLE = [("key1", "05 6b 65 79 31", 3288498), ("", "01", 0), ("é€", "03 e9 01 ac 41", 15587),
         (SMILE, "03 bd b0 03 80 bc 03", 1772899), ("\uffff", "02 ff ff 03", 65535)]


def test_field_value():
    assert wire.FIELDS["JSTRING"] == 8
    assert 5 not in wire.FIELDS.values() and 7 not in wire.FIELDS.values()
    assert J.EVENT_BODY == R.EVENT_BODY and J.MAX_BODY == R.MAX_BODY


def test_table_literals_bytes_and_hashes():
    for s, hexs, h in TABLE:
        b = bytes.fromhex(hexs)
        assert J.jstring(s) == b, (s, J.jstring(s).hex())
        assert wire.jstring_field(s) == b
        assert wire.jstring_bytes(s) == b[1:] == J.char_bytes(s)
        assert J.java_hash(s) == h, (s, J.java_hash(s))
    a127 = "a" * 127
    assert J.jstring(a127)[:4] == bytes.fromhex("80 01 61 61") and len(J.jstring(a127)) == 2 + 127
    assert wire.jstring_field(a127) == J.jstring(a127)
    assert J.jstring("a" * 126)[:2] == bytes.fromhex("7f 61") and len(J.jstring("a" * 126)) == 1 + 126
    assert J.java_hash(a127) == -1374877567
    assert J.java_hash("polygenelubricants") == -2147483648
    assert J.java_hash("Aa") == 2112 and J.java_hash("BB") == 2112
    assert J.jstring(None) == b"\x00" == wire.jstring_field(None)
    # the length prefix grows to three bytes at 16383 chars (len + 1 = 2^14)
    assert J.jstring("x" * 16382)[:3] == bytes.fromhex("ff 7f 78") and J.jstring("x" * 16383)[:4] == bytes.fromhex("80 80 01 78")


def test_code_unit_count_is_the_bytes_below_0x80():
    for s in ["", "key1", "é€", SMILE, "\uffff\u0080\u3fff\u4000", "\ud800", "a\udc00b"]:
        b = J.char_bytes(s)
        assert sum(1 for x in b if x < 0x80) == len(J.units(s))


def test_jstring_bytes_text_round_trip():
    rng = np.random.default_rng(5)
    vals = ["", "key1", "é€", SMILE, "\uffff", "\x00", "\x7f\x80", "\u3fff\u4000", "\ud83d", "\ude00", "x\udfffy\ud800",
            "polygenelubricants"]
    for _ in range(200):
        n = int(rng.integers(0, 40))
        us = rng.integers(0, 0x10000, n).tolist()                  # any code units, lone surrogates included
        vals.append(b"".join(struct.pack("<H", u) for u in us).decode("utf-16-le", "surrogatepass"))
    for s in vals:
        b = wire.jstring_bytes(s)
        assert b == J.char_bytes(s)
        assert wire.jstring_text(b) == s == J.text_of(b)
    assert wire.jstring_bytes("key1") == b"key1"                   # ASCII: the text itself
    for bad in (b"\x80\x00", b"\x80\x80\x04", b"\x80\x80\x80\x01", b"\x80"):
        with pytest.raises(ValueError):
            wire.jstring_text(bad)


def test_reference_snapshot_holds_the_reference_encoders_bytes():
    """The state values of the reference's window-operator migration checkpoint are Tuple2<String, Integer> written by
    TupleSerializer(StringSerializer, IntSerializer): the bytes of the wire value. Each, re-encoded, occurs in the file."""
    f = os.path.join(os.path.dirname(__file__), "golden", "flink_snapshots",
                     "win-op-migration-test-reduce-event-time-flink1.18-snapshot")
    blob = open(f, "rb").read()
    first, offs, data = H.read_operator_snapshot(blob)[0]
    lay = {0: ("kv", H.ser_time_window, H.ser_string, H.ser_tuple(H.ser_string, H.ser_int)),
           1: ("pq", H.ser_string, H.ser_time_window), 2: ("pq", H.ser_string, H.ser_time_window)}
    sec = H.read_key_groups(data, offs, first, lay)[0]
    assert len(sec[0]) >= 3
    seen = set()
    for (_st, _en), key, (k2, v) in sec[0]:
        assert k2 == key
        enc = J.value_bytes(["JSTRING", "INT"], (key, v))
        assert enc == J.jstring(key) + struct.pack(">i", v)
        assert enc in blob, (key, v)
        seen.add(key)
    assert seen == {"key1", "key2"}
    assert J.jstring("key1") == bytes.fromhex("05 6b 65 79 31")


def test_reference_decoder_on_its_own_streams():
    fields = ["LONG", "JSTRING", "INT", "DOUBLE"]
    rows = [(7, "key1", -3, 1.5), (8, None, 4, -0.0), (9, "", 5, 2.0), (-1, "é€" + SMILE, 6, 3.0)]
    for ts in (None, [10, 20, 30, 40]):
        data, starts = J.encode_stream(fields, rows, ts, events=[(1, 2, (99,)), (4, 4, (-1,))])
        rc, got = J.decode(fields, data, cols=[0, 2, 3])
        assert rc == 0 and got["n_records"] == 4 and got["n_events"] == 2 and got["consumed"] == len(data)
        assert got["ts"].tolist() == (ts or [J.LONG_MIN] * 4)
        assert got["cols"][0].astype(np.int64).tolist() == [7, 8, 9, -1]
        assert got["cols"][1].astype(np.int64).tolist() == [-3, 4, 5, 6]
        o, b, z = got["strings"][1]
        assert z.tolist() == [0, 1, 0, 0]
        assert [J.text_of(bytes(b[o[i]:o[i + 1]])) for i in range(4)] == ["key1", "", "", "é€" + SMILE]
        assert got["evt_pos"].tolist() == [1, 4] and got["evt_tag"].tolist() == [2, 4]
        for cut in range(len(data)):                               # any prefix decodes to whole elements and stops
            rc, part = J.decode(fields, data[:cut], cols=[0])
            assert rc == 0 and part["consumed"] <= cut
    # the corrupt forms, each at its element
    ok = J.frame(J.value_bytes(["JSTRING", "LONG"], ("ab", 1)))
    for raw in (b"\x05ab", b"\x02ab", b"\x02\x80\x80\x80\x01", b"\x02\x80\x80\x04", b"\x80\x00", b"\x02\x80\x00"):
        data = ok + J.frame(J.value_bytes(["JSTRING", "LONG"], (raw, 1))) + ok
        rc, got = J.decode(["JSTRING", "LONG"], data)
        assert rc == E_CORRUPT and got["err_pos"] == len(ok), raw
    big = J.frame(J.value_bytes(["JSTRING"], ("a" * 247,)))        # tag + length varint (2) + 247 = 250
    assert len(big) == 4 + 250
    assert J.decode(["JSTRING"], ok[:0] + big)[0] == E_UNSUPPORTED
    fit = J.frame(J.value_bytes(["JSTRING"], ("a" * 246,)))
    assert len(fit) == 4 + 249 and J.decode(["JSTRING"], fit)[0] == 0


# ---- the schema checks, made before a device is touched ----
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
    passed = (0, E_DEVICE)                                         # the schema is fine: a device, or the lack of one
    assert _create(wire.make_schema(["JSTRING", "LONG"], key_field=-1, cols=[1])) in passed
    assert _create(wire.make_schema(["LONG", "JSTRING", "INT", "DOUBLE"], key_field=-1, cols=[0, 2, 3])) in passed
    assert _create(wire.make_schema(["JSTRING", "JSTRING", "FLOAT"], key_field=-1, cols=[2])) in passed
    assert _create(wire.make_schema(["LONG", "JSTRING"], key_field=-1, ts_field=0)) in passed
    assert _create(wire.make_schema(["JSTRING"] * 16, key_field=-1)) in passed
    assert _create(wire.make_schema(["JSTRING", "LONG"], key_field=-1, cols=[1], fmt="ROWDATA")) == E_UNSUPPORTED
    assert _create(wire.make_schema(["JSTRING", "LONG"], key_field=0, cols=[1])) == E_ARG             # as key_field
    assert _create(wire.make_schema(["JSTRING", "LONG"], key_field=1)) == E_ARG                       # key_field is -1
    assert _create(wire.make_schema(["JSTRING", "LONG"], key_field=-1, ts_field=0)) == E_ARG          # as ts_field
    assert _create(wire.make_schema(["JSTRING", "LONG"], key_field=-1, cols=[0])) == E_ARG            # as a value column
    # nothing existing changes: STRING in a TUPLE, and the unassigned values
    assert _create(wire.make_schema(["STRING", "LONG"], key_field=-1, cols=[1])) == E_UNSUPPORTED
    assert _create(wire.make_schema(["STRING", "JSTRING", "LONG"], key_field=-1, cols=[2])) == E_UNSUPPORTED
    s = wire.make_schema(["JSTRING", "LONG", "LONG"], key_field=-1, cols=[1])
    for t in (5, 7, 9):
        s.field[2] = t
        assert _create(s) == E_UNSUPPORTED


def _enc_create(fields, fmt="TUPLE", record_ts=None):
    try:
        wire.WireEncoder(wire.make_out_schema(fields, fmt=fmt, record_ts=record_ts)).close()
    except EngineError as e:
        return e.code, str(e)
    return 0, ""


def test_encoder_create_refusals_and_acceptances():
    key = ("JSTRING", ("KEYCOL", 0, "STRING"))
    passed = (0, E_DEVICE)
    assert _enc_create([key, ("LONG", ("AGG", 0, "COUNT"))])[0] in passed
    assert _enc_create([("LONG", ("AGG", 0, "COUNT")), key, ("INT", ("AGG", 1, "SUM_I64")), ("LONG", "WIN_END")],
                       record_ts="WIN_TIME")[0] in passed
    assert _enc_create([key, ("JSTRING", ("KEYCOL", 1, "STRING"))])[0] in passed
    code, msg = _enc_create([key, ("LONG", "KEY")], fmt="ROWDATA")
    assert code == E_ARG and "TUPLE values only" in msg
    for src, what in [("KEY", "an int64"), ("WIN_END", "an int64"), (("AGG", 0, "COUNT"), "an int64"),
                      (("AGG", 0, "SUM_F64"), "a double"), (("KEYCOL", 0, "BIGINT"), "an int64"),
                      (("KEYCOL", 0, "INT"), "an int32"), (("KEYCOL", 0, "DOUBLE"), "a double")]:
        code, msg = _enc_create([("JSTRING", src)])
        assert code == E_ARG and (what + " source cannot be written as JSTRING") in msg, msg
    # FWA_FIELD_STRING in a TUPLE value stays refused with its message; 5 and 7 stay unknown
    code, msg = _enc_create([("LONG", "KEY"), ("STRING", ("KEYCOL", 0, "STRING"))])
    assert code == E_ARG and "STRING fields are written in ROWDATA rows only" in msg
    s = wire.make_out_schema([key, ("LONG", "KEY")])
    for t in (5, 7):
        s.field[1] = t
        with pytest.raises(EngineError) as ei:
            wire.WireEncoder(s)
        assert ei.value.code == E_ARG and "unknown field type" in str(ei.value)
    o = wire.make_out_schema([key])
    assert (o.field[0], o.src[0], o.src_index[0], o.src_kind[0]) == (8, 1, 0, 3)


class _Cfg:
    def __init__(self, key_kind):
        self.key_kind = key_kind


class _Engine:
    def __init__(self, key_kind):
        self.cfg = _Cfg(key_kind)


class _Dict:
    def __init__(self, types):
        self.types = types


def test_network_input_argument_errors():
    """Raised before anything native is created, so they need no device."""
    sc = wire.make_schema(["JSTRING", "LONG"], key_field=-1, cols=[1])
    pre, d = _Engine(A.KEY_PREHASHED), _Dict([wire.KEY_FIELD["STRING"]])

    def err(*a, **kw):
        with pytest.raises(EngineError) as ei:
            wire.NetworkInput(*a, **kw)
        assert ei.value.code == -1
        return str(ei.value)

    assert "exclude each other" in err(sc, pre, keydict=d, key_parts=[("str", 0)], key_string=0)
    assert "needs keydict" in err(sc, pre, key_string=0)
    assert "one field" in err(sc, pre, keydict=_Dict([3, 0]), key_string=0)
    assert "one field" in err(sc, pre, keydict=_Dict([0]), key_string=0)
    assert "JSTRING field" in err(sc, pre, keydict=d, key_string=1)
    assert "JSTRING field" in err(sc, pre, keydict=d, key_string=2)
    rd = wire.make_schema(["STRING", "LONG"], key_field=-1, cols=[1], fmt="ROWDATA")
    assert "JSTRING field" in err(rd, pre, keydict=d, key_string=0)
    for kind in (A.KEY_JAVA_LONG, A.KEY_BINROW_BIGINT, A.KEY_GROUP_PREFIXED):
        assert "KEY_PREHASHED" in err(sc, _Engine(kind), keydict=d, key_string=0)
    assert "go together" in err(sc, pre, keydict=d)                # as before: keydict without key_parts
