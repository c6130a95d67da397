"""STRING fields on the wire, without a GPU: the test-side encoder against hand-written bytes (row sizes as pinned in
tests/test_keydict_cpu.py: 16 bytes for one inline field, 24 for an 8-byte value), the sequential reference decoder on
random streams and on every refusal, and the schema refusals of fwa_wire_create (validation runs before the device is
touched)."""
import ctypes as C
import struct

import numpy as np
import pytest

from flink_amd import wire

import wire_strings_ref as R

F3 = ["STRING", "LONG", "STRING"]


def be(v, n):
    return (v & ((1 << (8 * n)) - 1)).to_bytes(n, "big")


def le(v, n=8):
    return (v & ((1 << (8 * n)) - 1)).to_bytes(n, "little")


def test_encoder_matches_hand_written_bytes():
    """(inline 'abc', BIGINT 7, 8-byte '12345678') with a StreamRecord timestamp, then (NULL, -1, '') without one."""
    row = (bytes(8)                                   # RowKind INSERT, no null bits
           + b"abc" + bytes(4) + b"\x83"              # inline: bytes from the lowest, 0x80 | 3 on top
           + le(7)
           + le((32 << 32) | 8)                       # variable part starts after 8 + 3 * 8 bytes
           + b"12345678")
    assert len(row) == 40
    lit = be(1 + 8 + 4 + 40, 4) + b"\x00" + be(77, 8) + be(40, 4) + row
    data, starts = R.encode_stream(F3, [("abc", 7, "12345678")], ts=[77])
    assert data == lit and starts == [0]
    row2 = (b"\x00\x01" + bytes(6)                    # null bit of field 0 = bit 8 (byte 1, bit 0)
            + bytes(8) + le(-1) + bytes(7) + b"\x80")
    lit2 = be(1 + 4 + 32, 4) + b"\x01" + be(32, 4) + row2
    data2, _ = R.encode_stream(F3, [(None, -1, "")])
    assert data2 == lit2
    # sizes of tests/test_keydict_cpu.py: one inline field 16 bytes, an 8-byte value 24
    assert len(R.row_bytes(["STRING"], ("1234567",))) == 16 and len(R.row_bytes(["STRING"], ("12345678",))) == 24
    rc, r = R.decode(F3, lit + R.W.encode_event(2, (13,)) + lit2, key_field=1)
    assert rc == 0 and r["consumed"] == len(lit) + 13 + len(lit2)
    assert r["ts"].tolist() == [77, R.LONG_MIN] and r["key"].tolist() == [7, -1]
    o, b, z = r["strings"][0]
    assert o.tolist() == [0, 3, 3] and b.tobytes() == b"abc" and z.tolist() == [0, 1]
    o, b, z = r["strings"][2]
    assert o.tolist() == [0, 8, 8] and b.tobytes() == b"12345678" and z.tolist() == [0, 0]
    assert r["evt_pos"].tolist() == [1] and r["evt_val"][0, 0] == 13


def random_rows(rng, fields, n, null_p=0.1, max_len=40):
    rows = []
    for _ in range(n):
        r = []
        for f in fields:
            if rng.random() < null_p:
                r.append(None)
            elif f == "STRING":
                r.append(bytes(rng.integers(0, 256, int(rng.integers(0, max_len + 1)), dtype=np.uint8)))
            elif f == "DOUBLE":
                r.append(float(rng.standard_normal()))
            elif f == "INT":
                r.append(int(rng.integers(-2**31, 2**31)))
            else:
                r.append(int(rng.integers(-2**62, 2**62)))
        rows.append(tuple(r))
    return rows


@pytest.mark.parametrize("seed", range(4))
def test_reference_decoder_round_trips_random_streams(seed):
    rng = np.random.default_rng(seed)
    fields = [["STRING", "LONG"], ["LONG", "STRING", "INT", "STRING"], ["STRING", "DOUBLE", "LONG"], F3][seed]
    n = 300
    rows = random_rows(rng, fields, n)
    ts = rng.integers(-2**40, 2**40, n) if seed % 2 else None
    events = [(int(p), 2, (int(rng.integers(-2**60, 2**60)),)) for p in np.sort(rng.integers(0, n + 1, 7))]
    events.insert(3, (events[3][0], 3, (5, -1, -2, 9)))
    data, starts = R.encode_stream(fields, rows, ts, events)
    nums = [f for f, t in enumerate(fields) if t in ("LONG", "INT")]
    rc, r = R.decode(fields, data, cols=nums)
    assert rc == 0 and r["consumed"] == len(data) and r["n_records"] == n and r["n_events"] == 8
    assert r["key"] is None and (ts is None or r["ts"].tolist() == ts.tolist())
    for f, t in enumerate(fields):
        if t != "STRING":
            continue
        o, b, z = r["strings"][f]
        raw = b.tobytes()
        assert z.tolist() == [int(x[f] is None) for x in rows]
        assert [raw[o[i]:o[i + 1]] for i in range(n)] == [x[f] or b"" for x in rows]
    for j, f in enumerate(nums):
        assert r["col_null"][j].tolist() == [int(x[f] is None) for x in rows]
        assert r["cols"][j].astype(np.int64).tolist() == [0 if x[f] is None else x[f] for x in rows]
    assert r["evt_pos"].tolist() == [e[0] for e in events] and r["evt_val"][3].tolist() == [5, -1, -2, 9]
    # a cut anywhere leaves whole elements and a tail that the next call completes
    for cut in rng.integers(1, len(data), 40).tolist() + [len(data) - 1, starts[-1] + 20]:
        rc, a = R.decode(fields, data[:cut])
        assert rc == 0 and a["consumed"] <= cut
        rc, b2 = R.decode(fields, data[a["consumed"]:])
        assert rc == 0 and a["n_records"] + b2["n_records"] == n and a["n_events"] + b2["n_events"] == 8


def test_reference_decoder_refusals():
    fields = ["STRING", "LONG"]
    good, starts = R.encode_stream(fields, [("k%d" % i * 5, i) for i in range(20)])
    at = starts[10]

    def spliced(elem):
        return good[:at] + elem + good[at:]

    fixed = 8 + 16
    long_row = R.row_bytes(fields, ("x" * 216, 1))                              # L = 5 + 24 + 216 = 245: fits
    assert R.decode(fields, spliced(R.frame(long_row)))[0] == 0
    rc, r = R.decode(fields, spliced(R.frame(R.row_bytes(fields, ("x" * 224, 1)))))   # L = 253
    assert (rc, r["err_pos"]) == (R.E_UNSUPPORTED, at)
    e = bytearray(R.frame(long_row))
    e[5 + 3] ^= 8                                                               # the size int, not L
    rc, r = R.decode(fields, spliced(bytes(e)))
    assert (rc, r["err_pos"]) == (R.E_CORRUPT, at)
    row = bytearray(R.row_bytes(fields, ("x" * 16, 1)))
    row[8:16] = struct.pack("<Q", (fixed << 32) | 17)                           # off + len > size
    rc, r = R.decode(fields, spliced(R.frame(bytes(row))))
    assert (rc, r["err_pos"]) == (R.E_CORRUPT, at)
    row[8:16] = struct.pack("<Q", ((fixed - 8) << 32) | 8)                      # off < fixed
    assert R.decode(fields, spliced(R.frame(bytes(row))))[0] == R.E_CORRUPT
    row[8:16] = struct.pack("<Q", (0x89 << 56) | 0x41)                          # inline length 9
    assert R.decode(fields, spliced(R.frame(bytes(row))))[0] == R.E_CORRUPT
    row[8:16] = struct.pack("<Q", (fixed << 32) | 3)                            # a short value in the variable part
    rc, r = R.decode(fields, spliced(R.frame(bytes(row))))
    assert rc == 0 and r["strings"][0][1].tobytes()[r["strings"][0][0][10]:r["strings"][0][0][11]] == b"xxx"
    row = bytearray(R.row_bytes(fields, ("abc", 1)))
    row[0] = 1                                                                  # RowKind UPDATE_BEFORE
    assert R.decode(fields, spliced(R.frame(bytes(row))))[0] == R.E_UNSUPPORTED


def _create(schema):
    from flink_amd.engine import lib
    L = wire._bind(lib())
    h = C.c_void_p()
    rc = L.fwa_wire_create(C.byref(schema), C.byref(h))
    assert rc != 0 and not h.value
    return rc


def test_create_refusals_without_gpu():
    S = ["STRING", "LONG", "LONG"]
    assert wire.FIELDS["STRING"] == 4
    assert _create(wire.make_schema(S, key_field=1, fmt="TUPLE")) == -7           # StringSerializer: another feature
    assert _create(wire.make_schema(S, key_field=-1, fmt="TUPLE")) == -7
    assert _create(wire.make_schema(S, key_field=0, ts_field=1, fmt="ROWDATA")) == -1     # STRING as key_field
    assert _create(wire.make_schema(S, key_field=1, ts_field=0, fmt="ROWDATA")) == -1     # ... as ts_field
    assert _create(wire.make_schema(S, key_field=1, ts_field=2, cols=[0], fmt="ROWDATA")) == -1   # ... as a column
    assert _create(wire.make_schema(["LONG", "LONG"], key_field=-1, fmt="ROWDATA")) == -1  # -1 needs a STRING field
    assert _create(wire.make_schema(S, key_field=-2, fmt="ROWDATA")) == -1
    s = wire.make_schema(S, key_field=1, fmt="ROWDATA")
    s.field[2] = 7
    assert _create(s) == -7                                                       # unknown types stay unsupported
    s.field[2] = 5
    assert _create(s) == -7
    # 16 fields: the fixed part alone is 16 + 128 bytes, still below the ceiling; the refusal is about the type
    s = wire.make_schema(["STRING"] * 16, key_field=-1, fmt="ROWDATA")
    s.field[3] = -1
    assert _create(s) == -7
