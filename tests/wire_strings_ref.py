"""TEST INFRASTRUCTURE ONLY: sender and sequential receiver of wire streams whose BinaryRowData rows carry STRING
fields (include/flink_amd_wire.h FWA_FIELD_STRING).

The encoder frames `oracle.oracle.binrow_bytes` rows (layout pinned against the reference's BinaryRowDataTest sizes in
tests/test_keydict_cpu.py) as BinaryRowDataSerializer / StreamElementSerializer / RecordWriter do:
    be32 L | tag | [be64 ts] | be32 size | row[size]            L = 1 (+ 8) + 4 + size
and takes non-record elements from `oracle.wire_encode.encode_event`.

The decoder is a plain loop over the bytes with the accept rules of the header, in this order per element at p:
    fewer than 5 bytes left                               -> END (the element continues in the next buffer)
    tag 2..5: L != the tag's body length                  -> CORRUPT; element past the end -> END
    tag > 5                                               -> CORRUPT
    tag 0 / 1: L < header + fixed part                    -> CORRUPT
               the size int is past the end               -> END
               size int != L - header                     -> CORRUPT
               L > 249                                    -> UNSUPPORTED (the ceiling; never CORRUPT)
               element past the end                       -> END
               RowKind byte != 0                          -> UNSUPPORTED
    per record: NULL rowtime field -> ARG; per non-NULL STRING slot: top bit set -> inline, length (slot >> 56) & 0x7f
    must be <= 7; else offset = slot >> 32, length = slot & 0xffffffff with fixed <= offset and offset + length <= size,
    anything else -> CORRUPT. Every error carries the byte position of its element.
"""
import struct

import numpy as np

from oracle import oracle as O
from oracle import wire_encode as W

OK, E_ARG, E_UNSUPPORTED, E_CORRUPT = 0, -1, -7, -9
MAX_BODY = 249
LONG_MIN = -(1 << 63)
EVENT_BODY = {2: 9, 3: 29, 4: 5, 5: 2}
_BINROW_TYPE = {"LONG": "BIGINT", "INT": "INT", "DOUBLE": "DOUBLE", "FLOAT": "INT", "STRING": "STRING"}


def row_bytes(fields, row):
    """BinaryRowData bytes of one row (values: int / float / str / bytes / None per field)."""
    vals = []
    for f, v in zip(fields, row):
        if f == "FLOAT" and v is not None:
            v = struct.unpack("<I", struct.pack("<f", v))[0]       # the float's bits in the slot's low half
        vals.append(v)
    return O.binrow_bytes([_BINROW_TYPE[f] for f in fields], tuple(vals))


def frame(rb, ts=None):
    """One record element around the row bytes rb."""
    body = (b"\x00" + struct.pack(">q", ts) if ts is not None else b"\x01") + struct.pack(">i", len(rb)) + rb
    return struct.pack(">I", len(body)) + body


def encode_stream(fields, rows, ts=None, events=()):
    """rows: tuples; ts: StreamRecord timestamps or None; events: (pos, tag, vals) sorted by pos, written before
    record `pos`. Returns the bytes and the byte offset of every record element."""
    out, starts, at, evs = [], [], 0, list(events)
    ei = 0
    for i, r in enumerate(rows):
        while ei < len(evs) and evs[ei][0] <= i:
            e = W.encode_event(evs[ei][1], evs[ei][2])
            out.append(e)
            at += len(e)
            ei += 1
        e = frame(row_bytes(fields, r), None if ts is None else int(ts[i]))
        starts.append(at)
        out.append(e)
        at += len(e)
    for _, tag, vals in evs[ei:]:
        out.append(W.encode_event(tag, vals))
    return b"".join(out), starts


def decode(fields, data, key_field=-1, ts_field=-1, cols=()):
    """Sequential decode. Returns (0, result dict) or (error code, {"err_pos": byte offset of the element})."""
    data = bytes(data)
    n = len(data)
    arity = len(fields)
    nb = W.nullbits_width(arity)
    fixed = nb + 8 * arity
    sf = [f for f in range(arity) if fields[f] == "STRING"]
    key, key_null, tss = [], [], []
    colv = [[] for _ in cols]
    coln = [[] for _ in cols]
    strs = {f: ([0], bytearray(), []) for f in sf}
    evt_pos, evt_tag, evt_val = [], [], []
    p = 0

    def isnull(row, f):
        bit = f + 8
        return (data[row + (bit >> 3)] >> (bit & 7)) & 1

    def slot(row, f):
        return int.from_bytes(data[row + nb + 8 * f: row + nb + 8 * f + 8], "little")

    while True:
        if p + 5 > n:
            break
        L = int.from_bytes(data[p:p + 4], "big")
        t = data[p + 4]
        if t > 5:
            return E_CORRUPT, {"err_pos": p}
        if t >= 2:
            if L != EVENT_BODY[t]:
                return E_CORRUPT, {"err_pos": p}
            if p + 4 + L > n:
                break
            q = p + 5
            v = [0, 0, 0, 0]
            if t == 2:
                v[0] = struct.unpack(">q", data[q:q + 8])[0]
            elif t == 4:
                v[0] = struct.unpack(">i", data[q:q + 4])[0]
            elif t == 3:
                v = list(struct.unpack(">qqqi", data[q:q + 28]))
            else:
                v[0] = int(data[q] != 0)
            evt_pos.append(len(tss))
            evt_tag.append(t)
            evt_val.append(v)
            p += 4 + L
            continue
        hdr = 13 if t == 0 else 5
        if L < hdr + fixed:
            return E_CORRUPT, {"err_pos": p}
        if p + 4 + hdr > n:
            break
        size = int.from_bytes(data[p + hdr:p + hdr + 4], "big")
        if size != L - hdr:
            return E_CORRUPT, {"err_pos": p}
        if L > MAX_BODY:
            return E_UNSUPPORTED, {"err_pos": p}
        if p + 4 + L > n:
            break
        row = p + 4 + hdr
        if data[row] != 0:
            return E_UNSUPPORTED, {"err_pos": p}
        if ts_field >= 0:
            if isnull(row, ts_field):
                return E_ARG, {"err_pos": p}
            v = slot(row, ts_field)
            tv = v - (1 << 64) if v >> 63 else v
            if fields[ts_field] == "INT":
                tv = struct.unpack("<i", struct.pack("<I", v & 0xFFFFFFFF))[0]
        else:
            tv = struct.unpack(">q", data[p + 5:p + 13])[0] if t == 0 else LONG_MIN
        got = {}
        for f in sf:
            if isnull(row, f):
                got[f] = (b"", 1)
                continue
            s = slot(row, f)
            if s >> 63:
                ln = (s >> 56) & 0x7F
                if ln > 7:
                    return E_CORRUPT, {"err_pos": p}
                got[f] = (data[row + nb + 8 * f: row + nb + 8 * f + ln], 0)
            else:
                off, ln = s >> 32, s & 0xFFFFFFFF
                if off < fixed or off + ln > size:
                    return E_CORRUPT, {"err_pos": p}
                got[f] = (data[row + off: row + off + ln], 0)
        tss.append(tv)
        if key_field >= 0:
            kn = isnull(row, key_field)
            key_null.append(kn)
            v = slot(row, key_field)
            if fields[key_field] == "INT":
                v = struct.unpack("<i", struct.pack("<I", v & 0xFFFFFFFF))[0]
            elif v >> 63:
                v -= 1 << 64
            key.append(0 if kn else v)
        for j, f in enumerate(cols):
            coln[j].append(isnull(row, f))
            v = slot(row, f)
            if fields[f] == "INT":
                v = struct.unpack("<i", struct.pack("<I", v & 0xFFFFFFFF))[0] & 0xFFFFFFFFFFFFFFFF
            elif fields[f] == "FLOAT":
                v &= 0xFFFFFFFF
            colv[j].append(v)
        for f in sf:
            b, z = got[f]
            strs[f][1].extend(b)
            strs[f][0].append(len(strs[f][1]))
            strs[f][2].append(z)
        p += 4 + L
    res = {"n_records": len(tss), "n_events": len(evt_pos), "consumed": p,
           "ts": np.array(tss, np.int64),
           "key": np.array(key, np.int64) if key_field >= 0 else None,
           "key_null": np.array(key_null, np.uint8) if key_field >= 0 else None,
           "cols": [np.array(c, np.uint64).astype(np.uint32) if fields[f] == "FLOAT" else np.array(c, np.uint64)
                    for c, f in zip(colv, cols)],
           "col_null": [np.array(c, np.uint8) for c in coln],
           "strings": {f: (np.array(o, np.int32), np.frombuffer(bytes(b), np.uint8), np.array(z, np.uint8))
                       for f, (o, b, z) in strs.items()},
           "evt_pos": np.array(evt_pos, np.int64), "evt_tag": np.array(evt_tag, np.int32),
           "evt_val": np.array(evt_val, np.int64).reshape(-1, 4)}
    return OK, res
