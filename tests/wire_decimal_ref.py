"""TEST INFRASTRUCTURE ONLY: sender and sequential receiver of wire streams whose BinaryRowData rows carry non-compact
DECIMAL fields (precision > 18; include/flink_amd_wire.h FWA_FIELD_DECIMAL) beside LONG / INT / DOUBLE / FLOAT / STRING
fields. Built on tests/wire_strings_ref.py (framing, events, status codes); values are Python ints or None, through
int.to_bytes / int.from_bytes.

A non-NULL DECIMAL field (AbstractBinaryWriter.writeDecimal :164-196): 16 bytes are reserved at the writer's cursor in
the row's variable-length part and zeroed, DecimalData.toUnscaledBytes() -- BigInteger.toByteArray, the minimal
big-endian two's complement, bitLength / 8 + 1 bytes -- is copied to their start, the slot is offset << 32 | length and
the cursor advances by 16. Variable-length parts follow the fixed part in field order, so they interleave with the
8-rounded parts of STRING values longer than 7 bytes.

NULL has two forms: null_form="setnull" is RowDataSerializer.toBinaryRow (:196-212) calling setNullAt -- the bit, a zero
slot, nothing reserved; null_form="write" is writeDecimal(pos, null, precision) -- the bit, slot = cursor << 32 | 0 and
16 zero bytes reserved.

The decoder restates wire_strings_ref.decode's element-level checks in their order, and per record: NULL rowtime field
-> ARG; the STRING slots as there; then per non-NULL DECIMAL slot offset = slot >> 32, length = slot & 0xffffffff with
fixed <= offset, offset + length <= size and 1 <= length <= 16, anything else -> CORRUPT (a zero-length BigInteger
throws in the reference; more than 16 bytes is outside DECIMAL(38)). The slot of a NULL field is never interpreted, the
length need not be minimal and offset + 16 may pass the row's end: BinarySegmentUtils.readDecimalData ->
DecimalData.fromUnscaledBytes -> new BigInteger(bytes) asks for neither. Every error carries the byte position of its
element.
"""
import struct

import numpy as np

from oracle import wire_encode as W

import wire_strings_ref as R

OK, E_ARG, E_UNSUPPORTED, E_CORRUPT = R.OK, R.E_ARG, R.E_UNSUPPORTED, R.E_CORRUPT
MAX_BODY, LONG_MIN, EVENT_BODY = R.MAX_BODY, R.LONG_MIN, R.EVENT_BODY
FIELD_TYPES = ("LONG", "INT", "DOUBLE", "FLOAT", "STRING", "DECIMAL")


def boundary_values():
    """Values around every step of the byte length: for k = 1..16, 2^(8k-1) - 1 takes k bytes, 2^(8k-1) takes k + 1,
    -2^(8k-1) takes k and -2^(8k-1) - 1 takes k + 1 (those that fit in 128 bits); and 0, +-1, +-(10^38 - 1), 2^127 - 1,
    -2^127."""
    vals = [0, 1, -1, 10 ** 38 - 1, -(10 ** 38 - 1), (1 << 127) - 1, -(1 << 127)]
    for k in range(1, 17):
        for v in ((1 << (8 * k - 1)) - 1, 1 << (8 * k - 1), -(1 << (8 * k - 1)), -(1 << (8 * k - 1)) - 1):
            if -(1 << 127) <= v < 1 << 127:
                vals.append(v)
    return vals


def unscaled_len(v):
    """Length of BigInteger.toByteArray: bitLength / 8 + 1 (bitLength excludes the sign bit)."""
    v = int(v)
    return (v.bit_length() if v >= 0 else (~v).bit_length()) // 8 + 1


def unscaled_bytes(v, length=None):
    """DecimalData.toUnscaledBytes of the unscaled value v; length: a longer, sign-extended (non-minimal) form."""
    n = unscaled_len(v)
    if length is not None:
        n = max(n, int(length))
    assert n <= 16, "outside DECIMAL(38): %d bytes" % n
    return int(v).to_bytes(n, "big", signed=True)


def row_bytes(fields, row, null_form="setnull", dec_len=None):
    """BinaryRowData bytes of one row. Values per field: int (LONG / INT / DECIMAL), float (DOUBLE / FLOAT),
    str / bytes (STRING) or None. dec_len: forced byte length of the DECIMAL values (None: minimal)."""
    assert null_form in ("setnull", "write")
    arity = len(fields)
    nb = W.nullbits_width(arity)
    fixed = nb + 8 * arity
    head, var = bytearray(fixed), bytearray()
    for f, (t, v) in enumerate(zip(fields, row)):
        assert t in FIELD_TYPES, t
        at = nb + 8 * f
        if v is None:
            head[(f + 8) >> 3] |= 1 << ((f + 8) & 7)
            if t == "DECIMAL" and null_form == "write":
                head[at:at + 8] = struct.pack("<Q", (fixed + len(var)) << 32)
                var += bytes(16)
        elif t == "LONG":
            head[at:at + 8] = struct.pack("<q", int(v))
        elif t == "INT":
            head[at:at + 4] = struct.pack("<i", int(v))
        elif t == "DOUBLE":
            head[at:at + 8] = struct.pack("<d", v)
        elif t == "FLOAT":
            head[at:at + 4] = struct.pack("<f", v)
        elif t == "STRING":
            b = v.encode() if isinstance(v, str) else bytes(v)
            if len(b) <= 7:
                head[at:at + 8] = b + bytes(7 - len(b)) + bytes([0x80 | len(b)])
            else:
                head[at:at + 8] = struct.pack("<Q", ((fixed + len(var)) << 32) | len(b))
                var += b + bytes(-len(b) % 8)
        else:
            b = unscaled_bytes(v, dec_len)
            head[at:at + 8] = struct.pack("<Q", ((fixed + len(var)) << 32) | len(b))
            var += b + bytes(16 - len(b))
    return bytes(head + var)


def encode_stream(fields, rows, ts=None, events=(), null_form="setnull", dec_len=None):
    """rows: tuples; ts: StreamRecord timestamps or None; events: (pos, tag, vals) sorted by pos, written before record
    `pos`; null_form / dec_len: one value for the stream, or a function of the record index giving the record's.
    Returns the bytes and the byte offset of every record element."""
    out, starts, at, evs = [], [], 0, list(events)
    ei = 0
    for i, r in enumerate(rows):
        while ei < len(evs) and evs[ei][0] <= i:
            e = W.encode_event(evs[ei][1], evs[ei][2])
            out.append(e)
            at += len(e)
            ei += 1
        nf = null_form(i) if callable(null_form) else null_form
        dl = dec_len(i) if callable(dec_len) else dec_len
        e = R.frame(row_bytes(fields, r, nf, dl), None if ts is None else int(ts[i]))
        starts.append(at)
        out.append(e)
        at += len(e)
    for _, tag, vals in evs[ei:]:
        out.append(W.encode_event(tag, vals))
    return b"".join(out), starts


def decode(fields, data, key_field=-1, ts_field=-1, cols=()):
    """Sequential decode. Returns (0, result dict) or (error code, {"err_pos": byte offset of the element}). A DECIMAL
    value column is a list of Python ints (0 under a NULL); the other columns are as in wire_strings_ref.decode."""
    data = bytes(data)
    n = len(data)
    arity = len(fields)
    nb = W.nullbits_width(arity)
    fixed = nb + 8 * arity
    sf = [f for f in range(arity) if fields[f] == "STRING"]
    df = [f for f in cols if fields[f] == "DECIMAL"]
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
        dec = {}
        for f in df:
            if isnull(row, f):                                    # the slot of a NULL field is not interpreted
                dec[f] = 0
                continue
            s = slot(row, f)
            off, ln = s >> 32, s & 0xFFFFFFFF
            if off < fixed or off + ln > size or not 1 <= ln <= 16:
                return E_CORRUPT, {"err_pos": p}
            dec[f] = int.from_bytes(data[row + off: row + off + ln], "big", signed=True)   # new BigInteger(bytes)
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
            if fields[f] == "DECIMAL":
                colv[j].append(dec[f])
                continue
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

    def column(c, f):
        if fields[f] == "DECIMAL":
            return list(c)
        a = np.array(c, np.uint64)
        return a.astype(np.uint32) if fields[f] == "FLOAT" else a
    res = {"n_records": len(tss), "n_events": len(evt_pos), "consumed": p,
           "ts": np.array(tss, np.int64),
           "key": np.array(key, np.int64) if key_field >= 0 else None,
           "key_null": np.array(key_null, np.uint8) if key_field >= 0 else None,
           "cols": [column(c, f) for c, f in zip(colv, cols)],
           "col_null": [np.array(c, np.uint8) for c in coln],
           "strings": {f: (np.array(o, np.int32), np.frombuffer(bytes(b), np.uint8), np.array(z, np.uint8))
                       for f, (o, b, z) in strs.items()},
           "evt_pos": np.array(evt_pos, np.int64), "evt_tag": np.array(evt_tag, np.int32),
           "evt_val": np.array(evt_val, np.int64).reshape(-1, 4)}
    return OK, res


def decode_rows(fields, data):
    """The records of a whole stream as tuples (int / None per LONG, INT and DECIMAL field, the 64 / 32 raw bits of a
    DOUBLE / FLOAT, bytes per STRING) and its events as (records before it, tag, vals). Asserts a clean decode."""
    nst = [f for f, t in enumerate(fields) if t != "STRING"]
    rc, got = decode(fields, data, cols=nst)
    assert rc == OK and got["consumed"] == len(data), (rc, got)
    rows = []
    for i in range(got["n_records"]):
        r = [None] * len(fields)
        for j, f in enumerate(nst):
            if got["col_null"][j][i]:
                continue
            v = int(got["cols"][j][i])
            if fields[f] in ("LONG", "INT") and v >> 63:
                v -= 1 << 64
            r[f] = v
        for f, (o, b, z) in got["strings"].items():
            r[f] = None if z[i] else bytes(b[o[i]:o[i + 1]])
        rows.append(tuple(r))
    events = list(zip(got["evt_pos"].tolist(), got["evt_tag"].tolist(), got["evt_val"].tolist()))
    return rows, events
