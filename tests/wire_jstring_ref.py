"""TEST INFRASTRUCTURE ONLY: sender and sequential receiver of wire streams whose TUPLE values carry java.lang.String
fields (include/flink_amd_wire.h FWA_FIELD_JSTRING), and String.hashCode(). Plain Python, independent of flink_amd/.

StringSerializer.serialize -> StringValue.writeString: `len + 1` as a varint (7-bit groups, low group first, bit 7 set on
every group but the last; len = UTF-16 code units), then every code unit coded the same way (1..3 bytes); null is 00.
TupleSerializer writes the fields back to back (fixed fields big-endian, java.io.DataOutput), StreamElementSerializer and
RecordWriter put   be32 L | tag | [be64 ts]   in front:  L = 1 (+ 8) + the value's bytes.

The decoder is a plain loop over the bytes with the accept rules of the header, in this order per element at p:
    fewer than 5 bytes left                               -> END (the element continues in the next buffer)
    tag > 5                                               -> CORRUPT
    tag 2..5: L != the tag's body length                  -> CORRUPT; element past the end -> END
    tag 0 / 1: L < tag + [timestamp] + fixed fields + one byte per JSTRING field  -> CORRUPT
               L > 249                                    -> UNSUPPORTED (the ceiling; never CORRUPT)
               element past the end                       -> END
    per record, the fields in order from a cursor behind the header; nothing at or past the element's end is read:
      fixed field: its 4 / 8 bytes must lie inside the element, else CORRUPT
      JSTRING: the length varint (at most 5 groups, else CORRUPT); a first byte of 00 is null; a varint of several groups
        whose value is 0 is CORRUPT (the reference reader would ask for char[-1]); then len chars, each at most 3 groups,
        its last group not zero behind a continuation group, its third group <= 3 (a value <= 0xFFFF), else CORRUPT;
        the element ending before the last char does -> CORRUPT
      after the last field the cursor must stand at the element's end, else CORRUPT.
    Every error carries the byte position of its element. A value is handed on as its char bytes as they stand.
"""
import struct

import numpy as np

OK, E_ARG, E_UNSUPPORTED, E_CORRUPT = 0, -1, -7, -9
MAX_BODY = 249
LONG_MIN = -(1 << 63)
EVENT_BODY = {2: 9, 3: 29, 4: 5, 5: 2}          # (the same table as wire_strings_ref.EVENT_BODY; a test pins that)
FIXED = {"LONG": (8, ">q"), "DOUBLE": (8, ">d"), "FLOAT": (4, ">f"), "INT": (4, ">i")}


def units(s):
    """UTF-16 code units of a Python str (lone surrogates are units like any other)."""
    raw = s.encode("utf-16-be", "surrogatepass")
    return [(raw[i] << 8) | raw[i + 1] for i in range(0, len(raw), 2)]


def varint(n):
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def char_bytes(s):
    """The canonical form of a value: the coding of its code units, without the length."""
    return b"".join(varint(u) for u in units(s))


def jstring(s):
    """The field bytes of a String (None: null)."""
    if s is None:
        return b"\x00"
    return varint(len(units(s)) + 1) + char_bytes(s)


def text_of(b):
    """Python str of canonical char bytes."""
    us, c, sh = [], 0, 0
    for x in bytes(b):
        c |= (x & 0x7F) << sh
        sh += 7
        if x < 0x80:
            us.append(c)
            c = sh = 0
    assert sh == 0
    return b"".join(struct.pack(">H", u) for u in us).decode("utf-16-be", "surrogatepass")


def java_hash(s):
    """String.hashCode(): s[0]*31^(n-1) + ... + s[n-1] over UTF-16 code units, as a Java int."""
    h = 0
    for u in units(s):
        h = (31 * h + u) & 0xFFFFFFFF
    return h - (1 << 32) if h >> 31 else h


def value_bytes(fields, row):
    """TupleSerializer bytes of one value; a JSTRING entry may also be raw field `bytes` (hand-made, for corrupt cases)."""
    out = bytearray()
    for f, v in zip(fields, row):
        if f == "JSTRING":
            out += v if isinstance(v, (bytes, bytearray)) else jstring(v)
        else:
            out += struct.pack(FIXED[f][1], v)
    return bytes(out)


def frame(value, ts=None):
    body = (b"\x00" + struct.pack(">q", ts) if ts is not None else b"\x01") + value
    return struct.pack(">I", len(body)) + body


def encode_event(tag, vals):
    vals = list(vals) + [0] * 4
    if tag == 2:
        body = struct.pack(">q", vals[0])
    elif tag == 4:
        body = struct.pack(">i", vals[0])
    elif tag == 3:
        body = struct.pack(">qqqi", *vals[:4])
    else:
        body = b"\x01" if vals[0] else b"\x00"
    body = bytes([tag]) + body
    assert len(body) == EVENT_BODY[tag]
    return struct.pack(">I", len(body)) + body


def encode_stream(fields, rows, ts=None, events=()):
    """rows: tuples; ts: StreamRecord timestamps or None; events: (pos, tag, vals) sorted by pos, written before
    record `pos` (pos >= len(rows): behind the last). Returns the bytes and the byte offset of every record element."""
    out, starts, at, evs = [], [], 0, list(events)
    ei = 0
    for i, r in enumerate(rows):
        while ei < len(evs) and evs[ei][0] <= i:
            e = encode_event(evs[ei][1], evs[ei][2])
            out.append(e)
            at += len(e)
            ei += 1
        e = frame(value_bytes(fields, r), None if ts is None else int(ts[i]))
        starts.append(at)
        out.append(e)
        at += len(e)
    for _, tag, vals in evs[ei:]:
        out.append(encode_event(tag, vals))
    return b"".join(out), starts


def _read_jstring(data, q, end):
    """(ok, next cursor, value start, null) of the JSTRING at q in an element ending at end."""
    lv, sh, first = 0, 0, None
    while True:
        if q >= end or sh > 28:
            return False, q, q, 0
        c = data[q]
        q += 1
        if first is None:
            first = c
        lv |= (c & 0x7F) << sh
        sh += 7
        if c < 0x80:
            break
    null = first == 0
    if not null and lv == 0:
        return False, q, q, 0
    n = 0 if null else lv - 1
    if n > end - q:
        return False, q, q, 0
    v0 = q
    for _ in range(n):
        groups = 0
        while True:
            if q >= end:
                return False, q, v0, 0
            c = data[q]
            q += 1
            groups += 1
            if c < 0x80:
                break
            if groups == 3:
                return False, q, v0, 0                             # a fourth group follows
        if groups > 1 and c == 0:
            return False, q, v0, 0
        if groups == 3 and c > 3:
            return False, q, v0, 0
    return True, q, v0, int(null)


def decode(fields, data, ts_field=-1, cols=()):
    """Sequential decode. Returns (0, result dict) or (error code, {"err_pos": byte offset of the element})."""
    data = bytes(data)
    n = len(data)
    sf = [f for f in range(len(fields)) if fields[f] == "JSTRING"]
    short = sum(1 if f == "JSTRING" else FIXED[f][0] for f in fields)
    tss = []
    colv = [[] for _ in cols]
    strs = {f: ([0], bytearray(), []) for f in sf}
    evt_pos, evt_tag, evt_val = [], [], []
    p = 0
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
        hdr = 9 if t == 0 else 1
        if L < hdr + short:
            return E_CORRUPT, {"err_pos": p}
        if L > MAX_BODY:
            return E_UNSUPPORTED, {"err_pos": p}
        if p + 4 + L > n:
            break
        end = p + 4 + L
        q = p + 4 + hdr
        tv = struct.unpack(">q", data[p + 5:p + 13])[0] if t == 0 else LONG_MIN
        got, raw = {}, {}
        for f, ft in enumerate(fields):
            if ft == "JSTRING":
                ok, q, v0, null = _read_jstring(data, q, end)
                if not ok:
                    return E_CORRUPT, {"err_pos": p}
                got[f] = (data[v0:q], null)
                continue
            nb = FIXED[ft][0]
            if q + nb > end:
                return E_CORRUPT, {"err_pos": p}
            u = int.from_bytes(data[q:q + nb], "big")
            if ft == "INT":
                u = (u - (1 << 32) if u >> 31 else u) & 0xFFFFFFFFFFFFFFFF     # sign-extended to the 64-bit column
            raw[f] = u
            q += nb
        if q != end:
            return E_CORRUPT, {"err_pos": p}
        if ts_field >= 0:
            u = raw[ts_field]
            tv = u - (1 << 64) if u >> 63 else u
        tss.append(tv)
        for j, f in enumerate(cols):
            colv[j].append(raw[f])
        for f in sf:
            b, z = got[f]
            strs[f][1].extend(b)
            strs[f][0].append(len(strs[f][1]))
            strs[f][2].append(z)
        p += 4 + L
    res = {"n_records": len(tss), "n_events": len(evt_pos), "consumed": p,
           "ts": np.array(tss, np.int64),
           "cols": [np.array(c, np.uint64).astype(np.uint32) if fields[f] == "FLOAT" else np.array(c, np.uint64)
                    for c, f in zip(colv, cols)],
           "strings": {f: (np.array(o, np.int32), np.frombuffer(bytes(b), np.uint8), np.array(z, np.uint8))
                       for f, (o, b, z) in strs.items()},
           "evt_pos": np.array(evt_pos, np.int64), "evt_tag": np.array(evt_tag, np.int32),
           "evt_val": np.array(evt_val, np.int64).reshape(-1, 4)}
    return OK, res
