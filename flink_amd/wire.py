"""On-GPU decoding of Flink's network wire format (include/flink_amd_wire.h).

`WireDecoder` binds fwa_wire_decode: the concatenated data-buffer payloads of one input channel go in, SoA
columns in HBM (zero-copy torch views, valid until the next decode) and the ordered non-record elements come
out. `NetworkInput` is the host-side mirror of the channel loop in front of the operator:
  AbstractStreamTaskNetworkInput.emitNext / processElement   flink-streaming-java/.../runtime/io/
                                                             AbstractStreamTaskNetworkInput.java:100-181
  StatusWatermarkValve (one channel)                         .../watermarkstatus/StatusWatermarkValve.java:93-115
It pushes each run of records between two events straight from HBM into the window engine and applies the
events in stream order: a watermark that advances the channel's watermark fires windows
(processWatermark), WatermarkStatus IDLE / ACTIVE toggles the channel, latency markers and record attributes
are forwarded. No CPU fallback: the HIP library must be present.

STRING fields (CHAR / VARCHAR / STRING of ROWDATA rows) come back through `DecodedBatch.strings(f)` as Arrow-style
(offsets, bytes, null) device views; `NetworkInput(schema, engine, keydict=kd, key_parts=[...])` turns them and the
value columns into key dictionary ids per run of records, so a VARCHAR-keyed Table job runs from the channel's bytes.

DECIMAL fields (precision > 18, non-compact, ROWDATA rows) decode to int64 [n, 2] (low, high) columns -- the layout
`_abi.dec128_column` makes and SUM_DEC128 / AVG_DEC128 read -- and the DECIMAL aggregates' results are written as
"DECIMAL" fields by the encoder. A DECIMAL with precision <= 18 is its unscaled long: "LONG" in both directions.

JSTRING fields (java.lang.String fields of TUPLE values, StringSerializer's varint-prefixed UTF-16 code units) come back
through `DecodedBatch.strings(f)` too, as their canonical char bytes (the bytes behind the length prefix, as they stand
on the wire; `jstring_text` / `jstring_bytes` convert for display). `NetworkInput(schema, engine, keydict=d, key_string=f)`
runs a String-keyed DataStream job from the channel's bytes: ids from `d.encode`, `String.hashCode()` from `jstring_hash`,
both on the device, pushed into a KEY_PREHASHED handle. A dictionary holding such values must not also be fed UTF-8
"STRING" values: the same non-ASCII text has different bytes in the two forms.

The other direction: `WireEncoder` binds fwa_wire_encode -- the SoA columns of a watermark step (fwa_out, and the decoded
key dictionary columns of a Table job) become the bytes RecordWriter would have produced, in HBM -- and `NetworkOutput`
is the mirror of RecordWriterOutput (flink-streaming-java/.../runtime/io/RecordWriterOutput.java:131-135 and its
emitWatermark / emitWatermarkStatus / emitLatencyMarker / emitRecordAttributes): emit(wm) fires the engine and returns
"rows, then the watermark" as channel bytes.
"""
import ctypes as C

import numpy as np

from . import _abi as A
from .engine import EngineError, _host_to_np, _is_torch_cuda, dev_view, lib
from .keydict import FIELD as KEY_FIELD, KeyStrings

MAX_FIELDS = 16
FORMATS = {"TUPLE": 0, "ROWDATA": 1}
FIELDS = {"LONG": 0, "DOUBLE": 1, "FLOAT": 2, "INT": 3, "STRING": 4, "DECIMAL": 6, "JSTRING": 8}   # (5, 7 are unassigned)
FIELD_DTYPE = {0: "i8", 1: "f8", 2: "f4", 3: "i8", 6: "i8"}  # value-column dtype per field type (DECIMAL: two per record)
TAG_REC_WITH_TIMESTAMP, TAG_REC_WITHOUT_TIMESTAMP, TAG_WATERMARK, TAG_LATENCY_MARKER, TAG_STREAM_STATUS, \
    TAG_RECORD_ATTRIBUTES = range(6)
WIRE_DEVICE_BYTES = 0x1
WATERMARK_STATUS_IDLE, WATERMARK_STATUS_ACTIVE = -1, 0     # WatermarkStatus.IDLE_STATUS / ACTIVE_STATUS


class Schema(C.Structure):
    _fields_ = [("format", C.c_int32), ("arity", C.c_int32), ("field", C.c_int32 * MAX_FIELDS),
                ("key_field", C.c_int32), ("ts_field", C.c_int32), ("num_cols", C.c_int32),
                ("col_field", C.c_int32 * 8), ("device", C.c_int32), ("max_bytes", C.c_int64)]


class Batch(C.Structure):
    _fields_ = [("n_records", C.c_int64), ("n_events", C.c_int64), ("consumed", C.c_int64),
                ("key", C.c_void_p), ("ts", C.c_void_p), ("col", C.c_void_p * 8), ("col_null", C.c_void_p * 8),
                ("key_null", C.c_void_p), ("evt_pos", C.c_void_p), ("evt_tag", C.c_void_p), ("evt_val", C.c_void_p)]


class Strings(C.Structure):                 # fwa_wire_strings
    _fields_ = [("offsets", C.c_void_p), ("bytes", C.c_void_p), ("null", C.c_void_p), ("total_bytes", C.c_int64)]


class WireStats(C.Structure):
    _fields_ = [("calls", C.c_int64), ("bytes_in", C.c_int64), ("records_out", C.c_int64),
                ("decode_ms", C.c_double), ("scan_ms", C.c_double)]


def make_schema(fields, key_field, ts_field=-1, cols=(), fmt="TUPLE", device=0, max_bytes=0):
    """fields: field type names in value order ("LONG", "DOUBLE", "FLOAT", "INT", "STRING" / "DECIMAL" in ROWDATA rows and
    "JSTRING", a java.lang.String, in TUPLE values); key_field -1 (schemas with a STRING field; always with a JSTRING
    field) = the caller builds the key; ts_field -1 = the StreamRecord
    timestamp; cols: the fields that become value columns 0, 1, ..."""
    s = Schema()
    s.format = FORMATS[fmt]
    s.arity = len(fields)
    for i, f in enumerate(fields):
        s.field[i] = FIELDS[f]
    s.key_field, s.ts_field = key_field, ts_field
    s.num_cols = len(cols)
    for j, f in enumerate(cols):
        s.col_field[j] = f
    s.device, s.max_bytes = device, max_bytes
    return s


def jstring_bytes(text):
    """The canonical char bytes of a String (StringValue.writeString's coding of each UTF-16 code unit, 1..3 bytes,
    without the length prefix): what DecodedBatch.strings returns for a JSTRING field and what a key dictionary of
    String keys holds. Lone surrogates are code units like any other."""
    raw = text.encode("utf-16-le", "surrogatepass")
    out = bytearray()
    for i in range(0, len(raw), 2):
        c = raw[i] | (raw[i + 1] << 8)
        while c >= 0x80:
            out.append((c & 0x7F) | 0x80)
            c >>= 7
        out.append(c)
    return bytes(out)


def jstring_text(data):
    """The String of canonical char bytes (the inverse of jstring_bytes)."""
    units = bytearray()
    c = sh = 0
    for b in bytes(data):
        c |= (b & 0x7F) << sh
        sh += 7
        if b < 0x80:
            if c > 0xFFFF or sh > 21 or (sh > 7 and b == 0):
                raise ValueError("not the canonical coding of a UTF-16 code unit")
            units += bytes((c & 0xFF, c >> 8))
            c = sh = 0
    if sh:
        raise ValueError("the bytes end inside a char")
    return bytes(units).decode("utf-16-le", "surrogatepass")


def jstring_field(text):
    """The field bytes StringSerializer writes: the varint of len + 1 (UTF-16 code units), then the chars; None is 00."""
    if text is None:
        return b"\x00"
    body = jstring_bytes(text)
    n = sum(1 for b in body if b < 0x80) + 1
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out) + body


def jstring_hash(offsets, data, nulls=None):
    """String.hashCode() of values in the canonical char-byte form, on the device: offsets int32 [n + 1] (they need not
    start at 0), data uint8, nulls uint8 [n] or None (a NULL value hashes to 0), all torch CUDA tensors. Returns a torch
    int32 CUDA tensor [n]: the key_hash column of WindowAggregator.push on a KEY_PREHASHED handle."""
    import torch
    for t in (offsets, data) + (() if nulls is None else (nulls,)):
        if not _is_torch_cuda(t):
            raise EngineError(-1, "jstring_hash takes CUDA tensors")
    if offsets.dtype != torch.int32 or data.dtype != torch.uint8:
        raise EngineError(-1, "jstring_hash: offsets are int32 and data uint8")
    offsets, data = offsets.contiguous(), data.contiguous()
    n = offsets.numel() - 1
    if n < 0:
        raise EngineError(-1, "jstring_hash: offsets has n + 1 entries")
    if nulls is not None:
        nulls = nulls.contiguous()
        if nulls.dtype == torch.bool:
            nulls = nulls.view(torch.uint8)
        if nulls.dtype != torch.uint8 or nulls.numel() != n:
            raise EngineError(-1, "jstring_hash: nulls is uint8 [n]")
    L = _bind(lib())
    out = torch.empty(n, dtype=torch.int32, device=offsets.device)
    torch.cuda.synchronize()
    rc = L.fwa_jstring_hash(offsets.data_ptr(), data.data_ptr(), None if nulls is None else nulls.data_ptr(), n,
                            out.data_ptr(), offsets.device.index or 0)
    if rc:
        raise EngineError(rc, "fwa_jstring_hash")
    return out


def _bind(L):
    if getattr(L, "_wire_bound", False):
        return L
    L.fwa_wire_create.argtypes = [C.POINTER(Schema), C.POINTER(C.c_void_p)]
    L.fwa_wire_create.restype = C.c_int
    L.fwa_wire_destroy.argtypes = [C.c_void_p]
    L.fwa_wire_destroy.restype = None
    L.fwa_wire_last_error.argtypes = [C.c_void_p]
    L.fwa_wire_last_error.restype = C.c_char_p
    L.fwa_wire_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(Batch)]
    L.fwa_wire_decode.restype = C.c_int
    L.fwa_wire_get_stats.argtypes = [C.c_void_p, C.POINTER(WireStats)]
    L.fwa_wire_get_stats.restype = C.c_int
    L.fwa_wire_strings_of.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Strings)]
    L.fwa_wire_strings_of.restype = C.c_int
    L.fwa_jstring_hash.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32]
    L.fwa_jstring_hash.restype = C.c_int
    L._wire_bound = True
    return L


class DecodedBatch:
    """Columns of one decode (torch CUDA views into decoder-owned HBM, valid until its next decode)."""

    def __init__(self, schema, b, decoder=None):
        self.n_records, self.n_events, self.consumed = b.n_records, b.n_events, b.consumed
        self._decoder = decoder
        n = self.n_records
        self.key = dev_view(b.key, n, np.dtype("i8")) if b.key else None
        self.ts = dev_view(b.ts, n, np.dtype("i8"))
        self.cols = []
        for j in range(schema.num_cols):
            t = schema.field[schema.col_field[j]]
            if t == FIELDS["DECIMAL"]:                             # 16-byte values as int64 [n, 2] (low, high)
                self.cols.append(dev_view(b.col[j], 2 * n, np.dtype("i8")).view(n, 2))
            else:
                self.cols.append(dev_view(b.col[j], n, np.dtype(FIELD_DTYPE[t])))
        rowdata = schema.format == FORMATS["ROWDATA"]
        self.col_null = [dev_view(b.col_null[j], n, np.dtype("u1")) for j in range(schema.num_cols)] if rowdata else None
        self.key_null = dev_view(b.key_null, n, np.dtype("u1")) if rowdata and b.key_null else None
        ne = self.n_events
        if ne:
            self.evt_pos = np.ctypeslib.as_array(C.cast(b.evt_pos, C.POINTER(C.c_int64)), (ne,)).copy()
            self.evt_tag = np.ctypeslib.as_array(C.cast(b.evt_tag, C.POINTER(C.c_int32)), (ne,)).copy()
            self.evt_val = np.ctypeslib.as_array(C.cast(b.evt_val, C.POINTER(C.c_int64)), (ne, 4)).copy()
        else:
            self.evt_pos = np.zeros(0, np.int64)
            self.evt_tag = np.zeros(0, np.int32)
            self.evt_val = np.zeros((0, 4), np.int64)

    def strings(self, f):
        """(offsets int32 [n + 1], bytes uint8, null uint8 [n]) of STRING or JSTRING field f (a JSTRING's canonical char bytes): views valid until the decoder's
        next decode. (offsets[a:b + 1], bytes) is what KeyDictionary.encode takes for records [a, b). Device input
        of the decode must still be alive and unchanged at the first call per field (the extraction is lazy)."""
        return self._decoder.strings_of(f, self.n_records)


class WireDecoder:
    """One decoder per input channel (single-threaded, like the channel's record deserializer)."""

    def __init__(self, schema):
        self.schema = schema
        self.L = _bind(lib())
        self.h = C.c_void_p()
        self._input = None                        # device input of the last decode (read again by strings_of)
        rc = self.L.fwa_wire_create(C.byref(schema), C.byref(self.h))
        if rc:
            raise EngineError(rc, "fwa_wire_create")

    def decode(self, data):
        """data: bytes / numpy uint8 (host, staged by the decoder) or a torch CUDA uint8 tensor (HBM)."""
        b = Batch()
        if _is_torch_cuda(data):
            import torch
            torch.cuda.current_stream(data.device).synchronize()   # the bytes' producer ran on torch's stream
            ptr, n, flags = C.c_void_p(data.data_ptr()), data.numel(), WIRE_DEVICE_BYTES
            keep = self._input = data
        else:
            arr = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, np.uint8)
            ptr, n, flags = arr.ctypes.data_as(C.c_void_p), arr.size, 0
            keep, self._input = arr, None
        rc =self.L.fwa_wire_decode(self.h, ptr, n, flags, C.byref(b))
        del keep
        if rc:
            raise EngineError(rc, self.L.fwa_wire_last_error(self.h).decode())
        return DecodedBatch(self.schema, b, self)

    def strings_of(self, f, n):
        s = Strings()
        rc = self.L.fwa_wire_strings_of(self.h, f, C.byref(s))
        if rc:
            raise EngineError(rc, self.L.fwa_wire_last_error(self.h).decode())
        return (dev_view(s.offsets, n + 1, np.dtype("i4")), dev_view(s.bytes, max(1, s.total_bytes), np.dtype("u1")),
                dev_view(s.null, n, np.dtype("u1")))

    def stats(self):
        s = WireStats()
        self.L.fwa_wire_get_stats(self.h, C.byref(s))
        return s

    def close(self):
        if self.h:
            self.L.fwa_wire_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NetworkInput:
    """One input channel in front of a window engine handle (flink_amd.engine.WindowAggregator).

    feed(buffer) takes the next data-buffer payload of the channel; an element that continues in the next
    buffer is carried over (SpanningWrapper). Returns the window rows fired by the watermarks in it.
    """

    def __init__(self, schema, engine, keydict=None, key_parts=None, key_string=None):
        """keydict (flink_amd.keydict.KeyDictionary) with key_parts, the key row's fields in the dictionary's order,
        each ("str", field) -- a STRING field of the schema -- or ("col", j) -- value column j: every run of records
        is pushed under the ids keydict.encode gives its key rows (NULL flags included; a NULL grouping key is a
        key like any other there). Without keydict the schema's key_field is the key, as before.
        keydict with key_string=f, a JSTRING field of a TUPLE schema: a DataStream job keyed by that String. keydict is a
        one-field STRING dictionary (it holds the keys' canonical char bytes) and engine a KEY_PREHASHED handle; every
        run of records is pushed under keydict.encode's ids with key_hash = jstring_hash(...), String.hashCode() computed
        on the device, so the handle's key-group check reads the hash Flink's would. A null key raises
        EngineError(-1, "Assigned key must not be null") like KeyGroupRangeAssignment.assignToKeyGroup."""
        if key_string is not None:
            if key_parts is not None:
                raise EngineError(-1, "key_string and key_parts exclude each other: a String key is one JSTRING field")
            if keydict is None:
                raise EngineError(-1, "key_string needs keydict, a one-field STRING KeyDictionary")
            if list(keydict.types) != [KEY_FIELD["STRING"]]:
                raise EngineError(-1, "key_string: the key dictionary has exactly one field, a STRING")
            key_string = int(key_string)
            if not (schema.format == FORMATS["TUPLE"] and 0 <= key_string < schema.arity
                    and schema.field[key_string] == FIELDS["JSTRING"]):
                raise EngineError(-1, "key_string names a JSTRING field of a TUPLE schema")
            if engine.cfg.key_kind != A.KEY_PREHASHED:
                raise EngineError(-1, "key_string needs a KEY_PREHASHED handle: the ids go beside String.hashCode()")
        elif (keydict is None) != (key_parts is None):
            raise EngineError(-1, "keydict and key_parts go together")
        self.key_string = key_string
        self.decoder = WireDecoder(schema)
        self.engine = engine
        self.keydict = keydict
        self.key_parts = None if key_parts is None else [(k, int(i)) for k, i in key_parts]
        if self.key_parts is not None and any(k not in ("str", "col") for k, _ in self.key_parts):
            raise EngineError(-1, "key_parts entries are ('str', field) or ('col', j)")
        self.carry = b""
        self.watermark = A.LONG_MIN                 # the channel's last forwarded watermark (valve)
        self.idle = False
        self.latency_markers = []                   # (markedTime, operatorId lower, upper, subtaskIndex)
        self.record_attributes = []                 # isBacklog flags, in order
        self.records_in = 0
        self.late_dropped = 0

    def _push(self, batch, a, b):
        if b <= a:
            return
        if getattr(self, "key_string", None) is not None:
            return self._push_string(batch, a, b)
        if getattr(self, "keydict", None) is not None:
            return self._push_dict(batch, a, b)
        if batch.key_null is not None and bool(batch.key_null[a:b].any()):
            raise EngineError(-7, "NULL grouping key: pass the key hash with FWA_KEY_PREHASHED instead")
        nulls = None
        if batch.col_null is not None:
            nulls = [c[a:b] for c in batch.col_null]
        self.late_dropped += self.engine.push(batch.key[a:b], batch.ts[a:b], [c[a:b] for c in batch.cols],
                                              nulls=nulls if nulls and self.engine.cfg.nullable_cols else None)
        self.records_in += b - a

    def _push_dict(self, batch, a, b):
        cols, nulls = [], []
        for kind, i in self.key_parts:
            if kind == "str":
                offs, data, nul = batch.strings(i)
                cols.append((offs[a:b + 1], data))               # offsets need not start at 0 (fwa_key_strings)
                nulls.append(nul[a:b])
            else:
                cols.append(batch.cols[i][a:b])
                nulls.append(batch.col_null[i][a:b] if batch.col_null is not None else None)
        ids = self.keydict.encode(cols, nulls)
        vn = None
        if batch.col_null is not None and self.engine.cfg.nullable_cols:
            vn = [c[a:b] for c in batch.col_null]
        self.late_dropped += self.engine.push(ids, batch.ts[a:b], [c[a:b] for c in batch.cols], nulls=vn)
        self.records_in += b - a

    def _push_string(self, batch, a, b):
        offs, data, nul = batch.strings(self.key_string)
        if bool(nul[a:b].any()):
            raise EngineError(-1, "Assigned key must not be null")   # KeyGroupRangeAssignment.assignToKeyGroup
        run = offs[a:b + 1]                                      # offsets need not start at 0
        ids = self.keydict.encode([(run, data)])
        self.late_dropped += self.engine.push(ids, batch.ts[a:b], [c[a:b] for c in batch.cols],
                                              key_hash=jstring_hash(run, data))
        self.records_in += b - a

    def feed(self, buffer):
        import torch
        if self.carry:
            if _is_torch_cuda(buffer):
                buffer = torch.cat([torch.frombuffer(bytearray(self.carry), dtype=torch.uint8).to(buffer.device), buffer])
            else:
                buffer = self.carry + bytes(buffer)
        batch = self.decoder.decode(buffer)
        rows = []
        at = 0
        for pos, tag, val in zip(batch.evt_pos.tolist(), batch.evt_tag.tolist(), batch.evt_val.tolist()):
            self._push(batch, at, pos)
            at = pos
            if tag == TAG_WATERMARK:
                # StatusWatermarkValve.inputWatermark: an idle channel's or a non-advancing watermark is ignored
                if not self.idle and val[0] > self.watermark:
                    self.watermark = val[0]
                    rows.append(self.engine.advance_watermark(val[0]))
            elif tag == TAG_STREAM_STATUS:
                self.idle = val[0] == WATERMARK_STATUS_IDLE
            elif tag == TAG_LATENCY_MARKER:
                self.latency_markers.append(tuple(val))
            else:
                self.record_attributes.append(bool(val[0]))
        self._push(batch, at, batch.n_records)
        tail = len(buffer) - batch.consumed if not _is_torch_cuda(buffer) else buffer.numel() - batch.consumed
        if tail:
            rest = buffer[batch.consumed:]
            self.carry = bytes(rest.cpu().numpy()) if _is_torch_cuda(rest) else bytes(rest)
        else:
            self.carry = b""
        return rows

    def close(self):
        self.decoder.close()


# ---- the sender side: fwa_wire_encode ----
SOURCES = {"KEY": 0, "KEYCOL": 1, "WIN_START": 2, "WIN_END": 3, "WIN_TIME": 4, "AGG": 5}
RECORD_TS = {None: 0, "NONE": 0, "WIN_TIME": 1}
WIRE_HOST_BYTES = 0x2
MAX_KEYCOLS = 8


class OutSchema(C.Structure):               # fwa_wire_out_schema
    _fields_ = [("format", C.c_int32), ("arity", C.c_int32), ("field", C.c_int32 * MAX_FIELDS),
                ("src", C.c_int32 * MAX_FIELDS), ("src_index", C.c_int32 * MAX_FIELDS),
                ("src_kind", C.c_int32 * MAX_FIELDS), ("record_ts", C.c_int32), ("device", C.c_int32),
                ("max_bytes", C.c_int64)]


class KeyCols(C.Structure):                 # fwa_wire_keycols
    _fields_ = [("n_cols", C.c_int32), ("pad", C.c_int32), ("col", C.c_void_p * MAX_KEYCOLS),
                ("null", C.c_void_p * MAX_KEYCOLS), ("str", KeyStrings * MAX_KEYCOLS)]


class Event(C.Structure):                   # fwa_wire_event
    _fields_ = [("tag", C.c_int32), ("pad", C.c_int32), ("val", C.c_int64 * 4)]


class WireBytes(C.Structure):               # fwa_wire_bytes
    _fields_ = [("dev", C.c_void_p), ("host", C.c_void_p), ("nbytes", C.c_int64)]


class EncStats(C.Structure):                # fwa_wire_enc_stats
    _fields_ = [("calls", C.c_int64), ("rows_in", C.c_int64), ("bytes_out", C.c_int64), ("encode_ms", C.c_double),
                ("scan_ms", C.c_double), ("size_ms", C.c_double)]


def make_out_schema(fields, fmt="TUPLE", record_ts=None, device=0, max_bytes=0):
    """fields, in the value's order: (wire type, source) pairs. The wire type is "LONG" / "DOUBLE" / "FLOAT" / "INT",
    "STRING" / "DECIMAL" in ROWDATA rows, or "JSTRING" in TUPLE values (a java.lang.String; its one source is
    ("KEYCOL", k, "STRING"), the dictionary-decoded key in the canonical char-byte form); the source is "KEY", "WIN_START", "WIN_END", "WIN_TIME" (win_end - 1),
    ("AGG", j, kind) with the aggregate's kind name as in flink_amd._abi.AGG_KINDS (it fixes the dtype of the result
    column), or ("KEYCOL", k, type) with the key dictionary column's type ("BIGINT" / "INT" / "DOUBLE" / "STRING").
    "DECIMAL" takes exactly the DECIMAL aggregates ("SUM_DEC" / "AVG_DEC" / "SUM_DEC128" / "AVG_DEC128": a DECIMAL(38, s)).
    record_ts: None (TAG_REC_WITHOUT_TIMESTAMP, Table rows) or "WIN_TIME" (the DataStream record timestamp win_end - 1).
    The pairing of sources and wire types is checked by fwa_wire_enc_create (WireEncoder)."""
    fields = list(fields)
    if not 1 <= len(fields) <= MAX_FIELDS:
        raise ValueError("arity %d out of range (1..%d)" % (len(fields), MAX_FIELDS))
    if fmt not in FORMATS:
        raise ValueError("unknown wire format %r" % (fmt,))
    if record_ts not in RECORD_TS:
        raise ValueError("record_ts is None or 'WIN_TIME', not %r" % (record_ts,))
    s = OutSchema()
    s.format, s.arity = FORMATS[fmt], len(fields)
    for i, fs in enumerate(fields):
        if not isinstance(fs, (tuple, list)) or len(fs) != 2:
            raise ValueError("field %d: a (wire type, source) pair is expected, not %r" % (i, fs))
        t, src = fs
        if t not in FIELDS:
            raise ValueError("field %d: unknown wire type %r" % (i, t))
        s.field[i] = FIELDS[t]
        if t == "DECIMAL" and not (isinstance(src, (tuple, list)) and len(src) == 3 and src[0] == "AGG" and src[2] in A.DEC_KINDS):
            raise ValueError("field %d: wire type 'DECIMAL' takes a DECIMAL aggregate, ('AGG', j, kind) with kind in %s, not %r"
                             % (i, "/".join(A.DEC_KINDS), src))
        if isinstance(src, str):
            if src not in SOURCES or src in ("AGG", "KEYCOL"):
                raise ValueError("field %d: source %r (AGG and KEYCOL are (name, index, kind) triples)" % (i, src))
            s.src[i] = SOURCES[src]
            continue
        if len(src) != 3 or src[0] not in ("AGG", "KEYCOL"):
            raise ValueError("field %d: source %r is not ('AGG', j, kind) or ('KEYCOL', k, type)" % (i, src))
        name, j, kind = src
        table, limit = (A.AGG_KINDS, A.FWA_MAX_AGGS) if name == "AGG" else (KEY_FIELD, MAX_KEYCOLS)
        if kind not in table:
            raise ValueError("field %d: unknown %s %r" % (i, "aggregate kind" if name == "AGG" else "key field type", kind))
        if not 0 <= int(j) < limit:
            raise ValueError("field %d: %s index %d out of range (0..%d)" % (i, name, j, limit - 1))
        s.src[i], s.src_index[i], s.src_kind[i] = SOURCES[name], int(j), table[kind]
    s.record_ts, s.device, s.max_bytes = RECORD_TS[record_ts], device, max_bytes
    return s


def _bind_enc(L):
    if getattr(L, "_wire_enc_bound", False):
        return L
    L.fwa_wire_enc_create.argtypes = [C.POINTER(OutSchema), C.POINTER(C.c_void_p)]
    L.fwa_wire_enc_create.restype = C.c_int
    L.fwa_wire_enc_destroy.argtypes = [C.c_void_p]
    L.fwa_wire_enc_destroy.restype = None
    L.fwa_wire_enc_last_error.argtypes = [C.c_void_p]
    L.fwa_wire_enc_last_error.restype = C.c_char_p
    L.fwa_wire_encode.argtypes = [C.c_void_p, C.POINTER(A.Out), C.POINTER(KeyCols), C.POINTER(Event), C.c_int32,
                                  C.c_int32, C.POINTER(WireBytes)]
    L.fwa_wire_encode.restype = C.c_int
    L.fwa_wire_enc_get_stats.argtypes = [C.c_void_p, C.POINTER(EncStats)]
    L.fwa_wire_enc_get_stats.restype = C.c_int
    L._wire_enc_bound = True
    return L


def _key_cols(keycols):
    """(cols, nulls) as KeyDictionary.decode_device returns them -> fwa_wire_keycols and the tensors it points into."""
    cols, nulls = keycols
    if len(cols) > MAX_KEYCOLS:
        raise EngineError(-1, "at most %d key columns" % MAX_KEYCOLS)
    kc = KeyCols()
    kc.n_cols = len(cols)
    for c, col in enumerate(cols):
        parts = col if isinstance(col, tuple) else (col,)
        z = None if nulls is None else nulls[c]
        for t in parts + ((z,) if z is not None else ()):
            if t is not None and not _is_torch_cuda(t):
                raise EngineError(-1, "key columns are CUDA tensors (KeyDictionary.decode_device)")
        if isinstance(col, tuple):
            kc.str[c].offsets, kc.str[c].bytes = col[0].data_ptr(), col[1].data_ptr()
        elif col is not None:
            kc.col[c] = col.data_ptr()
        if z is not None:
            kc.null[c] = z.data_ptr()
    return kc


class WireEncoder:
    """One encoder per output channel (single-threaded, like the RecordWriter's serializer)."""

    def __init__(self, schema):
        self.schema = schema
        self.L = _bind_enc(lib())
        self.h = C.c_void_p()
        rc = self.L.fwa_wire_enc_create(C.byref(schema), C.byref(self.h))
        if rc:
            raise EngineError(rc, self.L.fwa_wire_enc_last_error(None).decode() or "fwa_wire_enc_create")

    def encode(self, out, keycols=None, events=(), host=False):
        """out: the rows (flink_amd._abi.Out, as WindowAggregator.advance_watermark_raw returns them: device or host
        columns); keycols: (cols, nulls) of KeyDictionary.decode_device for the KEYCOL sources; events: (tag, vals) of
        the non-record elements written behind the rows. Returns the channel bytes: a zero-copy torch uint8 CUDA view
        valid until the next encode, or with host=True (FWA_WIRE_HOST_BYTES) a bytes object."""
        evs = list(events)
        earr = (Event * max(1, len(evs)))()
        for i, (tag, vals) in enumerate(evs):
            earr[i].tag = int(tag)
            for j, v in enumerate(list(vals)[:4]):
                earr[i].val[j] = int(v)
        kc = None if keycols is None else _key_cols(keycols)
        if out.on_device or kc is not None:
            import torch
            torch.cuda.synchronize()                               # the columns' producers ran on torch's streams
        b = WireBytes()
        rc = self.L.fwa_wire_encode(self.h, C.byref(out), None if kc is None else C.byref(kc), earr, len(evs),
                                    WIRE_HOST_BYTES if host else 0, C.byref(b))
        if rc:
            raise EngineError(rc, self.L.fwa_wire_enc_last_error(self.h).decode())
        if host:
            return C.string_at(b.host, b.nbytes) if b.nbytes else b""
        return dev_view(b.dev, b.nbytes, np.dtype("u1"))

    def stats(self):
        s = EncStats()
        self.L.fwa_wire_enc_get_stats(self.h, C.byref(s))
        return s

    def close(self):
        if self.h:
            self.L.fwa_wire_enc_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NetworkOutput:
    """One output channel behind a window engine handle: the mirror of RecordWriterOutput.

    emit(wm) is the operator's watermark step seen from the channel: the windows wm completes fire, their rows are
    written as StreamRecords in emission order and the watermark follows them (AbstractStreamOperator.processWatermark
    :610-615). With keydict (the handle runs on key dictionary ids) the fired ids are decoded to their key columns on the
    device and the schema's KEYCOL sources read those. The other elements go out as elements of their own."""

    def __init__(self, schema, engine, keydict=None, host=False):
        uses = any(schema.src[i] == SOURCES["KEYCOL"] for i in range(schema.arity))
        if uses and keydict is None:
            raise EngineError(-1, "the schema has KEYCOL sources: pass the handle's key dictionary")
        self.encoder = WireEncoder(schema)
        self.engine = engine
        self.keydict = keydict
        self.host = host
        self.rows_out = 0

    def _no_rows(self):
        out = A.Out()
        out.on_device, out.num_aggs = 1, A.FWA_MAX_AGGS
        kc = None if self.keydict is None else ([None] * len(self.keydict.types), None)
        return out, kc

    def emit(self, wm, events=()):
        """Advance the engine's watermark to wm; returns the bytes of the fired rows, the watermark, then `events`."""
        out = self.engine.advance_watermark_raw(wm)
        n = out.n_rows
        kc = None
        if self.keydict is not None:
            if n:
                i8 = np.dtype("i8")
                ids = dev_view(out.key, n, i8) if out.on_device else _host_to_np(out.key, n, i8)
                kc = self.keydict.decode_device(ids)
                if self.encoder.schema.format == FORMATS["TUPLE"]:   # TupleSerializer cannot write null fields
                    import torch
                    if bool(torch.stack(kc[1]).any()):
                        raise EngineError(-1, "a NULL key column in a TUPLE value: TupleSerializer cannot write null fields")
                    kc = (kc[0], None)
            else:
                kc = self._no_rows()[1]
        self.rows_out += n
        return self.encoder.encode(out, kc, [(TAG_WATERMARK, (int(wm),))] + list(events), host=self.host)

    def _event(self, tag, vals):
        out, kc = self._no_rows()
        return self.encoder.encode(out, kc, [(tag, vals)], host=self.host)

    def emit_watermark_status(self, status):
        """WatermarkStatus IDLE (-1) / ACTIVE (0)."""
        return self._event(TAG_STREAM_STATUS, (int(status),))

    def emit_latency_marker(self, marked_time, operator_id_lower, operator_id_upper, subtask_index):
        return self._event(TAG_LATENCY_MARKER, (marked_time, operator_id_lower, operator_id_upper, subtask_index))

    def emit_record_attributes(self, is_backlog):
        return self._event(TAG_RECORD_ATTRIBUTES, (1 if is_backlog else 0,))

    def close(self):
        self.encoder.close()
