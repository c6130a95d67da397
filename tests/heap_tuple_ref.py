"""Writer of Flink's heap keyed-state key-group sections (test infrastructure): the inverse of tests/heap_reader.py.

Plain-Python restatement of the reference's writers, used to check the engine's heap-layout bytes of DataStream
reductions and String keys (tests/test_heap_reduce_gpu.py): the engine's body is parsed with heap_reader, the parsed
entries are written again here in the same order, and the two byte strings must be equal -- so the engine's bytes hold
nothing but what the reader understood, in the reference's coding. Pinned by the reference's own reduce checkpoint
(tests/test_heap_reduce_cpu.py reproduces its key-group section byte for byte).

A key-group section (HeapSnapshotStrategy.java:154-175, java.io.DataOutput, big-endian):
  int keyGroupId; per state: short stateId, int n, then n entries
    key/value state: (namespace, key, value)                      CopyOnWriteStateMapSnapshot.writeState :138-148
    timer queue:     (long flipSignBit(ts), key, namespace)       TimerSerializer.serialize :147-152
Serializers (each a function value -> bytes): StringSerializer (StringValue.writeString: varint of len + 1, then every
UTF-16 code unit as a varint of 1..3 bytes; None is 00), LongSerializer, IntSerializer, DoubleSerializer,
FloatSerializer (the IEEE bits, big-endian), TimeWindow.Serializer (long start, long end), TupleSerializer (the fields
in order, no null mask). Double / Float values are handed over and returned as their bit patterns (ints), so that NaN
payloads and -0.0 survive a round trip unchanged; `ser_double` / `ser_float` are the matching readers for heap_reader's
layouts.
"""
import struct


def _varint(n):
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def units_of(text):
    """UTF-16 code units of a str (lone surrogates, as heap_reader.ser_string returns them, stay single units)."""
    raw = text.encode("utf-16-le", "surrogatepass")
    return [raw[i] | (raw[i + 1] << 8) for i in range(0, len(raw), 2)]


def w_string(text):
    if text is None:
        return b"\x00"
    u = units_of(text)
    return _varint(len(u) + 1) + b"".join(_varint(c) for c in u)


def w_long(v):
    return struct.pack(">q", v)


def w_int(v):
    return struct.pack(">i", v)


def w_double(bits):
    return struct.pack(">Q", bits)


def w_float(bits):
    return struct.pack(">I", bits)


def w_time_window(w):
    return struct.pack(">qq", w[0], w[1])


def w_void(_):
    return b"\x00"


def w_tuple(*fields):
    return lambda v: b"".join(f(x) for f, x in zip(fields, v))


def w_list(elem):
    return lambda v: struct.pack(">i", len(v)) + b"".join(elem(x) for x in v)


def ser_double(r):
    """DoubleSerializer -> the value's 64 bits"""
    return r.get(">Q")


def ser_float(r):
    """FloatSerializer -> the value's 32 bits"""
    return r.get(">I")


def java_string_hash(text):
    """String.hashCode(): h = 31 * h + unit over the UTF-16 code units, int wrap"""
    h = 0
    for c in units_of(text):
        h = (31 * h + c) & 0xFFFFFFFF
    return h - (1 << 32) if h >= 1 << 31 else h


def write_key_group(kg, states):
    """One key-group section. states: [(state id, layout, entries)] in the order they are written; a layout is
    ("kv", namespace writer, key writer, value writer) with entries (namespace, key, value), or ("pq", key writer,
    namespace writer) with entries (timestamp, key, namespace) -- the shapes heap_reader.read_key_groups returns."""
    out = bytearray(struct.pack(">i", kg))
    for sid, lay, ents in states:
        out += struct.pack(">hi", sid, len(ents))
        for e in ents:
            if lay[0] == "kv":
                out += lay[1](e[0]) + lay[2](e[1]) + lay[3](e[2])
            else:
                out += struct.pack(">Q", (e[0] ^ (1 << 63)) & 0xFFFFFFFFFFFFFFFF) + lay[1](e[1]) + lay[2](e[2])
    return bytes(out)


def write_key_groups(sections, layouts):
    """The sections heap_reader.read_key_groups parsed ({kg: {state id: entries}}, states in the order read) under the
    writer layouts {state id: layout}: (bytes, section offsets)."""
    out, offs = bytearray(), []
    for kg in sorted(sections):
        offs.append(len(out))
        out += write_key_group(kg, [(sid, layouts[sid], ents) for sid, ents in sections[kg].items()])
    return bytes(out), offs
