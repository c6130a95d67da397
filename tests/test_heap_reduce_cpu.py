"""The heap-layout writer of tests/heap_tuple_ref.py against the reference's own checkpoint and against heap_reader.

win-op-migration-test-reduce-event-time-flink1.18-snapshot (WindowOperatorMigrationTest.java:366-440) holds a
ReducingState<Tuple2<String, Integer>> keyed by a String under TimeWindow namespaces, and its timers. The writer, fed the
entries heap_reader parsed from it in the file's own order, must give the file's key-group section byte for byte; and
random sections of tuples over all four field types and String keys (1-, 2- and 3-byte chars, the empty string) must
survive writer -> reader unchanged with every byte consumed."""
import os
import random

import heap_reader as H
import heap_tuple_ref as W

FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "flink_snapshots",
                       "win-op-migration-test-reduce-event-time-flink1.18-snapshot")
R_LAY = {0: ("kv", H.ser_time_window, H.ser_string, H.ser_tuple(H.ser_string, H.ser_int)),
         1: ("pq", H.ser_string, H.ser_time_window), 2: ("pq", H.ser_string, H.ser_time_window)}
W_LAY = {0: ("kv", W.w_time_window, W.w_string, W.w_tuple(W.w_string, W.w_int)),
         1: ("pq", W.w_string, W.w_time_window), 2: ("pq", W.w_string, W.w_time_window)}


def test_writer_reproduces_the_reference_section():
    first, offs, data = H.read_operator_snapshot(open(FIXTURE, "rb").read())[0]
    secs = H.read_key_groups(data, offs, first, R_LAY)
    assert sorted(secs) == list(range(first, first + len(offs)))
    assert len(secs[first][0]) == 3 and len(secs[first][2]) == 3        # 3 reduced tuples, 3 timers: not an empty file
    bounds = list(offs) + [len(data)]
    for i, kg in enumerate(sorted(secs)):
        mine = W.write_key_group(kg, [(sid, W_LAY[sid], ents) for sid, ents in secs[kg].items()])
        assert mine == data[bounds[i]:bounds[i + 1]]


def test_string_coding_and_hash():
    assert W.w_string(None) == b"\x00"
    assert W.w_string("") == b"\x01"
    assert W.w_string("key1") == b"\x05key1"
    assert W.w_string("é") == b"\x02\xe9\x01"                       # 0xE9: two 7-bit groups, low group first
    assert W.w_string("€") == b"\x02\xac\x41"                       # 0x20AC < 2^14: two bytes
    assert W.w_string("中") == b"\x02\xad\x9c\x01"                   # 0x4E2D: three bytes
    assert W.w_string("\U0001f600") == b"\x03" + W.w_string("\ud83d")[1:] + W.w_string("\ude00")[1:]   # a surrogate pair
    assert W.w_string("x" * 127)[:2] == b"\x80\x01"                  # len + 1 = 128: a two-byte varint
    assert W.java_string_hash("") == 0
    assert W.java_string_hash("key1") == ((107 * 31 + 101) * 31 + 121) * 31 + 49 == 3288498
    assert W.java_string_hash("zzzzzzzz") < 0                            # int wrap
    r = H.Reader(W.w_string("Straße €中") + W.w_string(None) + W.w_string(""))
    assert (H.ser_string(r), H.ser_string(r), H.ser_string(r)) == ("Straße €中", None, "") and r.at == r.end


def _rand_string(rng):
    pools = ["abcXYZ019_", "éßΩЖ", "€中文￿䀀", "\x00\x7f\x80㿿"]
    return "".join(rng.choice(rng.choice(pools)) for _ in range(rng.choice([0, 0, 1, 2, 5, 9, 40])))


def test_writer_reader_round_trip():
    rng = random.Random(5)
    fields = {"long": (W.w_long, H.ser_long, lambda: rng.randrange(-2**63, 2**63)),
              "int": (W.w_int, H.ser_int, lambda: rng.randrange(-2**31, 2**31)),
              "double": (W.w_double, W.ser_double, lambda: rng.randrange(0, 2**64)),
              "float": (W.w_float, W.ser_float, lambda: rng.randrange(0, 2**32)),
              "string": (W.w_string, H.ser_string, lambda: _rand_string(rng))}
    for trial in range(40):
        key_t = rng.choice(["long", "string"])
        shape = [rng.choice(["long", "int", "double", "float"]) for _ in range(rng.randrange(1, 5))]
        shape.insert(rng.randrange(0, len(shape) + 1), key_t)
        wl = {0: ("kv", W.w_time_window, fields[key_t][0], W.w_tuple(*[fields[t][0] for t in shape])),
              1: ("kv", W.w_void, fields[key_t][0], W.w_list(W.w_tuple(W.w_time_window, W.w_time_window))),
              2: ("pq", fields[key_t][0], W.w_time_window), 3: ("pq", fields[key_t][0], W.w_time_window)}
        rl = {0: ("kv", H.ser_time_window, fields[key_t][1], H.ser_tuple(*[fields[t][1] for t in shape])),
              1: ("kv", H.ser_void, fields[key_t][1], H.ser_list(H.ser_tuple(H.ser_time_window, H.ser_time_window))),
              2: ("pq", fields[key_t][1], H.ser_time_window), 3: ("pq", fields[key_t][1], H.ser_time_window)}
        secs = {}
        for kg in range(3):
            win = lambda: (lambda s: (s, s + rng.randrange(1, 10**6)))(rng.randrange(-2**40, 2**40))
            n = rng.randrange(0, 6)
            secs[kg] = {0: [(win(), fields[key_t][2](), tuple(fields[t][2]() for t in shape)) for _ in range(n)],
                        1: [(None, fields[key_t][2](), [(win(), win()) for _ in range(rng.randrange(0, 3))])
                            for _ in range(rng.randrange(0, 3))],
                        2: [],
                        3: [(rng.choice([-2**63, -1, 0, 2999, 2**63 - 1]), fields[key_t][2](), win()) for _ in range(n)]}
        body, offs = W.write_key_groups(secs, wl)
        back = H.read_key_groups(body, offs, 0, rl)                      # (asserts that no read passes a section)
        assert back == secs, (trial, shape)
        again, offs2 = W.write_key_groups(back, wl)
        assert again == body and offs2 == offs
