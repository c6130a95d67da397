"""tests/key_place.py without a GPU: the hash's inverse, the aimed key sets, and the sequential table model against
key_slot's own arithmetic (jm::mix64 of java_math.h and the segment base / aligned home lines of ingest.inc, compiled
for the host). Every property a key set of tests/test_key_place_gpu.py is named for is asserted here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import key_place as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(10, 0), (12, 0), (12, 1), (9, 4), (13, 1)]

# key_slot's lines (ingest.inc): seg_base, smask and home, with kBucket = 8
PROBE = r'''
#include <stdint.h>
#include "java_math.h"
static const int kBucket = 8;
static uint64_t seg_base(uint64_t h, int seg_log, int part_bits) {
    return part_bits ? ((h >> (64 - part_bits)) << seg_log) : 0ull;
}
extern "C" {
void t_mix64(const uint64_t* z, int64_t n, uint64_t* out) { for (int64_t i = 0; i < n; ++i) out[i] = jm::mix64(z[i]); }
void t_place(const int64_t* keys, int64_t n, int seg_log, int part_bits, uint64_t* base_out, uint64_t* home_out) {
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t h = jm::mix64((uint64_t)keys[i]);
        const uint64_t base = seg_base(h, seg_log, part_bits);
        const uint64_t smask = ((uint64_t)1 << seg_log) - 1;
        const uint64_t home = h & smask & ~(uint64_t)(kBucket - 1);
        base_out[i] = base;
        home_out[i] = home;
    }
}
}
'''


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("key_place")
    src = d / "probe.cpp"
    src.write_text(PROBE)
    so = d / "probe.so"
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "flink_amd", "csrc"),
                           str(src), "-o", str(so)])
    L = ctypes.CDLL(str(so))
    L.t_mix64.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    L.t_mix64.restype = None
    L.t_place.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.t_place.restype = None
    return L


def test_restated_lines_are_key_slots():
    """The probe library restates three lines of key_slot; they must still be in the source as restated."""
    src = open(os.path.join(ROOT, "flink_amd", "csrc", "ingest.inc")).read()
    for line in ("return part_bits ? ((h >> (64 - part_bits)) << seg_log) : 0ull;",
                 "const uint64_t smask = ((uint64_t)1 << seg_log) - 1;",
                 "const uint64_t home = h & smask & ~(uint64_t)(kBucket - 1);",
                 "const uint64_t i = base | ((home + probe) & smask);",
                 "constexpr int kBucket = 8;",
                 "constexpr uint64_t kEmptyKey = 0x8000000000000000ull;"):
        assert line in src, line


def test_unmix64_inverts_mix64_both_ways(probe):
    rng = np.random.default_rng(1)
    vals = [0, 1, 1 << 63, (1 << 64) - 1] + [int(x) for x in rng.integers(0, 1 << 64, 20_000, dtype=np.uint64)]
    for v in vals:
        assert K.unmix64(K.mix64_int(v)) == v
        assert K.mix64_int(K.unmix64(v)) == v
    a = np.array(vals, np.uint64)
    out = np.empty_like(a)
    probe.t_mix64(a.ctypes.data, len(a), out.ctypes.data)        # the engine's own mix64, the array form, the int form
    assert out.tolist() == K.mix64(a).tolist() == [K.mix64_int(v) for v in vals]
    assert K.mix64(np.array([-1, K.LONG_MIN], np.int64)).tolist() == [K.mix64_int(-1), K.mix64_int(1 << 63)]


@pytest.mark.parametrize("shape", SHAPES)
def test_keys_at_returns_the_requested_place(shape):
    rng = np.random.default_rng(2)
    nb, ns = K.n_buckets(shape), K.n_segments(shape)
    for segment, bucket in {(0, 0), (ns - 1, nb - 1), (ns // 2, nb // 2), (ns - 1, 0), (0, nb - 1)}:
        keys = K.keys_at(shape, segment, bucket, 64, rng)
        assert keys.dtype == np.int64 and len(set(keys.tolist())) == 64
        assert set(K.segment_of(shape, keys).tolist()) == {segment}
        assert set(K.bucket_of(shape, keys).tolist()) == {bucket}
        assert all(not (-(1 << 31) <= k < (1 << 31)) and k != K.LONG_MIN for k in keys.tolist())
        more = K.keys_at(shape, segment, bucket, 16, rng, exclude=keys)
        assert not set(more.tolist()) & set(keys.tolist())
    if shape == (9, 4):                                         # narrow keys are found by search (one shape: 1 s)
        keys = K.keys_at(shape, ns - 1, nb - 1, 40, rng, wide=False)
        assert set(K.place_of(shape, keys).tolist()) == {ns * nb - 1} and len(set(keys.tolist())) == 40
        assert all(-(1 << 31) <= k < (1 << 31) for k in keys.tolist())


@pytest.mark.parametrize("shape", SHAPES)
def test_model_places_keys_where_key_slot_does(probe, shape):
    """Segment base and aligned home of 10^4 random keys (and the extreme ones) from key_slot's lines compiled for the
    host; the model's slot of a key inserted into an empty table is base | home."""
    rng = np.random.default_rng(3)
    ends, fam = K.edge_set()
    keys = np.r_[rng.integers(-(1 << 63), (1 << 63) - 1, 10_000, dtype=np.int64, endpoint=True),
                 ends[ends != K.LONG_MIN], fam]
    base = np.empty(len(keys), np.uint64)
    home = np.empty(len(keys), np.uint64)
    probe.t_place(keys.ctypes.data, len(keys), shape[0], shape[1], base.ctypes.data, home.ctypes.data)
    t = K.Table(shape)
    assert [t.home(k) for k in keys.tolist()] == list(zip(base.tolist(), home.tolist()))
    seg = 1 << shape[0]
    assert (K.segment_of(shape, keys) * seg).tolist() == base.tolist()
    assert (K.bucket_of(shape, keys) * 8).tolist() == home.tolist()
    assert int(base.max()) + seg == t.capacity and int(home.max()) == seg - 8          # every segment, the last bucket
    for k in keys[:200].tolist():
        e = K.Table(shape)
        assert e.insert(k) == e.home(k)[0] | e.home(k)[1] == e.find(k)
    assert K.Table(shape).insert(K.LONG_MIN) == t.capacity                              # the side slot


def test_model_probes_linearly_and_wraps_inside_the_segment():
    shape = (10, 1)
    rng = np.random.default_rng(4)
    keys = K.keys_at(shape, 0, K.n_buckets(shape) - 1, 12, rng)
    t, slots = K.place_all(shape, keys)
    assert slots == list(range(1016, 1024)) + [0, 1, 2, 3] and t.wrapped and t.max_disp == 1 and t.n_keys == 12
    assert [t.insert(k) for k in keys] == slots and t.n_keys == 12                       # found again, not inserted
    assert [t.find(k) for k in keys] == slots and t.find(12345) == -1
    assert t.segment_load(0) == 12 and t.segment_load(1) == 0
    d0 = K.Table(shape).digest()
    assert t.digest() != d0 and K.place_all(shape, keys)[0].digest() == t.digest()
    assert K.place_all(shape, keys[::-1])[0].digest() != t.digest()                      # the digest sees the order
    # FNV-1a restated over an empty 2-slot table by hand: the two empty words, then the side slot's zero
    h = 0xcbf29ce484222325
    for b in [0, 0, 0, 0, 0, 0, 0, 0x80] * 2 + [0] * 8:
        h = ((h ^ b) * 0x100000001b3) & K.M64
    e = K.Table((1, 0))
    assert e.digest() == K.signed(h)


@pytest.mark.parametrize("shape", SHAPES)
def test_sets_have_the_property_they_are_named_for(shape):
    rng = np.random.default_rng(5)
    K.check_chain(shape, K.chain_set(shape, rng))
    for segment in K.wrap_segments(shape):
        main, own, other = K.wrap_set(shape, rng, segment)
        K.check_wrap(shape, main, own, other)
        K.check_wrap(shape, main, own, other, order=np.r_[own, other, main])
        assert len(other) == (8 if shape[1] else 0)
    K.check_dense(shape, K.dense_set(shape, rng))
    K.check_race(shape, *K.race_set(shape, rng))
    assert K.wrap_segments(shape) == {0: [0], 1: [0, 1], 4: [0, 8, 15]}[shape[1]]


def test_edge_set():
    ends, fam = K.edge_set()
    assert set(ends.tolist()) == {0, 1, -1, (1 << 63) - 1, -(1 << 63), -(1 << 63) + 1}
    assert len(fam) == 20 and len(set(fam.tolist())) == 20
    t, slots = K.place_all((10, 0), np.r_[ends, fam])
    assert slots[4] == 1024 and len(set(slots)) == 26 and t.n_keys == 26


@pytest.mark.parametrize("shape", [(10, 0), (12, 1)])
def test_full_set_fills_exactly_one_segment(shape):
    """The two smallest shapes: the 1024-slot single-segment table and the two-segment table of key_capacity 4096."""
    rng = np.random.default_rng(6)
    segment = K.n_segments(shape) - 1
    parts, extra, other = K.full_set(shape, rng, segment)
    t = K.check_full(shape, parts, extra, other)
    assert sum(len(p) for p in parts) == 1 << shape[0] and all(len(p) > 0 for p in parts)
    assert (other is None) == (shape[1] == 0)
    assert t.max_disp >= 2
