"""Key sets aimed at chosen places of the engine's key table, and a sequential model of that table (no GPU).

The table (key_slot, flink_amd/csrc/ingest.inc) is 2^part_bits segments of 2^seg_log slots. h = mix64(key): the top
part_bits of h pick the segment, the low seg_log bits rounded down to an 8-slot bucket pick the home slot inside it,
probing is linear and wraps inside the segment; Long.MIN_VALUE (the empty mark) lives in a side slot at `capacity`.
A handle reports its shape through FWA_OPT_KEY_TABLE_SHAPE ("key_table_shape": seg_log | part_bits << 8).

mix64 is a bijection of the 64-bit words, so a key for a place is built backwards: choose the segment and the home
bucket, fill the other hash bits at random, and invert."""
import functools

import numpy as np

M64 = (1 << 64) - 1
BUCKET = 8
LONG_MIN = -(1 << 63)
EMPTY = 1 << 63                            # kEmptyKey: the table's empty word, Long.MIN_VALUE as unsigned
C1, C2 = 0xbf58476d1ce4e5b9, 0x94d049bb133111eb
C1_INV, C2_INV = 0x96de1b173f119089, 0x319642b2d24d8ec3
assert C1 * C1_INV & M64 == 1 and C2 * C2_INV & M64 == 1


def mix64(z):
    """jm::mix64 (java_math.h) of int64 / uint64 values, as uint64 (an array in, an array out; a scalar as an array)."""
    z = np.asarray(z)
    z = z.astype(np.int64).astype(np.uint64) if z.dtype != np.uint64 else z
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(C1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(C2)
    return z ^ (z >> np.uint64(31))


def mix64_int(z):
    """mix64 of one Python integer (any sign), as an unsigned Python integer."""
    z &= M64
    z = ((z ^ (z >> 30)) * C1) & M64
    z = ((z ^ (z >> 27)) * C2) & M64
    return z ^ (z >> 31)


def _unshift(y, s):
    """x with x ^ (x >> s) == y: each round fixes s more bits from the top."""
    x = y
    for _ in range(64 // s + 1):
        x = y ^ (x >> s)
    return x


def unmix64(h):
    """The exact inverse of mix64 on one Python integer: unmix64(mix64_int(k)) == k & M64."""
    h &= M64
    h = _unshift(h, 31)
    h = (h * C2_INV) & M64
    h = _unshift(h, 27)
    h = (h * C1_INV) & M64
    return _unshift(h, 30)


def signed(u):
    return u - (1 << 64) if u >> 63 else u


def shape_of(value):
    """(seg_log, part_bits) of an FWA_OPT_KEY_TABLE_SHAPE value."""
    return int(value) & 0xff, int(value) >> 8


def segment_of(shape, keys):
    seg_log, part_bits = shape
    h = mix64(keys)
    return (h >> np.uint64(64 - part_bits)).astype(np.int64) if part_bits else np.zeros(h.shape, np.int64)


def bucket_of(shape, keys):
    seg_log, part_bits = shape
    return ((mix64(keys) & np.uint64((1 << seg_log) - 1)) >> np.uint64(3)).astype(np.int64)


def place_of(shape, keys):
    """(segment, home bucket) of each key as one number: segment * buckets per segment + bucket."""
    return segment_of(shape, keys) * (1 << (shape[0] - 3)) + bucket_of(shape, keys)


def n_segments(shape):
    return 1 << shape[1]


def n_buckets(shape):
    return 1 << (shape[0] - 3)


@functools.lru_cache(maxsize=8)
def _narrow_pool(shape):
    """The keys of [-2^21, 2^21) sorted by place, and their places."""
    cand = np.arange(-(1 << 21), 1 << 21, dtype=np.int64)
    pl = place_of(shape, cand)
    order = np.argsort(pl, kind="stable")
    return cand[order], pl[order]


def keys_at(shape, segment, bucket, count, rng, wide=True, exclude=(), keep=None):
    """`count` distinct int64 keys whose hash has that segment and home bucket (an int64 array). wide: only keys
    outside the signed 32-bit range, which no narrow-entry path takes; wide=False: only keys inside it (found by
    search among 2^22 small keys, so for tables of up to about 2^16 slots). bucket None: a home bucket chosen at random per key (wide only). Never
    Long.MIN_VALUE, never a key of `exclude`; keep(key) -> bool: a further filter (a handle's owned key groups)."""
    seg_log, part_bits = shape
    assert 0 <= segment < (1 << part_bits) and (bucket is None or 0 <= bucket < (1 << (seg_log - 3)))
    seen = set(int(x) for x in exclude)
    out = []
    if not wide:
        cand, pl = _narrow_pool(shape)
        want = segment * (1 << (seg_log - 3)) + bucket
        lo, hi = np.searchsorted(pl, [want, want + 1])
        for k in rng.permutation(cand[lo:hi]).tolist():
            if k not in seen and len(out) < count and (keep is None or keep(k)):
                seen.add(k)
                out.append(k)
        assert len(out) == count, "no more narrow keys of that place"
        return np.array(out, np.int64)
    free = 64 - part_bits - seg_log + 3                    # hash bits a place leaves open
    while len(out) < count:
        mid = int(rng.integers(0, 1 << 62)) & ((1 << (free - 3)) - 1)
        low = int(rng.integers(0, BUCKET))
        b = int(rng.integers(0, 1 << (seg_log - 3))) if bucket is None else bucket
        h = (segment << (64 - part_bits) if part_bits else 0) | (mid << seg_log) | (b << 3) | low
        k = signed(unmix64(h))
        if k == LONG_MIN or k in seen or -(1 << 31) <= k < (1 << 31) or (keep is not None and not keep(k)):
            continue
        seen.add(k)
        out.append(k)
    return np.array(out, np.int64)


class Table:
    """key_slot, one key after the other, over an empty table of the shape. insert() returns the slot (kid), or -1
    when the key's segment is full; the table remembers the worst displacement and whether a probe wrapped."""

    def __init__(self, shape):
        self.seg_log, self.part_bits = shape
        self.capacity = 1 << (self.seg_log + self.part_bits)
        self.words = [EMPTY] * self.capacity + [0]          # [capacity]: the side slot of Long.MIN_VALUE, 0 or 1
        self.max_disp = 0                                   # largest distance slot - home, in buckets
        self.wrapped = False                                # a key was placed or found past its segment's end
        self.n_keys = 0

    def home(self, key):
        """(segment base, bucket-aligned home inside the segment)."""
        h = mix64_int(int(key))
        smask = (1 << self.seg_log) - 1
        base = (h >> (64 - self.part_bits)) << self.seg_log if self.part_bits else 0
        return base, h & smask & ~(BUCKET - 1)

    def insert(self, key):
        key = int(key)
        if key == LONG_MIN:
            if self.words[self.capacity] != 1:
                self.words[self.capacity] = 1
                self.n_keys += 1
            return self.capacity
        u = key & M64
        base, home = self.home(key)
        smask = (1 << self.seg_log) - 1
        for probe in range(smask + 1):
            i = base | ((home + probe) & smask)
            if self.words[i] == u or self.words[i] == EMPTY:
                if self.words[i] == EMPTY:
                    self.words[i] = u
                    self.n_keys += 1
                self.max_disp = max(self.max_disp, probe // BUCKET)
                self.wrapped = self.wrapped or home + probe > smask
                return i
        return -1

    def find(self, key):
        key = int(key)
        if key == LONG_MIN:
            return self.capacity if self.words[self.capacity] == 1 else -1
        base, home = self.home(key)
        smask = (1 << self.seg_log) - 1
        for probe in range(smask + 1):
            i = base | ((home + probe) & smask)
            if self.words[i] == key & M64:
                return i
            if self.words[i] == EMPTY:
                return -1
        return -1

    def segment_load(self, segment):
        seg = 1 << self.seg_log
        return sum(w != EMPTY for w in self.words[segment * seg:(segment + 1) * seg])

    def digest(self):
        """FWA_OPT_KEY_TABLE_DIGEST (fwa_get_option, engine.hip): FNV-1a over the bytes of the table's 64-bit words
        in slot order, each word low byte first, the side slot last; as the signed 64-bit value the option returns."""
        h = 0xcbf29ce484222325
        for b in np.array(self.words, np.uint64).astype("<u8").tobytes():
            h = ((h ^ b) * 0x100000001b3) & M64
        return signed(h)


def place_all(shape, keys):
    """A Table with `keys` inserted in that order, and their slots."""
    t = Table(shape)
    return t, [t.insert(k) for k in keys]


# ---- the named sets (each returns int64 keys; what a set is named for is checked with check_*) ----

def chain_set(shape, rng, segment=None, **kw):
    """40 keys of one mid-segment home bucket."""
    segment = n_segments(shape) // 2 if segment is None else segment
    return keys_at(shape, segment, n_buckets(shape) // 2, 40, rng, **kw)


def check_chain(shape, keys):
    t, slots = place_all(shape, keys)
    assert len(set(place_of(shape, keys).tolist())) == 1 and len(set(keys.tolist())) == len(keys) == 40
    disp = [(s - (t.home(k)[0] | t.home(k)[1])) // BUCKET for k, s in zip(keys.tolist(), slots)]
    assert max(disp) == 4 and min(disp) == 0 and 2 <= t.max_disp <= 5 and not t.wrapped
    assert sum(d >= 2 for d in disp) == 24                 # most of the set lives 2 to 4 buckets from home
    return t


def wrap_segments(shape):
    """Segment 0, the last one and a middle one, where there are several."""
    n = n_segments(shape)
    return sorted({0, n - 1, n // 2})


def wrap_set(shape, rng, segment, **kw):
    """(40 keys homed in the segment's last bucket, 8 guards homed in its bucket 0, 8 guards homed in bucket 0 of the
    next segment -- empty when the table has one segment)."""
    main = keys_at(shape, segment, n_buckets(shape) - 1, 40, rng, **kw)
    own = keys_at(shape, segment, 0, 8, rng, exclude=main, **kw)
    nxt = (segment + 1) % n_segments(shape)
    other = keys_at(shape, nxt, 0, 8, rng, exclude=np.r_[main, own], **kw) if nxt != segment else main[:0]
    return main, own, other


def check_wrap(shape, main, own, other, order=None):
    """The 40 keys run on from the segment's last bucket into its first ones, whichever of main / own came first; the
    next segment's guards stay in their bucket 0."""
    keys = np.r_[main, own, other] if order is None else order
    t, slots = place_all(shape, keys)
    seg = 1 << shape[0]
    segment = int(segment_of(shape, main[:1])[0])
    at = dict(zip(keys.tolist(), slots))
    inside = [at[k] - segment * seg for k in main.tolist()]
    assert t.wrapped and all(0 <= s < seg for s in inside)
    assert sum(s >= seg - BUCKET for s in inside) == 8 and sum(s < 6 * BUCKET for s in inside) == 32
    if len(other):
        nb = int(segment_of(shape, other[:1])[0]) * seg
        assert sorted(at[k] for k in other.tolist()) == list(range(nb, nb + 8))
    assert t.segment_load(segment) == 48
    return t


def dense_set(shape, rng, segment=None, m=6, **kw):
    """3 * 8 * m keys homed in m consecutive buckets (3 bucketfuls each)."""
    segment = n_segments(shape) // 2 if segment is None else segment
    b0 = n_buckets(shape) // 4
    got = []
    for b in range(b0, b0 + m):
        got.append(keys_at(shape, segment, b, 3 * BUCKET, rng, exclude=np.concatenate(got) if got else (), **kw))
    return rng.permutation(np.concatenate(got))


def check_dense(shape, keys, m=6):
    t, _ = place_all(shape, keys)
    assert len(keys) == 3 * BUCKET * m and len(set(bucket_of(shape, keys).tolist())) == m
    assert t.max_disp >= 2 * m - 1 and not t.wrapped          # the last bucket's keys walk through full buckets
    return t


def race_set(shape, rng, segment=None, **kw):
    """(one key for every lane of a tile, 24 distinct keys of one home bucket)."""
    segment = n_segments(shape) // 2 if segment is None else segment
    b = n_buckets(shape) // 8
    same = keys_at(shape, segment, b + 3, 1, rng, **kw)
    many = keys_at(shape, segment, b, 24, rng, exclude=same, **kw)
    return same, many


def check_race(shape, same, many):
    assert len(set(place_of(shape, many).tolist())) == 1 and len(set(many.tolist())) == 24
    t, _ = place_all(shape, np.r_[many, same])
    assert t.max_disp == 2
    return t


def edge_set():
    """(the extreme keys, families equal in their low 32 bits that must stay distinct keys)."""
    ends = np.array([0, 1, -1, (1 << 63) - 1, LONG_MIN, LONG_MIN + 1], np.int64)
    fam = []
    for k in (5, -7, 0x7fffffff, -(1 << 31), 123456789):
        fam += [k, k + (1 << 32), k - (1 << 32), signed((k & M64) ^ (1 << 63))]
    fam = np.array(fam, np.int64)
    assert len(set(fam.tolist()) | set(ends.tolist())) == len(fam) + len(ends)
    assert all(len(set((fam[i:i + 4] & 0xffffffff).tolist())) == 1 for i in range(0, len(fam), 4))
    return ends, fam


def full_set(shape, rng, segment):
    """(exactly 2^seg_log keys of the segment in three parts, one more key of it, one key of another segment or None).
    The keys are spread over every home bucket at random, as a hash would."""
    seg_log, part_bits = shape
    seg = 1 << seg_log
    keys = keys_at(shape, segment, None, seg + 1, rng)
    other = keys_at(shape, (segment + 1) % n_segments(shape), 3, 1, rng) if part_bits else None
    a, b = seg // 2, seg - 40
    return [keys[:a], keys[a:b], keys[b:seg]], keys[seg:], other


def check_full(shape, parts, extra, other):
    keys = np.concatenate(parts)
    segment = int(segment_of(shape, keys[:1])[0])
    t, slots = place_all(shape, keys)
    assert len(keys) == 1 << shape[0] and min(slots) >= 0 and len(set(slots)) == len(slots)
    assert t.segment_load(segment) == 1 << shape[0] and t.wrapped
    assert set(segment_of(shape, np.r_[keys, extra]).tolist()) == {segment}
    assert t.find(int(extra[0])) == -1 and t.insert(int(extra[0])) == -1          # the segment is full
    if other is not None:
        assert int(segment_of(shape, other)[0]) != segment and t.insert(int(other[0])) >= 0
    return t
