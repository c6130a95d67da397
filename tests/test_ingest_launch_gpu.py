"""Every row of the two-phase ingest's launch table (flink_amd/csrc/ingest_launch.inc, FWA_P3_INSTANCES and
FWA_C3_INSTANCES) launched once on the GPU and checked against the oracle.

Each case is a handle configuration, options and inputs that plan_v2 maps to the partition3 / combine3 tuple written
next to it (tests/test_ingest_launch_cpu.py checks, without a GPU, that the cases cover exactly the rows of the two
lists, and that the oracle fires rows for each). A case makes two pushes of 20 000 records over about 3 000 keys --
more than two tiles of the largest tile, 8 x 1024 records, so at least two blocks run and a block's tile loop wraps --
and one watermark that fires every window; rows are bit-exact with the oracle. The first push finds no slice yet (its
records reach the slots through the v1 replay), the second one fills the buckets.

What selects a row: the aggregate list (value columns, their widths, the combiner layout), skew_merge (PRE),
window_passes (MP), narrow_entries, ingest_variant bits 1 and 10, the owned key-group range with JAVA_LONG keys
(KG 1) or PREHASHED ones (KG 2), and a key column that is not 16-byte aligned (W16 0 with every key group owned)."""
import functools

import numpy as np
import pytest

from flink_amd import _abi as A
from helpers import assert_rows_equal

N = 20_000                         # records per push
KEYS = 3_000
CAP = 4096
SIZE_MS = 1000
MAXP = 128
OWNED = (0, 63)                    # the key-group range of the KG 1 / KG 2 cases
MP = 2                             # FWA_MP_IT

# handle: aggregates, semantics, value column dtypes, nullable columns
COUNT = ([("COUNT", 0)], "DATASTREAM", ("i8",), ())                                    # no value column, layout 2
# (one BIGINT accumulator past COUNT, but no value to add: the general layout, not COUNT + SUM's)
CNT_COL = ([("COUNT", 0), ("COUNT_COL", 0)], "TABLE", ("i8",), (0,))                   # no value column, layout 0
CNT_COL2 = ([("COUNT_COL", 0), ("COUNT_COL", 1)], "TABLE", ("i8", "i8"), (0, 1))       # no value column, layout 0
SUM64 = ([("COUNT", 0), ("SUM_I64", 0)], "DATASTREAM", ("i8",), ())                    # 8-byte column, layout 1
MAX64 = ([("COUNT", 0), ("MAX_I64", 0)], "DATASTREAM", ("i8",), ())                    # 8-byte column, layout 0
MAX32 = ([("COUNT", 0), ("MAX_F32", 0)], "DATASTREAM", ("f4",), ())                    # 4-byte column, layout 0
F4F4 = ([("MAX_F32", 0), ("MIN_F32", 1)], "DATASTREAM", ("f4", "f4"), ())              # VW 0
F8F4 = ([("COUNT", 0), ("SUM_F64", 1), ("AVG_F64", 1), ("MAX_F32", 0), ("MAX_F64", 1)], "TABLE", ("f4", "f8"), ())  # VW 1
F4F8 = ([("MAX_F32", 0), ("SUM_F64", 1)], "DATASTREAM", ("f4", "f8"), ())              # VW 2
I8F8 = ([("MAX_I64", 0), ("SUM_F64", 1)], "DATASTREAM", ("i8", "f8"), ())              # VW 3


def case(handle, p3, c3, kg=0, unaligned=False, **options):
    opts = dict(skew_merge=0, window_passes=0, narrow_entries=0, ingest_variant=0)
    opts.update(options)
    return dict(handle=handle, p3=p3, c3=c3, kg=kg, unaligned=unaligned, options=opts)


# name: case(handle, partition3 (NV, ITEMS, VW, KG, PRE, W16, NW, ROLL), combine3 (IT, NV, LAYOUT, PRE, MP, NW, LEAN), ...)
CASES = {
    # PRE: Phase P merges a tile's equal (key, slice) records
    "pre-count": case(COUNT, (0, 4, 3, 0, 1, 0, 0, 0), (4, 0, 2, 1, 0, 0, 0), skew_merge=1),
    "pre-count-kg1-mp": case(COUNT, (0, 4, 3, 1, 1, 0, 0, 0), (MP, 0, 2, 1, 1, 0, 0), kg=1, skew_merge=1, window_passes=1),
    "pre-count-kg2": case(COUNT, (0, 4, 3, 2, 1, 0, 0, 0), (4, 0, 2, 1, 0, 0, 0), kg=2, skew_merge=1),
    "pre-sum": case(SUM64, (1, 4, 3, 0, 1, 0, 0, 0), (4, 1, 1, 1, 0, 0, 0), skew_merge=1),
    "pre-sum-kg1-mp": case(SUM64, (1, 4, 3, 1, 1, 0, 0, 0), (MP, 1, 1, 1, 1, 0, 0), kg=1, skew_merge=1, window_passes=1),
    "pre-sum-kg2": case(SUM64, (1, 4, 3, 2, 1, 0, 0, 0), (4, 1, 1, 1, 0, 0, 0), kg=2, skew_merge=1),
    # no value column, both combiner layouts, without and with window passes
    "count": case(COUNT, (0, 8, 3, 0, 0, 0, 0, 0), (4, 0, 2, 0, 0, 0, 0)),
    "count-mp": case(COUNT, (0, 8, 3, 0, 0, 0, 0, 0), (MP, 0, 2, 0, 1, 0, 0), window_passes=1),
    "countcol-kg1": case(CNT_COL, (0, 8, 3, 1, 0, 0, 0, 0), (4, 0, 0, 0, 0, 0, 0), kg=1),
    "countcol-mp": case(CNT_COL, (0, 8, 3, 0, 0, 0, 0, 0), (MP, 0, 0, 0, 1, 0, 0), window_passes=1),
    "countcol2-kg2": case(CNT_COL2, (0, 6, 3, 2, 0, 0, 0, 0), (4, 0, 0, 0, 0, 0, 0), kg=2),
    "countcol2-mp": case(CNT_COL2, (0, 8, 3, 0, 0, 0, 0, 0), (MP, 0, 0, 0, 1, 0, 0), window_passes=1),
    # narrow entries: rolling and burst loads, lean and general body, window passes; the two-column kind
    "narrow": case(SUM64, (1, 6, 3, 0, 0, 1, 1, 1), (6, 1, 1, 0, 0, 1, 3), narrow_entries=1),
    "narrow-burst-general": case(SUM64, (1, 6, 3, 0, 0, 1, 1, 0), (6, 1, 1, 0, 0, 1, 0), narrow_entries=1,
                                 ingest_variant=1024 | 2),
    "narrow-mp": case(SUM64, (1, 6, 3, 0, 0, 1, 1, 1), (MP, 1, 1, 0, 1, 1, 0), narrow_entries=1, window_passes=1),
    "narrow2": case(F8F4, (2, 4, 1, 0, 0, 0, 2, 0), (4, 2, 0, 0, 0, 2, 0), narrow_entries=1),
    "narrow2-mp": case(F8F4, (2, 4, 1, 0, 0, 0, 2, 0), (MP, 2, 0, 0, 1, 2, 0), narrow_entries=1, window_passes=1),
    # one value column, paired loads
    "sum-paired": case(SUM64, (1, 6, 3, 0, 0, 1, 0, 0), (4, 1, 1, 0, 0, 0, 0)),
    "max32-paired": case(MAX32, (1, 6, 2, 0, 0, 1, 0, 0), (4, 1, 0, 0, 0, 0, 0)),
    # one value column, one record per load: an unaligned key column, or key groups to check
    "sum-unaligned-mp": case(SUM64, (1, 6, 3, 0, 0, 0, 0, 0), (MP, 1, 1, 0, 1, 0, 0), unaligned=True, window_passes=1),
    "max64-kg1": case(MAX64, (1, 6, 3, 1, 0, 0, 0, 0), (4, 1, 0, 0, 0, 0, 0), kg=1),
    "sum-kg2": case(SUM64, (1, 4, 3, 2, 0, 0, 0, 0), (4, 1, 1, 0, 0, 0, 0), kg=2),
    "max32-unaligned-mp": case(MAX32, (1, 6, 2, 0, 0, 0, 0, 0), (MP, 1, 0, 0, 1, 0, 0), unaligned=True, window_passes=1),
    "max32-kg1": case(MAX32, (1, 6, 2, 1, 0, 0, 0, 0), (4, 1, 0, 0, 0, 0, 0), kg=1),
    "max32-kg2": case(MAX32, (1, 4, 2, 2, 0, 0, 0, 0), (4, 1, 0, 0, 0, 0, 0), kg=2),
    # two value columns: every pair of widths, every key-group mode
    "f4f4": case(F4F4, (2, 4, 0, 0, 0, 0, 0, 0), (3, 2, 0, 0, 0, 0, 0)),
    "f4f4-kg1": case(F4F4, (2, 4, 0, 1, 0, 0, 0, 0), (3, 2, 0, 0, 0, 0, 0), kg=1),
    "f4f4-kg2": case(F4F4, (2, 2, 0, 2, 0, 0, 0, 0), (3, 2, 0, 0, 0, 0, 0), kg=2),
    "f8f4": case(F8F4, (2, 4, 1, 0, 0, 0, 0, 0), (3, 2, 0, 0, 0, 0, 0)),
    "f8f4-kg1": case(F8F4, (2, 4, 1, 1, 0, 0, 0, 0), (3, 2, 0, 0, 0, 0, 0), kg=1),
    "f8f4-kg2": case(F8F4, (2, 2, 1, 2, 0, 0, 0, 0), (3, 2, 0, 0, 0, 0, 0), kg=2),
    "f4f8-mp": case(F4F8, (2, 4, 2, 0, 0, 0, 0, 0), (MP, 2, 0, 0, 1, 0, 0), window_passes=1),
    "f4f8-kg1": case(F4F8, (2, 4, 2, 1, 0, 0, 0, 0), (3, 2, 0, 0, 0, 0, 0), kg=1),
    "f4f8-kg2": case(F4F8, (2, 2, 2, 2, 0, 0, 0, 0), (3, 2, 0, 0, 0, 0, 0), kg=2),
    "i8f8": case(I8F8, (2, 4, 3, 0, 0, 0, 0, 0), (3, 2, 0, 0, 0, 0, 0)),
    "i8f8-kg1": case(I8F8, (2, 4, 3, 1, 0, 0, 0, 0), (3, 2, 0, 0, 0, 0, 0), kg=1),
    "i8f8-kg2": case(I8F8, (2, 2, 3, 2, 0, 0, 0, 0), (3, 2, 0, 0, 0, 0, 0), kg=2),
}


def key_hash_of(keys):
    return (keys * 31 + 7).astype(np.int32)


@functools.lru_cache(maxsize=None)
def key_pool(kg):
    """About 3 000 keys; with a key-group mode, keys of the owned range only (a record of another is an error)."""
    from oracle.oracle import lib
    cand = np.random.default_rng(5).permutation(np.arange(-20_000, 20_000, dtype=np.int64))
    if kg == 0:
        return cand[:KEYS]
    kind = A.KEY_PREHASHED if kg == 2 else A.KEY_JAVA_LONG
    hs = key_hash_of(cand) if kg == 2 else np.zeros(len(cand), np.int32)
    groups = np.array([lib().or_key_group(int(k), kind, int(h), MAXP) for k, h in zip(cand[:4 * KEYS], hs[:4 * KEYS])])
    return cand[:4 * KEYS][(groups >= OWNED[0]) & (groups <= OWNED[1])][:KEYS]


def make_cfg(c, owned=True):
    aggs, sem, _, nullable = c["handle"]
    kw = {}
    if c["kg"] and owned:
        kw.update(kg_start=OWNED[0], kg_end=OWNED[1])
    return A.make_config(window_kind="TUMBLE", semantics=sem, size_ms=SIZE_MS, aggs=aggs, key_capacity=CAP,
                         nullable_cols=nullable, max_parallelism=MAXP,
                         key_kind=A.KEY_PREHASHED if c["kg"] == 2 else A.KEY_JAVA_LONG, **kw)


@functools.lru_cache(maxsize=None)
def pushes(name):
    """The case's two pushes: (keys, ts, columns, key hashes or None, NULL flags or None). Values fit 32 bits (narrow
    entries stay narrow) and float columns hold small integers, so every sum is exact in any order."""
    c = CASES[name]
    _, _, dtypes, nullable = c["handle"]
    rng = np.random.default_rng(sorted(CASES).index(name))
    pool = key_pool(c["kg"])
    assert len(pool) > KEYS - 200
    out = []
    for p in range(2):
        k = rng.choice(pool, N).astype(np.int64)
        ts = rng.integers(p * SIZE_MS, (p + 3) * SIZE_MS, N).astype(np.int64)
        cols = [rng.integers(-2**31, 2**31, N).astype(np.int64) if d == "i8" else
                rng.integers(-1000, 1000, N).astype(np.dtype(d)) for d in dtypes]
        nulls = [(rng.random(N) < 0.01).astype(np.uint8) for _ in nullable] if nullable else None
        out.append((k, ts, cols, key_hash_of(k) if c["kg"] == 2 else None, nulls))
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's rows of the case's one watermark (the oracle owns every key group)."""
    from oracle.oracle import Oracle
    o = Oracle(make_cfg(CASES[name], owned=False))
    for k, ts, cols, kh, nulls in pushes(name):
        assert o.push(k, ts, cols, key_hash=kh, nulls=nulls) == 0
    rows = o.advance_watermark(A.LONG_MAX)
    o.close()
    return rows


@pytest.fixture(scope="module")
def eng_mod():
    from flink_amd import engine
    engine.lib()
    return engine


def to_device(x, shifted=False):
    """x on the GPU; shifted: a view one element into its buffer, so not 16-byte aligned."""
    import torch
    t = torch.from_numpy(x)
    off = int(shifted)
    buf = torch.empty(len(x) + 2, dtype=t.dtype, device="cuda:0")
    buf[off:off + len(x)] = t.to("cuda:0")
    v = buf[off:off + len(x)]
    assert (v.data_ptr() % 16 != 0) == shifted
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_row(eng_mod, name):
    c = CASES[name]
    cfg = make_cfg(c)
    g = eng_mod.WindowAggregator(cfg, options=c["options"])
    try:
        for k, ts, cols, kh, nulls in pushes(name):
            if c["unaligned"]:
                assert kh is None and nulls is None
                k, ts, cols = to_device(k, shifted=True), to_device(ts), [to_device(x) for x in cols]
            assert g.push(k, ts, cols, key_hash=kh, nulls=nulls) == 0
        rows = g.advance_watermark(A.LONG_MAX)
        for opt, value in c["options"].items():
            assert g.get_option(opt) == value, opt
        st = g.stats()
        assert st.records_in == 2 * N and st.late_dropped == 0
        assert st.partition_ms > 0 and st.combine_ms > 0, "the two-phase ingest did not run"
    finally:
        g.close()
    want = reference(name)
    assert len(want["key"]) > KEYS
    assert_rows_equal(rows, want, A.agg_names(cfg), ctx=name)
