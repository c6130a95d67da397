"""Time-axis parity on the GPU: every device copy of "timestamp -> slice number" (for sessions: cell number) against
the oracle, bit for bit, along the axis the rest of the suite barely moves on -- slice sizes of all three modes of
jm::udiv64_make on both sides of Phase P's g * 4096 < 2^32 bound, time bases at 0 (both signs of ts - offset, the exact
negative multiple of g included), at +-1.7e12 (today's epoch), at +-2^62, and first live slice numbers on both sides of
+-2^40. tests/test_time_axis_cpu.py shows, without a GPU, that the oracle equals plain big-integer arithmetic
(tests/time_axis_ref.py) over the same matrix, so equality with the oracle is equality with the integers.

  (a) the two-phase ingest over the whole matrix, FWA_OPT_FAST_SLICE_PUSHES telling which form of Phase P's division ran;
  (b) the edges of Phase P's relative tables (32 entries by value, 4096 uploaded, the v1 replay past them);
  (c) the other copies: the v1 ingest, sliding / HOP / CUMULATE fires, the late fire, reductions, record lists, partial
      rows, the distinct sets and the float32 fold (host slice_q), the session cells, snapshot / restore.

Combinations fwa_create refuses for a reason include/flink_amd.h documents are asserted as refusals (REFUSED below);
nothing else is left out.

  REFUSED (what, the header's reason, status)
  fold_size_1, fold_size_3    FWA_CFG_F32_FOLD: windows shorter than 4 ms                       FWA_E_UNSUPPORTED
  distinct_size_7             FWA_COUNT_DISTINCT on TUMBLE: size_ms >= 64                       FWA_E_UNSUPPORTED
  hop_600000_420000,          Table SLIDE / CUMULATE: size_ms a multiple of slide_ms            FWA_E_ARG
  cumulate_600000_420000      (fwa_config.slide_ms; the reference refuses it too)
"""
import functools

import numpy as np
import pytest

import time_axis_ref as R
from flink_amd import _abi as A
from helpers import assert_rows_equal

pytestmark = pytest.mark.gpu

N = 20_000                         # records per push of (a) and (b): two blocks and a wrapped tile loop
CAP = 4096
NC, KEYS_C = 6000, 500             # (c)
P40 = 1 << 40

REFUSED = {
    "fold_size_1": (dict(window_kind="TUMBLE", size_ms=1, f32_fold=True, aggs=[("COUNT", 0), ("SUM_F32", 0)]), -7),
    "fold_size_3": (dict(window_kind="TUMBLE", size_ms=3, f32_fold=True, aggs=[("COUNT", 0), ("SUM_F32", 0)]), -7),
    "distinct_size_7": (dict(window_kind="TUMBLE", semantics="TABLE", size_ms=7, offset_ms=-2,
                             aggs=[("COUNT", 0), ("COUNT_DISTINCT", 0)]), -7),
    "hop_600000_420000": (dict(window_kind="SLIDE", semantics="TABLE", size_ms=600_000, slide_ms=420_000), -1),
    "cumulate_600000_420000": (dict(window_kind="CUMULATE", semantics="TABLE", size_ms=600_000, slide_ms=420_000), -1),
}


@pytest.fixture(scope="module")
def eng_mod():
    from flink_amd import engine
    engine.lib()
    return engine


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_documented_refusals(eng_mod, name):
    kw, code = REFUSED[name]
    with pytest.raises(eng_mod.EngineError) as ei:
        eng_mod.WindowAggregator(A.make_config(**kw))
    assert ei.value.code == code, str(ei.value)


def seed_of(*parts):
    import random
    return random.Random(repr(parts)).randrange(1 << 31)


def drive(eng_mod, cfg, steps, options=None, ocfg=None, late_idx=False, after_push=None, read=(), ctx=""):
    """Push every step (keys, ts, cols, nulls, watermarks) into a handle and the oracle: equal drop counts per push
    (and dropped record indices with late_idx), exactly equal rows per watermark. Returns (stats, {option: value})."""
    from oracle.oracle import Oracle
    names = A.agg_names(ocfg or cfg)
    g = eng_mod.WindowAggregator(cfg, options=options)
    o = Oracle(ocfg or cfg)
    try:
        for i, (k, ts, cols, nulls, wms) in enumerate(steps):
            dg, do = g.push(k, ts, cols, nulls=nulls), o.push(k, ts, cols, nulls=nulls)
            assert dg == do, "%s push %d: dropped %d, the oracle %d" % (ctx, i, dg, do)
            if late_idx:
                assert np.array_equal(g.late_records(), o.late_records()), "%s push %d: late record indices" % (ctx, i)
            if after_push:
                after_push(g, i)
            for wm in wms:
                assert_rows_equal(g.advance_watermark(wm), o.advance_watermark(wm), names, ctx="%s push %d wm %d" % (ctx, i, wm))
        st, ost = g.stats(), o.stats()
        assert st.late_dropped == ost.late_dropped and ost.rows_out > 0, ctx
        return st, {name: g.get_option(name) for name in read}
    finally:
        g.close()
        o.close()


# ---- (a) the two-phase ingest over the whole matrix --------------------------------------------------------------
A_SIZES = (1, 3, 7, 1000, 524_288, 524_289, 600_000, 1_048_575, 1_048_576, 1_048_577, 3_600_000, 86_400_000,
           604_800_000)
FAST_SIZES = tuple(g for g in A_SIZES if g * R.REL_CAP < 1 << 32)


def a_bases(g, narrow_matrix=False):
    b = {"zero": 0, "p1.7e12": 1_700_000_000_000}
    if narrow_matrix:
        return b
    b.update({"m1.7e12": -1_700_000_000_000, "p2^62": 1 << 62, "m2^62": -(1 << 62)})
    if g <= 1_048_575:   # first live slice numbers wholly inside and wholly outside +-2^40
        b.update({"in+2^40": (P40 - 10) * g, "out+2^40": (P40 + 4) * g, "in-2^40": -(P40 - 4) * g,
                  "out-2^40": -(P40 + 10) * g})
    return b


def a_cases(narrow_matrix=False):
    out = []
    for g in A_SIZES:
        for bname, base in a_bases(g, narrow_matrix).items():
            for off in sorted({0, -(g // 3)}, reverse=True):
                out.append(pytest.param(g, base, off, id="%d-%s-off%d" % (g, bname, off)))
    return out


def a_steps(g, base, off, wide):
    """Three pushes over slices q0 - 3 .. q0 + 3; a watermark after push 2 fires and retires the two earliest slices,
    whose records in push 3 are late. Returns (steps, the first live slice number each push meets)."""
    q0 = R.slice_number(base, off, g)
    s = [R.build_stream(base, off, g, N, seed_of("a", g, base, off, wide, p), wide=wide) for p in range(3)]
    wm1 = R.slice_first_ms(q0 - 1, off, g) - 1
    steps = [(s[0][0], s[0][1], [s[0][2]], None, []), (s[1][0], s[1][1], [s[1][2]], None, [wm1]),
             (s[2][0], s[2][1], [s[2][2]], None, [A.LONG_MAX])]
    return steps, [0, q0 - 3, q0 - 1]


def run_a(eng_mod, g, base, off, aggs, options, wide):
    steps, q_bases = a_steps(g, base, off, wide)
    cfg = A.make_config(window_kind="TUMBLE", size_ms=g, offset_ms=off, aggs=aggs, key_capacity=CAP)
    ctx = "g=%d base=%d off=%d" % (g, base, off)
    st, opt = drive(eng_mod, cfg, steps, options=options, read=("fast_slice_pushes",), ctx=ctx)
    assert st.partition_ms > 0 and st.combine_ms > 0, "the two-phase ingest did not run"
    assert st.late_dropped > N // 7, "push 3 carries records of the retired slices"
    want = sum(R.fast_form_expected(g, q, False, off) for q in q_bases)
    assert opt["fast_slice_pushes"] == want, "%s: %d fast pushes, expected %d (first live slices %s)" % (
        ctx, opt["fast_slice_pushes"], want, q_bases)
    if g * R.REL_CAP >= 1 << 32:
        assert opt["fast_slice_pushes"] == 0
    return opt["fast_slice_pushes"]


@pytest.mark.parametrize("g,base,off", a_cases())
def test_two_phase_narrow_count_sum(eng_mod, g, base, off):
    """[COUNT, SUM_I64] with default options: narrow entries, rolling loads."""
    fast = run_a(eng_mod, g, base, off, [("COUNT", 0), ("SUM_I64", 0)], None, wide=False)
    if g in FAST_SIZES and abs(R.slice_number(base, off, g)) < P40 - 16:
        assert fast == 3 if base == 0 else fast >= 2      # the 32-bit form ran on the pushes that meet live slices


@pytest.mark.parametrize("g,base,off", a_cases(narrow_matrix=True))
def test_two_phase_general_count_max_64bit(eng_mod, g, base, off):
    """[COUNT, MAX_I64], narrow_entries = 0: the general layout with 64-bit entries; keys and values need 64 bits."""
    run_a(eng_mod, g, base, off, [("COUNT", 0), ("MAX_I64", 0)], dict(narrow_entries=0), wide=True)


@pytest.mark.parametrize("sign", [1, -1], ids=["+2^40", "-2^40"])
@pytest.mark.parametrize("g", [g for g in A_SIZES if g * P40 < 1 << 62])
def test_stream_crosses_slice_2_to_the_40_between_pushes(eng_mod, g, sign):
    """The first live slice number moves across +-2^40 from push to push: Phase P changes form on a live handle. (Sizes
    whose slice 2^40 lies inside +-2^62 ms.)"""
    off = -(g // 3)
    qs = sorted(sign * P40 + d for d in (-6, -1, 4))
    steps = []
    for p, q in enumerate(qs):
        k, ts, v = R.build_stream(q * g + off, off, g, N, seed_of("cross", g, sign, p))
        assert R.slice_number(int(ts.min()), off, g) == q - 3 and R.slice_number(int(ts.max()), off, g) == q + 3
        wm = R.slice_first_ms(qs[p + 1] - 3, off, g) - 1 if p < 2 else A.LONG_MAX
        steps.append((k, ts, [v], None, [wm]))
    cfg = A.make_config(window_kind="TUMBLE", size_ms=g, offset_ms=off, aggs=[("COUNT", 0), ("SUM_I64", 0)], key_capacity=CAP)
    st, _ = drive(eng_mod, cfg, steps, ctx="cross g=%d sign=%d" % (g, sign))
    assert st.partition_ms > 0 and st.combine_ms > 0


# ---- (b) edges of the relative tables -----------------------------------------------------------------------------
TABLE_EDGES = (0, R.REL_TAB - 1, R.REL_TAB, R.REL_CAP - 1, R.REL_CAP, 5000)


@pytest.mark.parametrize("base", [0, 1_700_000_000_000], ids=["zero", "p1.7e12"])
@pytest.mark.parametrize("g", [1, 1000, 600_000])
def test_relative_table_edges(eng_mod, g, base):
    """Push 1 opens the slices q_base + {0, 31, 32, 4095, 4096, 5000}; pushes 2 and 3 put records at the first and the
    last ms of each. Relative slices 4096 and 5000 are past Phase P's table: only the v1 replay reaches them."""
    off = -(g // 3)
    q0 = R.slice_number(base, off, g)
    steps = []
    for p in range(3):
        k, ts, v = R.build_stream(base, off, g, N, seed_of("b", g, base, p), slices=TABLE_EDGES, edges_only=p > 0)
        assert {R.slice_number(t, off, g) - q0 for t in ts.tolist()} == set(TABLE_EDGES)
        steps.append((k, ts, [v], None, [A.LONG_MAX] if p == 2 else []))
    replay = []
    cfg = A.make_config(window_kind="TUMBLE", size_ms=g, offset_ms=off, aggs=[("COUNT", 0), ("SUM_I64", 0)], key_capacity=CAP)
    st, opt = drive(eng_mod, cfg, steps, after_push=lambda h, i: replay.append(h.stats().replay_records),
                    read=("fast_slice_pushes",), ctx="edges g=%d base=%d" % (g, base))
    assert st.partition_ms > 0 and st.combine_ms > 0 and st.late_dropped == 0
    assert replay[0] < replay[1] < replay[2], replay
    assert replay[2] - replay[1] > N // 6 - N // 20, replay     # about two of the six slices per push
    assert opt["fast_slice_pushes"] == sum(R.fast_form_expected(g, q, False, off) for q in (0, q0, q0))


# ---- (c) the other copies ------------------------------------------------------------------------------------------
C_SIZES = (7, 600_000, 1_048_577, 86_400_000)
C_BASES = {"zero": 0, "m1.7e12": -1_700_000_000_000, "p2^62": 1 << 62}
C_MATRIX = [pytest.param(g, b, id="%d-%s" % (g, n)) for g in C_SIZES for n, b in C_BASES.items()]
SLIDE_MATRIX = [pytest.param(s, sl, b, id="%d-%d-%s" % (s, sl, n)) for s, sl in R.SLIDES for n, b in C_BASES.items()]


@functools.lru_cache(maxsize=None)
def c_pool():
    return R.key_pool(KEYS_C, seed=7)


def c_streams(g, base, off, step=1, third=False, n=NC, tag="c"):
    """The (c) pushes, in units of `step` slices of size g (step = slide / g for sliding windows). Push 1: slices
    -3 .. 3 steps around the base, then three watermarks one step apart up to the base. Push 2: -6 .. 5 steps (the
    earliest are late, or inside the allowed lateness and fire late), three more watermarks. Push 3 (third): the same
    range again, every record of it at or below the watermark. Then the final watermark."""
    q0 = R.slice_number(base, off, g)
    wm = lambda j: R.slice_first_ms(q0 + j * step, off, g) - 1  # noqa: E731
    spans = [range(-3 * step, 3 * step + 1), range(-6 * step, 5 * step + 1)] + ([range(-6 * step, 2 * step + 1)] if third else [])
    out = []
    for p, sl in enumerate(spans):
        k, ts, v = R.build_stream(base, off, g, n, seed_of(tag, g, base, off, step, p), slices=sl, keys=c_pool())
        out.append((k, ts, v, [wm(j) for j in ((-2, -1, 0), (1, 2, 3), ())[p]]))
    out[-1][3].append(A.LONG_MAX)
    return out


def plain_steps(streams, ncols=1):
    return [(k, ts, [v] * ncols, None, wms) for k, ts, v, wms in streams]


@pytest.mark.parametrize("g,base", C_MATRIX)
def test_v1_ingest_rows_with_nulls(eng_mod, g, base):
    """Table TUMBLE over a nullable BIGINT column, one row in 20 NULL: rows with a NULL take ingest_kernel (v1)."""
    off = -(g // 3)
    steps = []
    for p, (k, ts, v, wms) in enumerate(c_streams(g, base, off, tag="v1")):
        nulls = (np.random.default_rng(seed_of("nulls", g, base, p)).random(len(k)) < 0.05).astype(np.uint8)
        steps.append((k, ts, [v], [nulls], wms))
    cfg = A.make_config(window_kind="TUMBLE", semantics="TABLE", size_ms=g, offset_ms=off, nullable_cols=(0,),
                        aggs=[("COUNT", 0), ("SUM_I64", 0), ("COUNT_COL", 0), ("MAX_I64", 0)], key_capacity=1024)
    st, _ = drive(eng_mod, cfg, steps, ctx="v1 g=%d base=%d" % (g, base))
    assert st.replay_records > NC // 40 and st.late_dropped > 0


def slide_cfg(kind, size, slide, off, **kw):
    wk, sem = {"ds_slide": ("SLIDE", "DATASTREAM"), "hop": ("SLIDE", "TABLE"), "cumulate": ("CUMULATE", "TABLE")}[kind]
    return A.make_config(window_kind=wk, semantics=sem, size_ms=size, slide_ms=slide, offset_ms=off, key_capacity=1024, **kw)


def table_slide_ok(kind, size, slide):
    return kind == "ds_slide" or size % slide == 0          # (the refused pair: REFUSED, test_documented_refusals)


@pytest.mark.parametrize("carried", [1, 0], ids=["carried", "recomputed"])
@pytest.mark.parametrize("size,slide,base", SLIDE_MATRIX)
@pytest.mark.parametrize("kind", ["ds_slide", "hop", "cumulate"])
def test_sliding_fires_one_slide_at_a_time(eng_mod, kind, size, slide, base, carried):
    g = R.slide_slice(size, slide)
    off = -(g // 3)
    if not table_slide_ok(kind, size, slide):
        with pytest.raises(eng_mod.EngineError) as ei:
            eng_mod.WindowAggregator(slide_cfg(kind, size, slide, off))
        assert ei.value.code == -1
        return
    cfg = slide_cfg(kind, size, slide, off, aggs=[("COUNT", 0), ("SUM_I64", 0), ("MIN_I64", 0)])
    steps = plain_steps(c_streams(g, base, off, step=slide // g, tag=kind))
    st, opt = drive(eng_mod, cfg, steps, options=dict(slide_carried=carried), read=("slide_carried",),
                    ctx="%s %d/%d base=%d" % (kind, size, slide, base))
    if not carried:
        assert opt["slide_carried"] == 0


@pytest.mark.parametrize("g,base", C_MATRIX)
def test_late_fire_tumble(eng_mod, g, base):
    """allowed_lateness_ms = 2 * g: push 2 and push 3 carry records of windows that already fired (late_fire_kernel) and
    of windows past their cleanup time (dropped; their indices are compared)."""
    off = -(g // 3)
    cfg = A.make_config(window_kind="TUMBLE", size_ms=g, offset_ms=off, allowed_lateness_ms=2 * g, late_indices=True,
                        aggs=[("COUNT", 0), ("SUM_I64", 0), ("MAX_I64", 0)], key_capacity=1024)
    st, _ = drive(eng_mod, cfg, plain_steps(c_streams(g, base, off, third=True, tag="late")), late_idx=True,
                  ctx="late tumble g=%d base=%d" % (g, base))
    assert st.late_dropped > 0


@pytest.mark.parametrize("size,slide,base", SLIDE_MATRIX)
def test_late_fire_slide(eng_mod, size, slide, base):
    g = R.slide_slice(size, slide)
    off = -(g // 3)
    cfg = slide_cfg("ds_slide", size, slide, off, allowed_lateness_ms=2 * g, late_indices=True,
                    aggs=[("COUNT", 0), ("SUM_I64", 0), ("MAX_I64", 0)])
    drive(eng_mod, cfg, plain_steps(c_streams(g, base, off, step=slide // g, third=True, tag="late_slide")), late_idx=True,
          ctx="late slide %d/%d base=%d" % (size, slide, base))


@pytest.mark.parametrize("lateness", [0, 2], ids=["on_time", "late"])
@pytest.mark.parametrize("op", ["sum", "max_by"])
@pytest.mark.parametrize("g,base", C_MATRIX)
def test_reductions(eng_mod, g, base, op, lateness):
    """WindowedStream.sum(1) / maxBy(1) over (key, Long, Long): integer fields, so every row is exact."""
    from flink_amd.operators import reduction_aggs
    off = -(g // 3)
    cfg = A.make_config(window_kind="TUMBLE", size_ms=g, offset_ms=off, allowed_lateness_ms=lateness * g, reduce=True,
                        aggs=reduction_aggs(op, 1, ("I64", "I64")), key_capacity=1024)
    steps = [(k, ts, [v, v ^ np.int64(0x5555)], None, wms)
             for k, ts, v, wms in c_streams(g, base, off, third=lateness > 0, tag="reduce")]
    drive(eng_mod, cfg, steps, ctx="%s g=%d base=%d lateness=%d" % (op, g, base, lateness))


@pytest.mark.parametrize("sem", ["DATASTREAM", "TABLE"])
@pytest.mark.parametrize("g,base", C_MATRIX)
def test_record_lists(eng_mod, g, base, sem):
    off = -(g // 3)
    kw = dict(window_kind="TUMBLE", semantics=sem, size_ms=g, offset_ms=off,
              aggs=[("COUNT", 0), ("SUM_I64", 0), ("MIN_I64", 0), ("MAX_I64", 0)])
    cfg = A.make_config(record_lists=True, **kw)
    g_ = eng_mod.WindowAggregator(cfg)
    assert g_.record_lists
    g_.close()
    drive(eng_mod, cfg, plain_steps(c_streams(g, base, off, tag="lists")), ocfg=A.make_config(**kw),
          ctx="record lists %s g=%d base=%d" % (sem, g, base))


@pytest.mark.parametrize("sem", ["DATASTREAM", "TABLE"])
@pytest.mark.parametrize("g,base", C_MATRIX)
def test_push_partials(eng_mod, g, base, sem):
    """A local handle's drained (key, slice) partials pushed into an owner: the owner's rows equal one operator's."""
    from oracle.oracle import Oracle
    off = -(g // 3)
    aggs = [("COUNT", 0), ("SUM_I64", 0)]
    cfg = A.make_config(window_kind="TUMBLE", semantics=sem, size_ms=g, offset_ms=off, aggs=aggs, key_capacity=1024)
    names = A.agg_names(cfg)
    local, owner, o = eng_mod.WindowAggregator(cfg), eng_mod.WindowAggregator(cfg), Oracle(cfg)
    try:
        late_l = late_o = 0
        for p, (k, ts, v, wms) in enumerate(c_streams(g, base, off, tag="partials")):
            late_l += local.push(k, ts, [v])
            late_o += o.push(k, ts, [v])
            for wm in wms:
                part = local.drain_partials(wm)
                for s in part["slice_start"].tolist():                        # slice timestamps on the slice grid
                    assert (s - off) % g == 0
                late_l += owner.push_partials(part["key"], part["slice_start"], part["count"],
                                              [part["acc%d" % j] for j in range(len(aggs))])
                assert_rows_equal(owner.advance_watermark(wm), o.advance_watermark(wm), names,
                                  ctx="partials %s g=%d base=%d push %d wm %d" % (sem, g, base, p, wm))
        assert late_l == late_o and o.stats().rows_out > 0
    finally:
        for h in (local, owner, o):
            h.close()


@pytest.mark.parametrize("g,base", C_MATRIX)
def test_drain_route_into_fire_partials(eng_mod, g, base):
    """fwa_drain_route for 3 destinations, each destination's rows fired by the handle owning its key groups."""
    import torch
    from flink_amd import keygroups as KG
    from oracle.oracle import Oracle
    off = -(g // 3)
    kw = dict(window_kind="TUMBLE", size_ms=g, offset_ms=off, aggs=[("COUNT", 0), ("SUM_I64", 0)], key_capacity=1024)
    names = A.agg_names(A.make_config(**kw))
    local = eng_mod.WindowAggregator(A.make_config(output_on_device=1, **kw))
    owners = []
    for d in range(3):
        lo, hi = KG.key_group_range_for_operator(128, 3, d)
        owners.append(eng_mod.WindowAggregator(A.make_config(kg_start=lo, kg_end=hi, **kw)))
    o = Oracle(A.make_config(**kw))
    try:
        late_l = late_o = 0
        for p, (k, ts, v, wms) in enumerate(c_streams(g, base, off, tag="route")):
            late_l += local.push(torch.from_numpy(k).cuda(), torch.from_numpy(ts).cuda(), [torch.from_numpy(v).cuda()])
            late_o += o.push(k, ts, [v])
            for wm in wms:
                parts, counts, m = local.drain_route(wm, 3)
                assert m == 4
                parts = [x.clone() for x in parts]                            # views die with the next call
                fired = [own.fire_partials(parts[d], [2, 3], wm) for d, own in enumerate(owners)]
                got = {f: np.concatenate([r[f] for r in fired]) for f in fired[0]}
                assert_rows_equal(got, o.advance_watermark(wm), names, ctx="route g=%d base=%d push %d wm %d" % (g, base, p, wm))
        assert late_l + sum(own.stats().late_dropped for own in owners) == late_o
        assert sum(own.get_option("fire_partials") for own in owners) > 0, "no call merged and fired on chip"
    finally:
        for h in [local, o] + owners:
            h.close()


DISTINCT_AGGS = [("COUNT", 0), ("COUNT_DISTINCT", 0)]


def drive_distinct(eng_mod, kw, steps, ctx):
    """A handle with [COUNT, COUNT_DISTINCT(col 0)] against the oracle's rows of [COUNT, COUNT] over the same stream,
    whose second column is replaced by a brute-force count in Python integers: the different values among the accepted
    records of the row's key with a timestamp in [win_start, win_end). (The oracle has no distinct aggregate.)"""
    from oracle.oracle import Oracle
    names = ["COUNT", "COUNT"]
    g = eng_mod.WindowAggregator(A.make_config(aggs=DISTINCT_AGGS, **kw))
    o = Oracle(A.make_config(aggs=[("COUNT", 0), ("COUNT", 0)], late_indices=True, **kw))
    accepted = {}
    try:
        for i, (k, ts, cols, _, wms) in enumerate(steps):
            dg, do = g.push(k, ts, cols), o.push(k, ts, cols)
            assert dg == do, "%s push %d: dropped %d, the oracle %d" % (ctx, i, dg, do)
            late = set(o.late_records().tolist())
            assert len(late) == do
            for j, (key, t, v) in enumerate(zip(k.tolist(), ts.tolist(), cols[0].tolist())):
                if j not in late:
                    accepted.setdefault(key, []).append((t, v))
            for wm in wms:
                ro = o.advance_watermark(wm)
                want = [len({v for t, v in accepted[key] if s <= t < e})
                        for key, s, e in zip(ro["key"].tolist(), ro["win_start"].tolist(), ro["win_end"].tolist())]
                assert ro["agg0"].tolist() == [sum(1 for t, _ in accepted[key] if s <= t < e) for key, s, e in
                                               zip(ro["key"].tolist(), ro["win_start"].tolist(), ro["win_end"].tolist())]
                ro["agg1"] = np.array(want, dtype=np.int64)
                assert_rows_equal(g.advance_watermark(wm), ro, names, ctx="%s push %d wm %d" % (ctx, i, wm))
        assert o.stats().rows_out > 0 and o.stats().late_dropped > 0, ctx
    finally:
        g.close()
        o.close()


@pytest.mark.parametrize("g,base", C_MATRIX)
def test_count_distinct_tumble(eng_mod, g, base):
    """COUNT(DISTINCT) on Table TUMBLE: the set is keyed by the host's slice numbers (size 7: REFUSED)."""
    off = -(g // 3)
    kw = dict(window_kind="TUMBLE", semantics="TABLE", size_ms=g, offset_ms=off, key_capacity=1024)
    if g < 64:
        with pytest.raises(eng_mod.EngineError) as ei:
            eng_mod.WindowAggregator(A.make_config(aggs=DISTINCT_AGGS, **kw))
        assert ei.value.code == -7 and "DISTINCT" in str(ei.value)
        return
    steps = [(k, ts, [v % 5], None, wms) for k, ts, v, wms in c_streams(g, base, off, tag="distinct")]
    drive_distinct(eng_mod, kw, steps, ctx="distinct g=%d base=%d" % (g, base))


@pytest.mark.parametrize("size,slide", [(3_600_000, 600_000), (21, 7)])
@pytest.mark.parametrize("bname", list(C_BASES))
def test_count_distinct_range_hop(eng_mod, size, slide, bname):
    """FWA_CFG_DISTINCT_RANGE on Table HOP (the (600 000, 420 000) pair is no Table HOP: REFUSED)."""
    base, g = C_BASES[bname], R.slide_slice(size, slide)
    off = -(g // 3)
    kw = dict(window_kind="SLIDE", semantics="TABLE", size_ms=size, slide_ms=slide, offset_ms=off, key_capacity=1024,
              distinct_range=True)
    steps = [(k, ts, [v % 5], None, wms) for k, ts, v, wms in c_streams(g, base, off, step=slide // g, tag="range")]
    drive_distinct(eng_mod, kw, steps, ctx="distinct range %d/%d base=%d" % (size, slide, base))


@pytest.mark.parametrize("sem", ["DATASTREAM", "TABLE"])
@pytest.mark.parametrize("g,base", C_MATRIX)
def test_f32_fold(eng_mod, g, base, sem):
    """FWA_CFG_F32_FOLD: values are small integers, so the float32 fold is exact in any order and equals the oracle's
    sum bit for bit."""
    off = -(g // 3)
    kw = dict(window_kind="TUMBLE", semantics=sem, size_ms=g, offset_ms=off, aggs=[("COUNT", 0), ("SUM_F32", 0)], key_capacity=1024)
    steps = [(k, ts, [(v % 17 - 8).astype(np.float32)], None, wms) for k, ts, v, wms in c_streams(g, base, off, tag="fold")]
    drive(eng_mod, A.make_config(f32_fold=True, **kw), steps, ocfg=A.make_config(**kw), read=("f32_fold_slots",),
          ctx="fold %s g=%d base=%d" % (sem, g, base))


# ---- sessions: the cell number floor((ts - first ts of the push) / gap) ---------------------------------------------
SESSION_GAPS = (7, 600_000, 1_048_577)
SESSION_AGGS = [("COUNT", 0), ("SUM_I64", 0), ("MIN_I64", 0), ("MAX_I64", 0)]
# route: (records, keys, pushes, cells per push, options, ingest_variant, path every push must take) -- the record
# counts at which tests/test_sessions_gpu.py asserts the routes
SESSION_ROUTES = {
    "general": (6000, 500, 3, 10, dict(session_cells=0), 0, 0),
    "sorted_cells": (60_000, 500, 2, 50, None, 0, 1),
    "preagg_s5_hash": (50_000, 3000, 3, 11, None, 0, 2),
    "preagg_s4_probe": (50_000, 3000, 3, 11, None, 8, 2),
}


def session_steps(base, gap, n, nkeys, pushes, cells, seed):
    """An in-order stream from `base` on, `cells` gaps of event time per push; every push also holds chains of six
    records exactly one gap apart (windows that touch, so they merge across cell borders into one session)."""
    rng = np.random.default_rng(seed)
    span = cells * gap
    steps = []
    for p in range(pushes):
        lo = base + p * span
        m = n // pushes
        t = [lo + d for d in np.sort(rng.integers(0, span, m)).tolist()]
        k = rng.integers(0, nkeys, m).tolist()
        for c in range(40):                                               # chain keys are no one else's
            t0 = lo + int(rng.integers(0, max(1, span - 6 * gap)))
            t += [t0 + i * gap for i in range(6)]
            k += [100_000 + c] * 6
        order = sorted(range(len(t)), key=t.__getitem__)
        ts = np.array([t[i] for i in order], dtype=np.int64)
        keys = np.array([k[i] for i in order], dtype=np.int64)
        v = rng.integers(-(1 << 40), 1 << 40, len(ts)).astype(np.int64)
        wm = int(ts.max()) - 1 if p < pushes - 1 else A.LONG_MAX
        steps.append((keys, ts, [v], None, [wm]))
    return steps


@pytest.mark.parametrize("sem", ["DATASTREAM", "TABLE"])
@pytest.mark.parametrize("bname", list(C_BASES))
@pytest.mark.parametrize("gap", SESSION_GAPS)
@pytest.mark.parametrize("route", list(SESSION_ROUTES))
def test_session_cells(eng_mod, route, gap, bname, sem):
    n, nkeys, pushes, cells, options, variant, want_path = SESSION_ROUTES[route]
    base = C_BASES[bname] - pushes * cells * gap // 2                   # "zero": the pushes straddle 0
    if options is not None or variant:
        options = dict(options or {}, **({"ingest_variant": variant} if variant else {}))
    cfg = A.make_config(window_kind="SESSION", semantics=sem, gap_ms=gap, aggs=SESSION_AGGS, key_capacity=8192)
    paths = []
    st, _ = drive(eng_mod, cfg, session_steps(base, gap, n, nkeys, pushes, cells, seed_of("sess", route, gap, base)),
                  options=options, after_push=lambda h, i: paths.append(h.get_option("session_path")),
                  ctx="sessions %s gap=%d base=%d %s" % (route, gap, base, sem))
    assert paths == [want_path] * pushes, paths
    assert st.late_dropped == 0
    if want_path:
        assert st.replay_records == 0


# ---- snapshot / restore ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["tumble", "hop"])
def test_snapshot_restore_at_a_negative_epoch(eng_mod, kind):
    """Size 600 000 at base -1.7e12, Table TUMBLE and HOP: the blob taken after push 1 restored into a fresh handle; the
    rows afterwards equal the oracle's uninterrupted run (restore re-derives every slice number on the host)."""
    from oracle.oracle import Oracle
    g, base = 600_000, -1_700_000_000_000
    off = -(g // 3)
    aggs = [("COUNT", 0), ("SUM_I64", 0), ("MAX_I64", 0)]
    if kind == "tumble":
        cfg = A.make_config(window_kind="TUMBLE", semantics="TABLE", size_ms=g, offset_ms=off, aggs=aggs, key_capacity=1024)
        step = 1
    else:
        cfg = slide_cfg("hop", 6 * g, g, off, aggs=aggs)
        step = 1
    names = A.agg_names(cfg)
    h, o = eng_mod.WindowAggregator(cfg), Oracle(cfg)
    try:
        for p, (k, ts, v, wms) in enumerate(c_streams(g, base, off, step=step, tag="snap")):
            assert h.push(k, ts, [v]) == o.push(k, ts, [v])
            if p == 0:
                blob = h.snapshot()
                h.close()
                h = eng_mod.WindowAggregator(cfg)
                h.restore(blob)
            for wm in wms:
                assert_rows_equal(h.advance_watermark(wm), o.advance_watermark(wm), names, ctx="snapshot %s push %d wm %d" % (kind, p, wm))
        assert h.stats().rows_out > 0 and o.stats().late_dropped > 0
    finally:
        h.close()
        o.close()
