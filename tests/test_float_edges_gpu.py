"""SUM / AVG / MIN / MAX over FLOAT and DOUBLE on non-reduce handles against the exact per-row reference of
tests/float_ref.py, on every path that carries float accumulators: the one-pass ingest with the three TUMBLE fires,
the two-phase ingest in each value-width shape (FLOAT then DOUBLE and two FLOAT columns among them), the combiner's
stragglers, record lists, sessions on each of their paths, partial accumulators and snapshots.

Every case runs the `finite` stream (ill-conditioned sums, subnormals, FLOAT sums past FLT_MAX, both zeros) and the
`special` stream (NaNs of either sign and with a payload, infinities, zeros in both orders; exact sums) and compares
every row after every watermark: sums inside [S-B, S+B] pushed through the engine's own final operations, MIN / MAX bit
for bit under the engine's bit order and admissible for the reference's fold. Late indices and late_dropped equal the
oracle's. Each case asserts the indicator of the path it is about."""
import numpy as np
import pytest

import float_ref as F
from flink_amd import _abi as A

pytestmark = pytest.mark.gpu

STREAMS = ["finite", "special"]
# value columns: 0 DOUBLE, 1 FLOAT, 2 DOUBLE, 3 FLOAT
ONE_PASS = {      # three or four distinct value columns: not eligible for the two-phase ingest; 5 accumulator columns
    "a": [("COUNT", 0), ("SUM_F64", 0), ("MIN_F32", 1), ("MAX_F64", 2), ("AVG_F32", 3)],
    "b": [("COUNT", 0), ("AVG_F64", 2), ("SUM_F32", 1), ("MAX_F32", 3), ("MIN_F64", 0)],
}
TWO_PHASE = {     # by the byte widths of the carried value columns
    "float": [("COUNT", 0), ("SUM_F32", 1), ("AVG_F32", 1), ("MIN_F32", 1), ("MAX_F32", 1)],
    "double": [("COUNT", 0), ("SUM_F64", 0), ("AVG_F64", 0), ("MIN_F64", 0), ("MAX_F64", 0)],
    "float_float": [("COUNT", 0), ("SUM_F32", 1), ("MIN_F32", 1), ("MAX_F32", 1), ("AVG_F32", 3), ("MIN_F32", 3),
                    ("MAX_F32", 3)],
    "double_float": [("COUNT", 0), ("SUM_F64", 0), ("MIN_F64", 0), ("MAX_F64", 0), ("AVG_F32", 1), ("MIN_F32", 1),
                     ("MAX_F32", 1)],
    "float_double": [("COUNT", 0), ("SUM_F32", 1), ("MIN_F32", 1), ("MAX_F32", 1), ("AVG_F64", 0), ("MIN_F64", 0),
                     ("MAX_F64", 0)],
    "double_double": [("COUNT", 0), ("SUM_F64", 0), ("MIN_F64", 0), ("MAX_F64", 0), ("AVG_F64", 2), ("MIN_F64", 2),
                      ("MAX_F64", 2)],
}
SESSION_AGGS = [("COUNT", 0), ("SUM_F64", 0), ("AVG_F64", 0), ("MIN_F32", 1), ("MAX_F64", 2)]
LIST_AGGS = [("COUNT", 0), ("SUM_F64", 0), ("AVG_F64", 2), ("MIN_F64", 0), ("MAX_F64", 2), ("SUM_F32", 1),
             ("MIN_F32", 3), ("MAX_F32", 1)]


@pytest.fixture(scope="module")
def eng_mod():
    from flink_amd import engine
    engine.lib()
    return engine


def handle(eng_mod, kw, aggs, options=None, **more):
    return eng_mod.WindowAggregator(A.make_config(aggs=aggs, late_indices=True, **dict(kw, **more)), options=options)


def finish(g, ref, rows):
    st = g.stats()
    assert rows == ref.n_rows                                  # every row was compared
    assert st.late_dropped == ref.n_late
    g.close()
    return st


# ---- one-pass ingest ----
@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("aggs", list(ONE_PASS))
@pytest.mark.parametrize("kind,variant", [("tumble", 0), ("tumble", 256), ("tumble", 256 | 32), ("hop", 0),
                                          ("cumulate", 0)])
def test_one_pass_ingest(eng_mod, kind, variant, aggs, stream):
    """TUMBLE fires: the walk over a watermark's windows (default), the multi-column fire (FWA_OPT_INGEST_VARIANT bit 8
    switches the walk off) and the generic one (bit 5 switches the multi-column fire off too)."""
    kw, ref = F.case(stream, kind)
    g = handle(eng_mod, kw, ONE_PASS[aggs], options={"ingest_variant": variant})
    rows = F.run_engine(g, ref, ONE_PASS[aggs], ctx="%s %s variant %d" % (stream, kind, variant))
    assert g.get_option("ingest_variant") == variant
    st = finish(g, ref, rows)
    assert st.partition_ms == 0                                # the one-pass ingest took every push


# ---- two-phase ingest ----
def two_phase(eng_mod, stream, kind, shape, options, device=False, **more):
    kw, ref = F.case(stream, kind)
    aggs = TWO_PHASE[shape]
    g = handle(eng_mod, kw, aggs, options=options, **more)
    rows = F.run_engine(g, ref, aggs, device=device, ctx="%s %s %s %s" % (stream, kind, shape, options))
    for name, value in options.items():
        assert g.get_option(name) == value, name
    st = finish(g, ref, rows)
    assert st.partition_ms > 0, "the two-phase ingest did not run"
    assert st.replay_records < len(ref.keys) // 8, st.replay_records
    return st


SHAPES = [(s, {}) for s in TWO_PHASE if s != "double_float"] + \
    [("double_float", {"narrow_entries": 0}), ("double_float", {"narrow_entries": 1})]


@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("passes", [0, 1])
@pytest.mark.parametrize("shape,options", SHAPES, ids=["%s%s" % (s, "".join("-%s%d" % kv for kv in o.items()))
                                                        for s, o in SHAPES])
def test_two_phase_ingest_hop(eng_mod, shape, options, passes, stream):
    """Every value-width shape of partition3 / combine3 on a HOP handle, without and with the combiner's window passes."""
    two_phase(eng_mod, stream, "hop", shape, dict(options, window_passes=passes))


@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("kind", ["tumble", "cumulate"])
@pytest.mark.parametrize("shape", ["float_double", "float_float"])
def test_two_phase_ingest_float_first(eng_mod, shape, kind, stream):
    two_phase(eng_mod, stream, kind, shape, {})


@pytest.mark.parametrize("stream", STREAMS)
def test_two_phase_ingest_device_inputs_and_outputs(eng_mod, stream):
    two_phase(eng_mod, stream, "hop", "float_double", {}, device=True, output_on_device=1)


@pytest.mark.parametrize("shape", ["double_float", "float_double"])
def test_stragglers_with_float_entries(eng_mod, shape):
    """One push over 6 slices in event-time order whose last third returns to the first slice: every combiner block has
    slid its window past that slice by then, so those entries go to the slots through strag_apply (carried_f64 /
    carried_ord), more than the 256 a block lists in LDS. A key table of 2^13 slots has at most 2^13 / 2^9 = 16
    combiner blocks (segments hold at least 512 keys)."""
    kw, ref = F.straggler_case()
    aggs = TWO_PHASE[shape]
    g = handle(eng_mod, kw, aggs)
    rows = F.run_engine(g, ref, aggs, ctx="stragglers %s" % shape)
    stragglers = g.get_option("stragglers")
    st = finish(g, ref, rows)
    assert st.partition_ms > 0 and st.replay_records < len(ref.keys) // 8
    assert stragglers > 256 * 16, stragglers


# ---- record lists ----
@pytest.mark.parametrize("stream", STREAMS)
def test_record_lists(eng_mod, stream):
    kw, ref = F.case(stream, "tumble")
    g = handle(eng_mod, kw, LIST_AGGS, record_lists=True)
    assert g.record_lists
    rows = F.run_engine(g, ref, LIST_AGGS, ctx="%s record lists" % stream)
    finish(g, ref, rows)


# ---- sessions ----
@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("kind,cells,path", [("session1000", 0, 0), ("session150", -1, 1), ("session1000", -1, 2)],
                         ids=["general", "sorted_cells", "cell_preaggregation"])
def test_sessions(eng_mod, kind, cells, path, stream):
    """DataStream gap sessions on each FWA_OPT_SESSION_PATH: 0 the general path (cells switched off), 1 the sort-based
    cell path (a push spans more than 16 cells of 150 ms), 2 the cell pre-aggregation (at most 16 cells of 1 s)."""
    kw, ref = F.case(stream, kind)
    g = handle(eng_mod, kw, SESSION_AGGS, options={"session_cells": cells})
    paths = []
    rows = F.run_engine(g, ref, SESSION_AGGS, ctx="%s %s" % (stream, kind),
                        after_push=lambda h: paths.append(h.get_option("session_path")))
    finish(g, ref, rows)
    assert paths == [path] * 4, paths


# ---- partial accumulators ----
@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("kind", ["tumble", "hop"])
def test_drain_partials_into_push_partials(eng_mod, kind, stream):
    """A local handle drains (key, slice) accumulators -- double bits and ordered MIN / MAX keys -- and the owner merges
    them and fires: the rows of one operator."""
    kw, ref = F.case(stream, kind)
    aggs = ONE_PASS["a"]
    loc, own = handle(eng_mod, kw, aggs), handle(eng_mod, kw, aggs)
    rows = 0
    for b, (keys, ts, cols, wm) in enumerate(ref.batches):
        if len(keys):
            assert loc.push(keys, ts, cols) == len(ref.late[b])
            assert np.array_equal(loc.late_records(), ref.late[b])
        if wm is None:
            continue
        p = loc.drain_partials(wm)
        if len(p["key"]):
            assert own.push_partials(p["key"], p["slice_start"], p["count"], [p["acc%d" % j] for j in range(len(aggs))]) == 0
        rows += F.compare_rows(own.advance_watermark(wm), ref, b, aggs, ctx="%s %s partials" % (stream, kind))
    assert rows == ref.n_rows and loc.stats().late_dropped == ref.n_late
    st = own.stats()
    assert st.late_dropped == 0 and st.partition_ms == 0       # float lists merge on the one-pass path
    loc.close()
    own.close()


@pytest.mark.parametrize("stream", STREAMS)
def test_drain_route_into_fire_partials(eng_mod, stream):
    """fwa_drain_route's packed rows into the owner's on-chip merge + fire (the plumbing of test_fire_partials_gpu.py)."""
    import torch
    kw, ref = F.case(stream, "tumble")
    aggs = ONE_PASS["b"]
    names = [a[0] for a in aggs]
    ship = [j for j, nm in enumerate(names) if nm != "COUNT"]
    cells = [2 if nm == "COUNT" else 3 + ship.index(j) for j, nm in enumerate(names)]
    loc, own = handle(eng_mod, kw, aggs, output_on_device=1), handle(eng_mod, kw, aggs)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    rows = steps = 0
    for b, (keys, ts, cols, wm) in enumerate(ref.batches):
        if len(keys):
            assert loc.push(dev(keys), dev(ts), [dev(c) for c in cols]) == len(ref.late[b])
        if wm is None:
            continue
        parts, counts, m = loc.drain_route(wm, 1)
        assert m == 3 + len(ship)
        rows += F.compare_rows(own.fire_partials(parts[0], cells, wm), ref, b, aggs, ctx="%s fire_partials" % stream)
        steps += 1
    assert rows == ref.n_rows and loc.stats().late_dropped == ref.n_late
    assert own.get_option("fire_partials") == steps            # every step merged and fired on chip
    loc.close()
    own.close()


# ---- snapshot / restore ----
@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("kind,aggs", [("hop", TWO_PHASE["float_double"]), ("tumble", ONE_PASS["a"]),
                                       ("session1000", SESSION_AGGS)], ids=["hop_two_phase", "tumble_one_pass", "session"])
def test_snapshot_mid_stream(eng_mod, kind, aggs, stream):
    """snapshot() behind the second watermark (live slices hold special accumulators), restore() into a fresh handle,
    on to end of input."""
    kw, ref = F.case(stream, kind)
    cut = len(ref.batches) - 3
    g = handle(eng_mod, kw, aggs)
    rows = F.run_engine(g, ref, aggs, last=cut, ctx="%s %s before the snapshot" % (stream, kind))
    blob = g.snapshot()
    g.close()
    h = handle(eng_mod, kw, aggs)
    h.restore(blob)
    rows += F.run_engine(h, ref, aggs, first=cut, ctx="%s %s restored" % (stream, kind))
    st = h.stats()
    assert rows == ref.n_rows                                   # (run_engine compared the late indices of every push)
    if aggs is TWO_PHASE["float_double"]:
        assert st.partition_ms > 0                              # the restored handle went on with the two-phase ingest
    else:
        assert st.partition_ms == 0
    h.close()
