"""The float32 arrival-order fold (FWA_CFG_F32_FOLD), CPU side: what "the reference" means and why a GPU test that
passes cannot be passing with the engine's f64 sum.

The oracle folds x->f = x->f + v per record in arrival order from 0.0f (oracle/fwa_oracle.c), the rule of
SumAggFunction's FLOAT buffer and of SumAggregator.reduce on a Float field. fold_model (f32_fold_ref.py) is the same rule
in ten lines of numpy; here it must equal the oracle's SUM_F32 bit for bit on the streams the GPU tests use, dropped
late records and NULL inputs included. On those streams a large share of the rows must differ from
float32(float64 sum of the same records), which is what the engine returns without the flag."""
import numpy as np
import pytest

from f32_fold_ref import SIZE, f32_bits, fold_model, make_stream
from flink_amd import _abi as A

STREAMS = {
    "datastream": (dict(semantics="DATASTREAM"), dict(seed=7)),
    "table_offset": (dict(semantics="TABLE", offset_ms=250), dict(seed=8)),
    "table_nulls": (dict(semantics="TABLE", nullable_cols=(1,)), dict(seed=9, null_frac=0.1)),
}


def _oracle_rows(cfg_kw, batches):
    from oracle.oracle import Oracle
    cfg = A.make_config(window_kind="TUMBLE", size_ms=SIZE, aggs=[("COUNT", 0), ("SUM_F32", 1)], **cfg_kw)
    o = Oracle(cfg)
    rows, dropped = {}, 0
    for (k, t, cols, nulls, wm) in list(batches) + [(None, None, None, None, A.LONG_MAX)]:
        if k is not None:
            dropped += o.push(k, t, cols, nulls=nulls)
        r = o.advance_watermark(wm)
        for i in range(len(r["key"])):
            nul = "null1" in r and bool(r["null1"][i])
            rows[(int(r["key"][i]), int(r["win_start"][i]))] = None if nul else r["agg1"][i]
    o.close()
    return rows, dropped


@pytest.mark.parametrize("name", sorted(STREAMS))
def test_numpy_model_equals_the_oracle_bit_for_bit(name):
    cfg_kw, stream_kw = STREAMS[name]
    batches = make_stream(**stream_kw)
    model, dropped = fold_model(batches, offset=cfg_kw.get("offset_ms", 0))
    rows, odropped = _oracle_rows(cfg_kw, batches)
    assert dropped == odropped and dropped > 100
    assert set(rows) == set(model) and len(rows) > 700
    for g, got in rows.items():
        exp = model[g][0]
        if cfg_kw["semantics"] == "TABLE" and exp is None:
            assert got is None, g                          # no non-NULL input: SQL NULL
            continue
        assert got is not None and f32_bits(got) == f32_bits(np.float32(0.0) if exp is None else exp), (g, got, exp)


@pytest.mark.parametrize("name", sorted(STREAMS))
def test_streams_tell_the_fold_from_an_f64_sum(name):
    """At least 25 % of the fired rows have a fold whose bits differ from float32(float64 sum of the same records)."""
    cfg_kw, stream_kw = STREAMS[name]
    model, _ = fold_model(make_stream(**stream_kw), offset=cfg_kw.get("offset_ms", 0))
    rows = [(acc, v) for acc, v in model.values() if acc is not None]
    differ = sum(f32_bits(acc) != f32_bits(np.float32(np.sum(np.asarray(v, np.float64)))) for acc, v in rows)
    assert len(rows) > 700 and differ >= 0.25 * len(rows), (differ, len(rows))


def test_make_config_sets_the_flag():
    assert A.CFG_F32_FOLD == 0x80
    assert A.make_config(f32_fold=True).flags & 0x80
    assert not A.make_config().flags & 0x80
    assert A.make_config(f32_fold=True, reduce=True).flags == 0x88


def test_facades_pass_the_flag_through():
    from flink_amd.assigners import TumblingEventTimeWindows
    from flink_amd.operators import ReduceWindowOperator, WindowOperator
    made = []

    class Fake:
        def __init__(self, cfg):
            made.append(cfg.flags)

        def close(self):
            pass

    WindowOperator(TumblingEventTimeWindows.of(1000), [("SUM_F32", 0)], engine_factory=Fake, f32_fold=True)
    WindowOperator(TumblingEventTimeWindows.of(1000), [("SUM_F32", 0)], engine_factory=Fake)
    ReduceWindowOperator(TumblingEventTimeWindows.of(1000), "sum", 1, ("F32", "I64"), engine_factory=Fake, f32_fold=True)
    assert made == [0x80, 0, 0x88]
