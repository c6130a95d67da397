"""Engine snapshot / restore of COUNT(DISTINCT) handles: the blob carries the live entries of the distinct set, so a
restored handle (same or rescaled key-group ranges) does not count values from before the checkpoint again; blobs of
handles without the aggregate keep their bytes."""
import importlib.util
import os

import numpy as np
import pytest

from distinct_ref import FirstOccurrence, reference_aggs
from flink_amd import _abi as A
from helpers import GOLDEN, assert_rows_equal

pytestmark = pytest.mark.gpu

TABLE = dict(window_kind="TUMBLE", semantics="TABLE", size_ms=1000)
AGGS = [("COUNT", 0), ("SUM_I64", 0), ("COUNT_DISTINCT", 1)]
PLAIN_BLOB = os.path.join(GOLDEN, "snapshot_table_tumble_count_sum.bin")


@pytest.fixture(scope="module")
def eng_mod():
    from flink_amd import engine
    engine.lib()
    return engine


def _plain_blob(eng_mod):
    """tests/golden/gen_snapshot_plain_blob.py: the stream, and how the committed file was written."""
    spec = importlib.util.spec_from_file_location("gen_snapshot_plain_blob", os.path.join(GOLDEN, "gen_snapshot_plain_blob.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.OUT == PLAIN_BLOB
    return m.plain_blob(eng_mod)


def test_dense_blob_without_the_aggregate_is_byte_identical(eng_mod):
    """Against the blob commit ef1fe48, the last build without the aggregate, wrote (dense layout; generator and command
    in tests/golden/gen_snapshot_plain_blob.py), committed once as a golden file."""
    with open(PLAIN_BLOB, "rb") as f:
        want = f.read()
    got = _plain_blob(eng_mod)
    assert got == want
    from flink_amd import snapshot as S
    assert "distinct" not in S.parse(got)


def _stream():
    rng = np.random.default_rng(21)
    n = 20_000
    keys = rng.integers(0, 200, n).astype(np.int64)
    ts = np.sort(rng.integers(0, 10_000, n)).astype(np.int64) - rng.integers(0, 2500, n)
    cols = [rng.integers(-50, 50, n).astype(np.int64), rng.integers(0, 30, n).astype(np.int64)]
    nulls = [None, (rng.random(n) < 0.1).astype(np.uint8)]
    return keys, ts, cols, nulls


def test_snapshot_restore_with_rescale(eng_mod):
    from flink_amd import snapshot as S
    from oracle.oracle import Oracle
    keys, ts, cols, nulls = _stream()
    n, cut = len(keys), len(keys) // 2
    wm1 = int(ts[:cut].max()) - 400                      # inside a window: its values repeat after the checkpoint
    assert (wm1 + 1) % 1000 != 0
    raggs, dcols = reference_aggs(AGGS, 2)
    names = [a[0] for a in raggs]
    kw = dict(TABLE, key_capacity=1024, nullable_cols=(1,))
    first = FirstOccurrence(1000)
    mark = first.mark(keys, ts, cols[1], nulls[1])
    o = Oracle(A.make_config(aggs=raggs, **kw))
    o.push(keys[:cut], ts[:cut], [c[:cut] for c in cols] + [mark[:cut]], nulls=[None, nulls[1][:cut], None])
    ref1 = o.advance_watermark(wm1)
    late2 = o.push(keys[cut:], ts[cut:], [c[cut:] for c in cols] + [mark[cut:]], nulls=[None, nulls[1][cut:], None])
    ref2 = o.advance_watermark(A.LONG_MAX)
    o.close()
    assert len(ref1["key"]) > 0 and len(ref2["key"]) > 0 and late2 > 0

    g = eng_mod.WindowAggregator(A.make_config(aggs=AGGS, **kw))
    g.push(keys[:cut], ts[:cut], [c[:cut] for c in cols], nulls=[None, nulls[1][:cut]])
    assert_rows_equal(g.advance_watermark(wm1), ref1, names)
    blob = g.snapshot()
    g.close()
    snap = S.parse(blob)
    d = snap["distinct"]
    assert d["agg_mask"] == 4 and d["n"] > 0 and snap["watermark"] == wm1
    assert (d["slice_start"] + 1000 - 1 > wm1).all() and (d["column"] == 0).all()
    assert int(d["kg_offsets"][-1]) == d["n"] and (np.diff(d["kg_offsets"]) >= 0).all()

    kgs, _ = eng_mod.key_groups(keys, 128, 1, A.KEY_JAVA_LONG)
    for layout in ([(0, 127)], [(0, 63), (64, 127)]):
        outs, late = [], 0
        for lo, hi in layout:
            h = eng_mod.WindowAggregator(A.make_config(aggs=AGGS, kg_start=lo, kg_end=hi, **kw))
            h.restore(blob)
            m = (kgs[cut:] >= lo) & (kgs[cut:] <= hi)
            late += h.push(keys[cut:][m], ts[cut:][m], [c[cut:][m] for c in cols], nulls=[None, nulls[1][cut:][m]])
            outs.append(h.advance_watermark(A.LONG_MAX))
            h.close()
        assert late == late2
        assert_rows_equal({f: np.concatenate([r[f] for r in outs]) for f in outs[0]}, ref2, names)


def test_blobs_of_other_aggregate_lists_are_refused(eng_mod):
    k = np.arange(4, dtype=np.int64)
    plain = eng_mod.WindowAggregator(A.make_config(aggs=[("COUNT", 0), ("SUM_I64", 0)], **TABLE))
    dist = eng_mod.WindowAggregator(A.make_config(aggs=[("COUNT", 0), ("COUNT_DISTINCT", 0)], **TABLE))
    for g in (plain, dist):
        g.push(k, k, [k])
    bp, bd = plain.snapshot(), dist.snapshot()
    plain.close()
    dist.close()
    for aggs, blob in (([("COUNT", 0), ("COUNT_DISTINCT", 0)], bp), ([("COUNT", 0), ("SUM_I64", 0)], bd)):
        h = eng_mod.WindowAggregator(A.make_config(aggs=aggs, **TABLE))
        with pytest.raises(eng_mod.EngineError) as ei:
            h.restore(blob)
        assert ei.value.code == -1
        h.close()
    h = eng_mod.WindowAggregator(A.make_config(aggs=[("COUNT", 0), ("COUNT_DISTINCT", 0)], **TABLE))
    h.restore(bd)                                         # ... and its own kind is accepted
    r = h.advance_watermark(A.LONG_MAX)
    assert sorted(zip(r["key"].tolist(), r["agg1"].tolist())) == [(0, 1), (1, 1), (2, 1), (3, 1)]
    h.close()
