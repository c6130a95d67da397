"""The exact float reference (tests/float_ref.py) on the CPU alone: its streams hold what they are meant to hold (the
non-vacuity counts), its intervals are well formed, and the oracle -- one legal arrival order of the reference's folds
-- lies inside them: the double sums in [S-B, S+B], MIN / MAX in the admissible set of every row and equal to the
bit-order extreme wherever the multiset has neither a NaN nor both zeros."""
import numpy as np
import pytest

import float_ref as F
from flink_amd import _abi as A

ORACLE_AGGS = [("COUNT", 0), ("SUM_F64", 0), ("AVG_F64", 0), ("MIN_F64", 0), ("MAX_F64", 0), ("SUM_F32", 1),
               ("MIN_F32", 1), ("MAX_F32", 1)]
ALL_KINDS = list(F.KINDS)
TINY64, TINY32 = 2.0 ** -1022, 2.0 ** -126


def oracle_rows(kw, ref):
    """The oracle with the float aggregates over the reference's stream: its rows per batch."""
    from oracle.oracle import Oracle
    o = Oracle(A.make_config(aggs=ORACLE_AGGS, late_indices=True, **kw))
    out = []
    for keys, ts, cols, wm in ref.batches:
        if len(keys):
            o.push(keys, ts, cols)
        out.append(None if wm is None else o.advance_watermark(wm))
    o.close()
    return out


@pytest.mark.parametrize("kind", ALL_KINDS)
@pytest.mark.parametrize("stream", ["finite", "special"])
def test_oracle_lies_inside_the_reference(stream, kind):
    kw, ref = F.case(stream, kind)
    assert ref.n_rows > 300
    rows = 0
    for b, ro in enumerate(oracle_rows(kw, ref)):
        if ro is not None:
            rows += F.compare_rows(ro, ref, b, ORACLE_AGGS, ctx="oracle %s %s" % (stream, kind),
                                   mode="oracle_merged" if kind.startswith("session") else "oracle",
                                   only=("COUNT", "SUM_F64", "AVG_F64", "MIN_F64", "MAX_F64", "MIN_F32", "MAX_F32"))
    assert rows == ref.n_rows


@pytest.mark.parametrize("kind", ALL_KINDS)
@pytest.mark.parametrize("stream", ["finite", "special"])
def test_intervals_are_well_formed(stream, kind):
    _, ref = F.case(stream, kind)
    n = 0
    for name, c in (("SUM_F64", 0), ("AVG_F64", 0), ("SUM_F32", 1), ("AVG_F32", 1), ("SUM_F64", 2), ("AVG_F32", 3)):
        for exp in ref.expect(name, c):
            for e in exp or ():
                if e[0] in ("frac", "range"):
                    assert e[1] <= e[2], (name, c, e)
                    n += 1
    assert n > 500


@pytest.mark.parametrize("kind", F.TABLE_KINDS)
def test_finite_stream_holds_what_it_is_meant_to(kind):
    """Ill-conditioned sums in a tenth of the rows, subnormal results, float sums at or past FLT_MAX, late drops."""
    kw, ref = F.case("finite", kind)
    assert 1 << 13 < len(ref.keys) < 1 << 15
    assert ref.n_late > 50
    ill = sub = over = 0
    base, f32 = ref.sum_base(0), ref.expect("SUM_F32", 1)
    mins = [ref.expect("MIN_F64", 0), ref.expect("MAX_F64", 0), ref.expect("MIN_F32", 1), ref.expect("MAX_F32", 1)]
    oracle = oracle_rows(kw, ref)
    for b, i, idx in ref.each_row():
        e = base[b][i]
        assert e[0] == "fin"                                             # no NaN and no infinity in this stream
        _, S, Aq = e[:3]
        ill += abs(S) < Aq / 1000
        sub += (0 < abs(S) < TINY64) or any(0 < abs(float(m[b][i][1])) < (TINY64 if j < 2 else TINY32)
                                            for j, m in enumerate(mins))
        over += bool(np.isinf(f32[b][i][1]) or np.isinf(f32[b][i][2]))
    for b, ro in enumerate(oracle):                                      # rows on which the oracle's float fold overflowed
        if ro is not None:
            x = ro["agg5"][np.lexsort((ro["win_end"], ro["win_start"], ro["key"]))]
            over += int(sum(not np.isfinite(v) and np.isfinite(e[1]) and np.isfinite(e[2])
                            for v, e in zip(x, f32[b])))
    assert ill * 10 >= ref.n_rows, (ill, ref.n_rows)
    assert sub >= 20 and over >= 20, (sub, over)
    zeros = ref.column(0).w[ref.column(0).w == 0]
    assert len(set(np.signbit(zeros).tolist())) == 2                     # both zeros among the inputs


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_special_stream_holds_every_class(kind):
    """At least 20 rows per class show the class's special value, in the DOUBLE and in the FLOAT column; a class
    confined to one slice also has 20 clean rows, and 20 clean rows of windows that end behind the last window holding
    that slice (fired after it retired, from slots used again)."""
    _, ref = F.case("special", kind)
    ncls = len(F.SPECIAL_CLASSES)
    for c in (0, 1):
        w = ref.column(c).w
        hit = dict.fromkeys(F.SPECIAL_CLASSES, 0)
        clean = dict.fromkeys(F.CONFINED, 0)
        behind = dict.fromkeys(F.CONFINED, 0)
        for b, i, idx in ref.each_row():
            key = int(ref.rows[b]["key"][i])
            if key == F.SEED_KEY:
                continue
            name = F.SPECIAL_CLASSES[key % ncls]
            if F.holds_special(name, w[idx]):
                hit[name] += 1
            elif name in F.CONFINED:
                assert np.isfinite(w[idx]).all()
                clean[name] += 1
                behind[name] += int(ref.rows[b]["win_end"][i]) > (F.CONFINED[name] + 4) * F.SLICE
        assert min(hit.values()) >= 20, (kind, c, hit)
        if kind in ("hop", "cumulate"):
            assert min(clean.values()) >= 20 and min(behind.values()) >= 20, (kind, clean, behind)


def test_membership_rule_rows():
    """The rule was checked against the oracle's COUNT on every row of every case (Reference asserts it)."""
    for kind in ALL_KINDS:
        for stream in ("finite", "special"):
            _, ref = F.case(stream, kind)
            assert sum(len(idx) == c for b, i, idx in ref.each_row() for c in [ref.rows[b]["count"][i]]) == ref.n_rows
