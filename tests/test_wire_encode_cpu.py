"""CPU checks around the wire encoder (fwa_wire_encode): the two reference encoders the GPU is judged by agree with each
other and with the sequential reference decoder, and the argument checks that need no device."""
import numpy as np
import pytest

from flink_amd import wire
from oracle import wire_encode as W

import wire_strings_ref as R

ROW = ["LONG", "LONG", "DOUBLE", "INT", "LONG"]


def _rows(rng, n):
    k = rng.integers(-(1 << 62), 1 << 62, n)
    a = rng.integers(-(1 << 40), 1 << 40, n)
    d = rng.standard_normal(n)
    i = rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32)
    e = rng.integers(0, 1 << 45, n)
    nulls = [None, rng.random(n) < 0.3, rng.random(n) < 0.3, rng.random(n) < 0.3, None]
    return [k, a, d, i, e], nulls


@pytest.mark.parametrize("with_ts", [False, True])
def test_fixed_rowdata_references_agree(with_ts):
    """oracle.wire_encode and wire_strings_ref write the same bytes for rows without strings, and the reference decoder
    reads them back: columns, NULL flags, timestamps and the trailing events."""
    rng = np.random.default_rng(3)
    n = 300
    vals, nulls = _rows(rng, n)
    ts = rng.integers(0, 1 << 44, n) if with_ts else None
    events = [(n, 2, (12345,)), (n, 4, (-1,)), (n, 3, (1, 2, 3, 4)), (n, 5, (1,))]
    a = W.encode_stream(ROW, vals, ts, "ROWDATA", events, nulls)
    rows = [tuple(None if (m is not None and m[r]) else (float(v[r]) if f == "DOUBLE" else int(v[r]))
                  for f, v, m in zip(ROW, vals, nulls)) for r in range(n)]
    b, starts = R.encode_stream(ROW, rows, ts, events)
    assert a == b and len(starts) == n
    rc, got = R.decode(ROW, a, key_field=0, ts_field=-1, cols=[1, 2, 3, 4])
    assert rc == 0 and got["n_records"] == n and got["consumed"] == len(a)
    assert np.array_equal(got["key"], vals[0])
    if with_ts:
        assert np.array_equal(got["ts"], ts)
    for j, f in enumerate([1, 2, 3, 4]):
        z = np.zeros(n, bool) if nulls[f] is None else nulls[f]
        assert np.array_equal(got["col_null"][j].astype(bool), z)
        want = np.where(z, 0, vals[f]).astype(W.FIELD_NP[ROW[f]])
        if ROW[f] == "INT":
            want = want.astype(np.int64)                                  # the decoder sign-extends INT columns
        assert np.array_equal(got["cols"][j].view(np.uint8), want.view(np.uint8))
    assert got["evt_tag"].tolist() == [2, 4, 3, 5] and got["evt_pos"].tolist() == [n] * 4
    assert got["evt_val"].tolist() == [[12345, 0, 0, 0], [-1, 0, 0, 0], [1, 2, 3, 4], [1, 0, 0, 0]]


def test_string_reference_reads_back_what_it_writes():
    rng = np.random.default_rng(4)
    fields = ["STRING", "LONG", "STRING", "DOUBLE"]
    lens = [0, 1, 6, 7, 8, 9, 15, 16, 17, 40]
    rows = []
    for i in range(200):
        s = None if i % 11 == 0 else "a" * lens[i % 10]
        t = None if i % 7 == 0 else "b" * lens[(i * 3) % 10]
        rows.append((s, i - 100, t, None if i % 5 == 0 else float(i) / 3))
    data, starts = R.encode_stream(fields, rows, None, [(200, 2, (77,))])
    rc, got = R.decode(fields, data, cols=[1, 3])
    assert rc == 0 and got["n_records"] == 200 and got["consumed"] == len(data)
    for f in (0, 2):
        o, b, z = got["strings"][f]
        for i, r in enumerate(rows):
            assert bool(z[i]) == (r[f] is None)
            assert bytes(b[o[i]:o[i + 1]]) == (b"" if r[f] is None else r[f].encode())
    assert got["cols"][0].view(np.int64).tolist() == [r[1] for r in rows]
    assert got["evt_tag"].tolist() == [2] and got["evt_val"][0, 0] == 77
    # element sizes: fixed part + the 8-rounded lengths of the values longer than 7 bytes
    sizes = np.diff(starts + [len(data) - 13])
    want = [4 + 5 + 8 + 32 + sum((len(v) + 7) // 8 * 8 for v in (r[0], r[2]) if v is not None and len(v) > 7) for r in rows]
    assert sizes.tolist() == want


def test_make_out_schema_arguments():
    ok = wire.make_out_schema([("LONG", "KEY"), ("LONG", ("AGG", 0, "SUM_I64")), ("DOUBLE", ("AGG", 1, "AVG_F64")),
                               ("STRING", ("KEYCOL", 0, "STRING")), ("LONG", "WIN_TIME")], fmt="ROWDATA")
    assert (ok.format, ok.arity, ok.record_ts) == (1, 5, 0)
    assert list(ok.field)[:5] == [0, 0, 1, 4, 0] and list(ok.src)[:5] == [0, 5, 5, 1, 4]
    assert list(ok.src_index)[:5] == [0, 0, 1, 0, 0] and list(ok.src_kind)[:5] == [0, 1, 12, 3, 0]
    assert wire.make_out_schema([("LONG", "KEY")], record_ts="WIN_TIME").record_ts == 1
    import flink_amd
    assert flink_amd.make_out_schema is wire.make_out_schema and flink_amd.WireEncoder is wire.WireEncoder
    assert flink_amd.NetworkOutput is wire.NetworkOutput
    bad = [
        (dict(fields=[]), "arity 0"),
        (dict(fields=[("LONG", "KEY")] * 17), "arity 17"),
        (dict(fields=[("LONG", "KEY")], fmt="AVRO"), "wire format"),
        (dict(fields=[("LONG", "KEY")], record_ts="KEY"), "record_ts"),
        (dict(fields=["KEY"]), "pair"),
        (dict(fields=[("DECIMAL", "KEY")]), "wire type"),
        (dict(fields=[("LONG", "WINDOW")]), "source"),
        (dict(fields=[("LONG", "AGG")]), "triples"),
        (dict(fields=[("LONG", ("AGG", 0))]), "AGG"),
        (dict(fields=[("LONG", ("AGG", 0, "MEDIAN"))]), "aggregate kind"),
        (dict(fields=[("LONG", ("AGG", 8, "COUNT"))]), "out of range"),
        (dict(fields=[("LONG", ("KEYCOL", 0, "VARCHAR"))]), "key field type"),
        (dict(fields=[("LONG", ("KEYCOL", -1, "BIGINT"))]), "out of range"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            wire.make_out_schema(**kw)


def test_encoder_struct_sizes_match_header():
    """The ctypes mirrors of the encoder's structs against the C layout (a probe compiled with gcc)."""
    import ctypes
    import os
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "flink_amd_wire.h"
int main(void){printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(fwa_wire_out_schema), sizeof(fwa_wire_keycols),
 sizeof(fwa_wire_event), sizeof(fwa_wire_bytes), sizeof(fwa_wire_enc_stats), offsetof(fwa_wire_out_schema, record_ts),
 offsetof(fwa_wire_keycols, str));return 0;}
'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [ctypes.sizeof(x) for x in (wire.OutSchema, wire.KeyCols, wire.Event, wire.WireBytes, wire.EncStats)] + \
        [wire.OutSchema.record_ts.offset, wire.KeyCols.str.offset]


def test_create_refuses_a_bad_schema_before_it_touches_a_device():
    """fwa_wire_enc_create checks the schema first, so its refusals and their messages need no GPU."""
    cases = [
        ([("STRING", ("KEYCOL", 0, "STRING"))], "TUPLE", -1, "ROWDATA rows only"),
        ([("LONG", ("AGG", 0, "SUM_F64"))], "TUPLE", -1, "a double source cannot be written as LONG"),
        ([("FLOAT", ("AGG", 0, "SUM_I32"))], "ROWDATA", -1, "an int32 source cannot be written as FLOAT"),
        ([("LONG", ("KEYCOL", 1, "STRING"))], "ROWDATA", -1, "a STRING source cannot be written as LONG"),
        ([("LONG", "KEY"), ("LONG", ("AGG", 0, "SUM_DEC128"))], "ROWDATA", -7, "DECIMAL"),
    ]
    for fields, fmt, code, msg in cases:
        with pytest.raises(Exception) as ei:
            wire.WireEncoder(wire.make_out_schema(fields, fmt=fmt))
        assert ei.value.code == code and msg in str(ei.value), str(ei.value)
    for arity in (0, 17):
        s = wire.make_out_schema([("LONG", "KEY")])
        s.arity = arity
        with pytest.raises(Exception) as ei:
            wire.WireEncoder(s)
        assert ei.value.code == -1 and ("arity %d out of range" % arity) in str(ei.value)
