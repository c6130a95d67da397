"""What DECIMAL(38) fields cost on the wire (FWA_FIELD_DECIMAL; flink_amd/csrc/wire_encode.inc, wire.hip): the
encoder's and the decoder's HIP-event times per call for one schema with DECIMAL fields, beside the same schema with LONG
in their place and a STRING-keyed schema, all in one process and in turn.

Shapes (--rows rows per call, device-resident columns, one watermark element behind the rows, ROWDATA without timestamp):
  decimal  key, SUM_DEC128, COUNT, AVG_DEC, window_start, window_end with a quarter of each DECIMAL column NULL: 65-byte
           fixed part + 16 per non-NULL DECIMAL (the values' lengths run from 1 to 16 bytes); size, scan and write passes
  long     the same six fields with LONG (SUM_I64) in place of the two DECIMALs: 65-byte elements, the fixed-length kernel
  string   one VARCHAR key column of 8..40 bytes beside window_start, window_end, sum, count (tools/wire_encode_cost.py's)
Each round encodes the three shapes in turn and decodes each shape's bytes (still in HBM) with the GPU decoder; --reps
timed rounds after one warm-up round. Per shape: the median (minimum) of
  encode_ms   fwa_wire_enc_stats.encode_ms per call, and its size / scan shares
  decode_ms   fwa_wire_stats.decode_ms per call, and its scan share
and the bytes moved per row: column bytes read and element bytes written by the encoder; element bytes read (twice: scan
and decode) and column bytes written by the decoder.
--lib PATH loads another build of the library (the parent commit's, to compare the shapes without DECIMAL fields on one
box in one session); a library that refuses the DECIMAL schema reports so and measures the rest. What runs before a
shape in the round moves its figures by a few per cent, so builds are compared with the same --shapes list.
Output: python tools/wire_decimal_cost.py > profiles/<tag>_wire_decimal_cost.txt"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from flink_amd import _abi as A  # noqa: E402
from flink_amd import engine  # noqa: E402
from flink_amd import wire  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1 << 20)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--shapes", default="decimal,long,string", help="the shapes to run, in this order")
ap.add_argument("--lib", default=None, help="another libflink_amd.so to measure (default: this tree's)")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("wire_decimal_cost.py measures on the GPU: none found")
if args.lib:
    engine.LIB_PATH = os.path.abspath(args.lib)
dev = torch.device("cuda", 0)
N = args.rows
g = torch.Generator(device=dev)
g.manual_seed(0x5eed)


def rnd(lo, hi):
    return torch.randint(lo, hi, (N,), device=dev, generator=g, dtype=torch.int64)


idx = torch.arange(N, device=dev, dtype=torch.int64)
key = rnd(-(1 << 62), 1 << 62)
win_start = 1_700_000_000_000 + (idx % 7) * 10_000
win_end = win_start + 10_000
count = rnd(1, 1 << 20)
total = rnd(-(1 << 40), 1 << 40)


def dec128(shift_by):
    """[N, 2] (low, high). Even rows: a 64-bit value shifted right arithmetically by 0..62 and sign-extended (1..8 bytes
    on the wire); odd rows: the high half shifted by 0..63 over a random low half (8..16 bytes)."""
    small = rnd(-(1 << 62), 1 << 62) >> ((idx + shift_by) % 63)
    lo = torch.where(idx % 2 == 0, small, rnd(-(1 << 62), 1 << 62))
    hi = torch.where(idx % 2 == 0, small >> 63, rnd(-(1 << 62), 1 << 62) >> ((idx + shift_by) % 64))
    return torch.stack([lo, hi], 1).contiguous()


d0, d2 = dec128(0), dec128(31)
z0 = (rnd(0, 4) == 0).to(torch.uint8)
z2 = (rnd(0, 4) == 0).to(torch.uint8)
lens = 8 + (idx * 7919) % 33
offs = torch.zeros(N + 1, dtype=torch.int32, device=dev)
offs[1:] = torch.cumsum(lens, 0).to(torch.int32)
chars = torch.randint(0x20, 0x7F, (int(offs[-1].item()),), device=dev, generator=g, dtype=torch.int64).to(torch.uint8)


def rows(aggs, nulls=()):
    out = A.Out()
    out.n_rows, out.on_device, out.num_aggs = N, 1, len(aggs)
    out.key, out.win_start, out.win_end = key.data_ptr(), win_start.data_ptr(), win_end.data_ptr()
    for j, a in enumerate(aggs):
        out.agg[j] = a.data_ptr()
        if j < len(nulls) and nulls[j] is not None:
            out.agg_null[j] = nulls[j].data_ptr()
    return out


TAIL = [("LONG", "WIN_START"), ("LONG", "WIN_END")]
SHAPES = {
    "decimal": dict(
        out=rows([d0, count, d2], [z0, None, z2]), kc=None, read=8 + 17 + 8 + 17 + 16,
        enc=[("LONG", "KEY"), ("DECIMAL", ("AGG", 0, "SUM_DEC128")), ("LONG", ("AGG", 1, "COUNT")),
             ("DECIMAL", ("AGG", 2, "AVG_DEC"))] + TAIL,
        dec=dict(fields=["LONG", "DECIMAL", "LONG", "DECIMAL", "LONG", "LONG"], key_field=0, ts_field=5, cols=[1, 2, 3, 4]),
        written=69),
    "long": dict(
        out=rows([total, count, total], [z0, None, z2]), kc=None, read=8 + 9 + 8 + 9 + 16,
        enc=[("LONG", "KEY"), ("LONG", ("AGG", 0, "SUM_I64")), ("LONG", ("AGG", 1, "COUNT")),
             ("LONG", ("AGG", 2, "SUM_I64"))] + TAIL,
        dec=dict(fields=["LONG"] * 6, key_field=0, ts_field=5, cols=[1, 2, 3, 4]), written=53),
    "string": dict(
        out=rows([total, count]), kc=([(offs, chars)], None), read=None,
        enc=[("STRING", ("KEYCOL", 0, "STRING"))] + TAIL + [("LONG", ("AGG", 0, "SUM_I64")), ("LONG", ("AGG", 1, "COUNT"))],
        dec=dict(fields=["STRING", "LONG", "LONG", "LONG", "LONG"], key_field=-1, ts_field=2, cols=[1, 3, 4]),
        written=48),
}
WM = [(wire.TAG_WATERMARK, (1_700_000_060_000,))]
print("%d rows per call, %d timed rounds after one warm-up, the shapes in turn; HIP-event times per call, median (minimum); library %s"
      % (N, args.reps, args.lib or "of this tree"))
live = {}
for name in args.shapes.split(","):
    s = SHAPES[name]
    try:
        live[name] = (wire.WireEncoder(wire.make_out_schema(s["enc"], fmt="ROWDATA")),
                      wire.WireDecoder(wire.make_schema(fmt="ROWDATA", **s["dec"])))
    except engine.EngineError as e:
        print("%-8s refused by this library: %s" % (name, e))
samples = {name: [] for name in live}
nbytes = {}
for rep in range(args.reps + 1):
    for name, (enc, dec) in live.items():
        s = SHAPES[name]
        e0, d0s = enc.stats(), dec.stats()
        view = enc.encode(s["out"], keycols=s["kc"], events=WM)
        batch = dec.decode(view)
        assert batch.n_records == N and batch.consumed == view.numel() and batch.n_events == 1
        e1, d1s = enc.stats(), dec.stats()
        nbytes[name] = view.numel()
        if rep:
            samples[name].append((e1.encode_ms - e0.encode_ms, e1.size_ms - e0.size_ms, e1.scan_ms - e0.scan_ms,
                                  d1s.decode_ms - d0s.decode_ms, d1s.scan_ms - d0s.scan_ms))
for name, xs in samples.items():
    med = [statistics.median(x[i] for x in xs) for i in range(5)]
    low = [min(x[i] for x in xs) for i in range(5)]
    per = (nbytes[name] - 13) / N
    s = SHAPES[name]
    rd = "%d" % s["read"] if s["read"] else "40 + %.1f" % (float(offs[-1].item()) / N + 4)
    print("%-8s %6.1f MB, %.1f B/row on the wire | encode %.3f ms (min %.3f; size %.3f, scan %.3f), %s B/row read + %.1f written, %.0f GB/s of "
          "wire bytes | decode %.3f ms (min %.3f; scan %.3f), 2 x %.1f B/row read + %d written, %.0f GB/s of wire bytes"
          % (name, nbytes[name] / 1e6, per, med[0], low[0], med[1], med[2], rd, per, nbytes[name] / med[0] / 1e6,
             med[3], low[3], med[4], per, s["written"], nbytes[name] / med[3] / 1e6), flush=True)
for enc, dec in live.values():
    enc.close()
    dec.close()
