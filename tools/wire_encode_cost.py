"""What the wire encoder costs (flink_amd/csrc/wire_encode.inc, fwa_wire_encode): the encoder's HIP-event time per call
for three shapes of a C2-sized fire (--rows rows per watermark, device-resident columns, one watermark element behind
them), beside a device-to-device copy of the same number of output bytes timed in the same run.

Shapes:
  rowdata  key, window_start, window_end, sum, count as a BinaryRowData row without timestamp: 57-byte elements
  tuple    key, window_start, sum, count as a Tuple4 with the record timestamp win_end - 1: 45-byte elements
  string   one VARCHAR key column of 8..40 bytes (length a function of the row) beside window_start, window_end, sum,
           count: 65..97-byte elements; the size pass, the scan and the write pass are reported separately
The three are encoded in turn, --reps rounds after one warm-up round, each followed by its copy, so every figure of a
shape is taken beside the others'. Numbers per shape, mean and minimum over the rounds:
  encode_ms   fwa_wire_enc_stats.encode_ms (HIP events on the encoder's stream around its kernels)
  copy_ms     torch events around dst.copy_(src) of as many bytes: the floor the write pass is compared against
              (it reads and writes every byte once; the encoder reads 40 B of columns per row instead). A reference,
              not a target.
  GB/s        output bytes / encode_ms, a whole-call rate
Output: python tools/wire_encode_cost.py > profiles/<tag>_wire_encode_cost.txt"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from flink_amd import _abi as A  # noqa: E402
from flink_amd import wire  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("wire_encode_cost.py measures on the GPU: none found")
dev = torch.device("cuda", 0)
N = args.rows
g = torch.Generator(device=dev)
g.manual_seed(0x5eed)
key = torch.randint(-(1 << 62), 1 << 62, (N,), device=dev, generator=g, dtype=torch.int64)
win_start = 1_700_000_000_000 + (torch.arange(N, device=dev, dtype=torch.int64) % 7) * 10_000
win_end = win_start + 10_000
total = torch.randint(-(1 << 40), 1 << 40, (N,), device=dev, generator=g, dtype=torch.int64)
count = torch.randint(1, 1 << 20, (N,), device=dev, generator=g, dtype=torch.int64)
lens = 8 + (torch.arange(N, device=dev, dtype=torch.int64) * 7919) % 33
offs = torch.zeros(N + 1, dtype=torch.int32, device=dev)
offs[1:] = torch.cumsum(lens, 0).to(torch.int32)
chars = torch.randint(0x20, 0x7F, (int(offs[-1].item()),), device=dev, generator=g, dtype=torch.int64).to(torch.uint8)

out = A.Out()
out.n_rows, out.on_device, out.num_aggs = N, 1, 2
out.key, out.win_start, out.win_end = key.data_ptr(), win_start.data_ptr(), win_end.data_ptr()
out.agg[0], out.agg[1] = total.data_ptr(), count.data_ptr()
AGGS = [("LONG", ("AGG", 0, "SUM_I64")), ("LONG", ("AGG", 1, "COUNT"))]
SHAPES = {
    "rowdata": (wire.make_out_schema([("LONG", "KEY"), ("LONG", "WIN_START"), ("LONG", "WIN_END")] + AGGS, fmt="ROWDATA"), None),
    "tuple": (wire.make_out_schema([("LONG", "KEY"), ("LONG", "WIN_START")] + AGGS, fmt="TUPLE", record_ts="WIN_TIME"), None),
    "string": (wire.make_out_schema([("STRING", ("KEYCOL", 0, "STRING")), ("LONG", "WIN_START"), ("LONG", "WIN_END")] + AGGS,
                                    fmt="ROWDATA"), ([(offs, chars)], None)),
}
WM = [(wire.TAG_WATERMARK, (1_700_000_060_000,))]
enc = {name: wire.WireEncoder(s) for name, (s, _) in SHAPES.items()}
samples = {name: [] for name in SHAPES}
nbytes = {}
for rep in range(args.reps + 1):
    for name, (_, kc) in SHAPES.items():
        e = enc[name]
        s0 = e.stats()
        view = e.encode(out, keycols=kc, events=WM)
        s1 = e.stats()
        nbytes[name] = view.numel()
        dst = torch.empty_like(view)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(view)
        b.record()
        torch.cuda.synchronize()
        if rep:
            samples[name].append((s1.encode_ms - s0.encode_ms, s1.size_ms - s0.size_ms, s1.scan_ms - s0.scan_ms, a.elapsed_time(b)))
        del dst

print("%d rows per call, %d timed rounds after one warm-up, the shapes in turn; HIP-event times per call" % (N, args.reps))
for name, xs in samples.items():
    r = len(xs)
    mean = [sum(x[i] for x in xs) / r for i in range(4)]
    low = [min(x[i] for x in xs) for i in range(4)]
    nb = nbytes[name]
    line = "%-8s %6.1f MB (%.1f B/row): encode %.3f ms (min %.3f), copy of as many bytes %.3f ms (min %.3f), encode / copy %.2f; %.0f GB/s" % (
        name, nb / 1e6, nb / N, mean[0], low[0], mean[3], low[3], mean[0] / mean[3], nb / mean[0] / 1e6)
    if name == "string":
        line += "; size pass %.3f ms, scan %.3f ms, write pass %.3f ms (write / copy %.2f)" % (
            mean[1], mean[2], mean[0] - mean[1] - mean[2], (mean[0] - mean[1] - mean[2]) / mean[3])
    print(line, flush=True)
for e in enc.values():
    e.close()
