"""What the exact SUM(FLOAT) costs (FWA_CFG_F32_FOLD, flink_amd/csrc/f32fold.inc): the fold pass ahead of the ingest and
the lookup at the fire.

Stream: a C2-shaped stream of fwa_generate with a FLOAT value column (1e6 records per second of event time, bounded
out-of-orderness 1 s, inputs in HBM), Table TUMBLE 10 s, aggregates COUNT + SUM_F32, one warm-up push then --pushes
timed pushes, each followed by its watermark. Two lines, each pushing the same records through one build twice, flag
off and flag on:
  uniform   1M uniform keys, 2^26 records per push: ~64 records per (key, window) run and push
  zipf      Zipf(1.1) over the same keys, 2^22 records per push: the hot key's run is one serial walk by one lane (a
            float32 fold cannot be split or tree-reduced without changing its bits), which is the honest price of the
            exact result on skewed keys
Numbers per push: device ms of resolve, sort and fold (FWA_OPT_F32_FOLD_*_US: HIP events on the handle's stream, also
part of fwa_stats.ingest_ms), the fire's lookup per watermark, the handle's whole ingest_ms, G rec/s over
push + watermark by the host clock (calls that end in a synchronise), and the ratio on / off of that wall time.
Bytes the pass moves per record: resolve reads key 8 + ts 8, probes one 16-byte entry, writes slot 4 + index 4; the
sort reads and writes 8 B per record and digit pass; the fold reads slot 4 + index 4 and gathers one 4-byte value.
A step that hangs on the hot key's run is ended from outside: run each line under its own time limit, sized from the
uniform line, e.g.
    timeout -k 10 300 python tools/f32_fold_cost.py --line uniform > profiles/<tag>_f32_fold_cost.txt
    timeout -k 10 300 python tools/f32_fold_cost.py --line zipf >> profiles/<tag>_f32_fold_cost.txt"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from flink_amd import _abi as A  # noqa: E402
from flink_amd import engine as E  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--line", choices=["uniform", "zipf"], default="uniform")
ap.add_argument("--pushes", type=int, default=4)
ap.add_argument("--batch", type=int, default=0, help="records per push (0: 2^26 uniform, 2^22 zipf)")
ap.add_argument("--keys", type=int, default=1_000_000)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("f32_fold_cost.py measures on the GPU: none found")

zipf = args.line == "zipf"
B, S = args.batch or (1 << 22 if zipf else 1 << 26), args.pushes + 1
dev = torch.device("cuda", 0)
p = A.GenParams(seed_k=0x5eed0001, seed_t=0x5eed0002, seed_v=0x5eed0003, first_index=0, total_records=S * B,
                num_keys=args.keys, t0_ms=1_700_000_000_000, span_ms=S * B * 1_000_000 // 1_000_000_000,
                max_delay_ms=1000, key_dist=1 if zipf else 0, val_kind=1)
if zipf:
    w = 1.0 / np.arange(1, args.keys + 1, dtype=np.float64) ** 1.1
    zcdf = torch.from_numpy(np.cumsum(w) / w.sum()).to(dev)
    p.zipf_cdf = zcdf.data_ptr()
keys = torch.empty(B, dtype=torch.int64, device=dev)
ts = torch.empty_like(keys)
vals = torch.empty(B, dtype=torch.float32, device=dev)
vals_d = torch.empty(B, dtype=torch.float64, device=dev)


def batch(b):
    p.first_index = b * B
    E.generate(p, B, keys, ts, None, vals, vals_d)
    torch.cuda.synchronize()
    return int(ts.max().item())


def run(flag):
    g = E.WindowAggregator(A.make_config(window_kind="TUMBLE", semantics="TABLE", size_ms=10_000, f32_fold=flag,
                                         aggs=[("COUNT", 0), ("SUM_F32", 0)], key_capacity=args.keys, output_on_device=1))
    mx, wall, rows, base = -2**63, 0.0, 0, {}
    opts = ("f32_fold_resolve_us", "f32_fold_sort_us", "f32_fold_runs_us", "f32_fold_rows_us")
    for b in range(S):
        mx = max(mx, batch(b))
        if b == 1:
            g.reset_timers()
            base = {o: g.get_option(o) for o in opts} if flag else {}
        t0 = time.perf_counter()
        g.push(keys, ts, [vals])
        rows += g.advance_watermark_raw(mx - 1001).n_rows
        torch.cuda.synchronize()
        if b >= 1:
            wall += time.perf_counter() - t0
    st = g.stats()
    n = args.pushes
    line = "%-7s flag %-3s %6.3f G rec/s (push + watermark %.2f ms); ingest %.2f ms/push, fire %.2f ms/push" % (
        args.line, "on" if flag else "off", n * B / wall / 1e9, wall / n * 1e3, st.ingest_ms / n, st.fire_ms / n)
    if flag:
        ms = {o: (g.get_option(o) - base[o]) / 1e3 / n for o in opts}
        slots = g.get_option("f32_fold_slots")
        line += ("; fold pass: resolve %.2f + sort %.2f + fold %.2f ms/push, lookup %.3f ms/watermark; set %.2f GB "
                 "(%d slots), %d rebuilds" % (ms[opts[0]], ms[opts[1]], ms[opts[2]], ms[opts[3]], slots * 20 / 1e9, slots,
                                              g.get_option("f32_fold_rebuilds")))
    print(line + "; rows %d, late %d" % (rows, st.late_dropped), flush=True)
    g.close()
    return wall / n


print("%s keys, %d timed pushes of %d records after one warm-up, %d keys, TUMBLE 10 s (Table), COUNT + SUM_F32"
      % ("Zipf(1.1)" if zipf else "uniform", args.pushes, B, args.keys), flush=True)
off = run(False)
on = run(True)
print("%-7s push + watermark on / off = %.2f" % (args.line, on / off), flush=True)
