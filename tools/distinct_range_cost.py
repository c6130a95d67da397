"""What COUNT(DISTINCT) over HOP windows costs (FWA_CFG_DISTINCT_RANGE, flink_amd/csrc/distinct.inc): the marking pass
of every push and the two passes of every firing step.

Stream: the C3 stream of bench.py scaled down to a short run -- HOP 60 s / 1 s (Table), Zipf(1.1) keys over --keys
items, 1e6 records per second of event time, bounded out-of-orderness 1 s, --batch records per push (2^24: 16.8 s of
event time, so a step fires 16 or 17 windows), inputs in HBM, --warmup pushes then --pushes timed pushes, each followed
by its watermark. Three handles over the same records (--kinds selects some), run one after the other, --repeats
times alternating:
  sum       COUNT + SUM_I64(v)                                    (the same handle without the distinct aggregate)
  distinct  COUNT + COUNT_DISTINCT(v & 15) under the flag         (16 values per key)
  distsum   distinct + SUM_DISTINCT_I64(v & 15)                   (FWA_AGG_DISTINCT: the count pass also adds each
            counted value and 1 to two per-row columns, and a finish kernel writes the sum and its NULL flag)
Numbers, per timed step (means over the timed steps of a run; every run is printed, so the spread is visible):
  step      push + watermark, host clock around calls that end in a device synchronise
  fire      fwa_stats.fire_ms (HIP events on the handle's stream; for the distinct handle it includes the two passes)
  marking   fwa_stats.ingest_ms - partition_ms - combine_ms (the range-mode marking kernel, HIP events)
  index     FWA_OPT_DISTINCT_INDEX_US (dist_rows_index_kernel, HIP events)
  count     FWA_OPT_DISTINCT_COUNT_US (dist_range_count_kernel, HIP events)
and the set's slots, live block entries and rebuilds at the end.
Output: python tools/distinct_range_cost.py --kinds sum,distinct > profiles/<tag>_distinct_range_cost.txt
        python tools/distinct_range_cost.py > profiles/<tag>_distinct_sum_range_cost.txt"""
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
ap.add_argument("--pushes", type=int, default=6)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=2)
ap.add_argument("--batch", type=int, default=1 << 24)
ap.add_argument("--keys", type=int, default=1_000_000)
ap.add_argument("--kinds", default="sum,distinct,distsum")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("distinct_range_cost.py measures on the GPU: none found")

B, S = args.batch, args.warmup + args.pushes
dev = torch.device("cuda", 0)
w = 1.0 / np.arange(1, args.keys + 1, dtype=np.float64) ** 1.1
zcdf = torch.from_numpy(np.cumsum(w) / w.sum()).to(dev)
p = A.GenParams(seed_k=0x5eed0001, seed_t=0x5eed0002, seed_v=0x5eed0003, first_index=0, total_records=S * B,
                num_keys=args.keys, t0_ms=1_700_000_000_000, span_ms=S * B * 1_000_000 // 1_000_000_000,
                max_delay_ms=1000, key_dist=1, val_kind=0)
p.zipf_cdf = zcdf.data_ptr()
keys = torch.empty(S * B, dtype=torch.int64, device=dev)
ts = torch.empty_like(keys)
vals = torch.empty_like(keys)
E.generate(p, S * B, keys, ts, vals)
dcol = torch.bitwise_and(vals, 15)
torch.cuda.synchronize()
bmax = ts.view(S, B).max(dim=1).values.cpu().numpy()
wms = np.maximum.accumulate(bmax) - 1001


def run(kind):
    aggs = [("COUNT", 0), ("SUM_I64", 0)] if kind == "sum" else [("COUNT", 0), ("COUNT_DISTINCT", 0)]
    if kind == "distsum":
        aggs.append(("SUM_DISTINCT_I64", 0))
    g = E.WindowAggregator(A.make_config(window_kind="SLIDE", semantics="TABLE", size_ms=60_000, slide_ms=1_000, aggs=aggs,
                                         key_capacity=args.keys, output_on_device=1, distinct_range=kind != "sum"))
    col = vals if kind == "sum" else dcol
    wall, rows, base = 0.0, 0, (0, 0, 0)
    for b in range(S):
        sl = slice(b * B, (b + 1) * B)
        if b == args.warmup:
            g.reset_timers()
            if kind != "sum":
                base = tuple(g.get_option(n) for n in ("distinct_index_us", "distinct_count_us", "distinct_count_steps"))
        t0 = time.perf_counter()
        g.push(keys[sl], ts[sl], [col[sl]])
        n = g.advance_watermark_raw(int(wms[b])).n_rows
        torch.cuda.synchronize()
        if b >= args.warmup:
            wall += time.perf_counter() - t0
            rows += n
    st = g.stats()
    n = args.pushes
    line = "%-8s step %8.2f ms; fire %7.2f ms; ingest %7.2f ms (marking %6.2f); rows/step %d" % (
        kind, wall / n * 1e3, st.fire_ms / n, st.ingest_ms / n,
        (st.ingest_ms - st.partition_ms - st.combine_ms) / n if kind != "sum" else 0.0, rows // n)
    if kind != "sum":
        now = tuple(g.get_option(x) for x in ("distinct_index_us", "distinct_count_us", "distinct_count_steps"))
        steps = max(1, now[2] - base[2])
        slots = g.get_option("distinct_slots")
        line += "; index %.3f ms, count %.3f ms per step (%d steps); set %d slots (%.2f GB), %d live blocks, %d rebuilds" % (
            (now[0] - base[0]) / 1e3 / steps, (now[1] - base[1]) / 1e3 / steps, steps, slots, slots * 32 / 1e9,
            g.get_option("distinct_live"), g.get_option("distinct_rebuilds"))
    print(line + "; late %d" % st.late_dropped, flush=True)
    g.close()


print("C3-shaped stream, %d timed pushes of %d records after %d warm-up, %d Zipf(1.1) keys, HOP 60 s / 1 s (Table)"
      % (args.pushes, B, args.warmup, args.keys), flush=True)
for _ in range(args.repeats):
    for kind in args.kinds.split(","):
        run(kind)
