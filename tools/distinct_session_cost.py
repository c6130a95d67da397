"""What COUNT(DISTINCT) over Table SESSION windows costs (FWA_CFG_DISTINCT_SESSION, flink_amd/csrc/distinct.inc): the
marking pass behind every push's ingest and the three passes of every firing step.

Stream: the C5s stream of bench.py as a Table handle -- SESSION gap 5 s, uniform keys over --keys items, 1e6 records
per second of event time, bounded out-of-orderness 1 s, --batch records per push (2^26: 67 s of event time), inputs in
HBM, --warmup pushes then --pushes timed pushes, each followed by its watermark. Two handles over the same records
(--kinds selects some), run one after the other, --repeats times alternating:
  count     COUNT(*)                                              (the same handle without the distinct aggregate)
  distinct  COUNT(*) + COUNT_DISTINCT(v mod --values) under the flag   (about 1000 values)
Numbers, per timed step (means over the timed steps of a run; every run is printed, so the spread is visible):
  step      push + watermark, host clock around calls that end in a device synchronise
  fire      fwa_stats.fire_ms (HIP events on the handle's stream; for the distinct handle it includes the three passes)
  marking   the distinct handle's fwa_stats.ingest_ms minus the count handle's of the same repeat (the drop mask and
            distinct_mark_session_kernel, HIP events; the ingest itself is the same)
  index     FWA_OPT_DISTINCT_INDEX_US (the sizing pre-pass and dist_sess_index_kernel, HIP events)
  count     FWA_OPT_DISTINCT_COUNT_US (dist_sess_count_kernel and dist_sess_clear_kernel, HIP events)
and the set's slots, live block entries and rebuilds at the end.
Output: python tools/distinct_session_cost.py > profiles/<tag>_distinct_session_cost.txt"""
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
ap.add_argument("--pushes", type=int, default=4)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=2)
ap.add_argument("--batch", type=int, default=1 << 26)
ap.add_argument("--keys", type=int, default=1_000_000)
ap.add_argument("--values", type=int, default=1000)
ap.add_argument("--kinds", default="count,distinct")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("distinct_session_cost.py measures on the GPU: none found")

B, S = args.batch, args.warmup + args.pushes
dev = torch.device("cuda", 0)
p = A.GenParams(seed_k=0x5eed0001, seed_t=0x5eed0002, seed_v=0x5eed0003, first_index=0, total_records=S * B,
                num_keys=args.keys, t0_ms=1_700_000_000_000, span_ms=S * B * 1_000_000 // 1_000_000_000,
                max_delay_ms=1000, key_dist=0, val_kind=0)
keys = torch.empty(S * B, dtype=torch.int64, device=dev)
ts = torch.empty_like(keys)
vals = torch.empty_like(keys)
E.generate(p, S * B, keys, ts, vals)
dcol = torch.remainder(vals, args.values)
del vals
torch.cuda.synchronize()
bmax = ts.view(S, B).max(dim=1).values.cpu().numpy()
wms = np.maximum.accumulate(bmax) - 1001
ingest = {}


def run(kind):
    aggs = [("COUNT", 0)] if kind == "count" else [("COUNT", 0), ("COUNT_DISTINCT", 0)]
    g = E.WindowAggregator(A.make_config(window_kind="SESSION", semantics="TABLE", gap_ms=5_000, aggs=aggs,
                                         key_capacity=args.keys, output_on_device=1, distinct_session=kind != "count"))
    wall, rows, base, paths = 0.0, 0, (0, 0, 0), set()
    for b in range(S):
        sl = slice(b * B, (b + 1) * B)
        if b == args.warmup:
            g.reset_timers()
            if kind != "count":
                base = tuple(g.get_option(n) for n in ("distinct_index_us", "distinct_count_us", "distinct_count_steps"))
        t0 = time.perf_counter()
        g.push(keys[sl], ts[sl], [dcol[sl]])
        n = g.advance_watermark_raw(int(wms[b])).n_rows
        torch.cuda.synchronize()
        paths.add(g.get_option("session_path"))
        if b >= args.warmup:
            wall += time.perf_counter() - t0
            rows += n
    st = g.stats()
    n = args.pushes
    ingest[kind] = st.ingest_ms / n
    line = "%-8s step %8.2f ms; fire %7.2f ms; ingest %7.2f ms; rows/step %d; session paths %s" % (
        kind, wall / n * 1e3, st.fire_ms / n, st.ingest_ms / n, rows // n, sorted(paths))
    if kind != "count":
        now = tuple(g.get_option(x) for x in ("distinct_index_us", "distinct_count_us", "distinct_count_steps"))
        steps = max(1, now[2] - base[2])
        slots = g.get_option("distinct_slots")
        if "count" in ingest:
            line += "; marking %.2f ms per push" % (ingest[kind] - ingest["count"])
        line += "; index %.3f ms, count + clear %.3f ms per step (%d steps); set %d slots (%.2f GB), %d live blocks, %d rebuilds" % (
            (now[0] - base[0]) / 1e3 / steps, (now[1] - base[1]) / 1e3 / steps, steps, slots, slots * 32 / 1e9,
            g.get_option("distinct_live"), g.get_option("distinct_rebuilds"))
    print(line + "; late %d" % st.late_dropped, flush=True)
    g.close()


print("C5s-shaped stream, %d timed pushes of %d records after %d warm-up, %d uniform keys, %d values, Table SESSION gap 5 s"
      % (args.pushes, B, args.warmup, args.keys, args.values), flush=True)
for _ in range(args.repeats):
    for kind in args.kinds.split(","):
        run(kind)
