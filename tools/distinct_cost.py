"""What COUNT(DISTINCT) costs on the C2 stream (flink_amd/csrc/distinct.inc): the marking pass ahead of the ingest.

Stream: the C2 stream of fwa_generate (2^26 records per push, 1M uniform keys, 1e6 records per second of event time,
bounded out-of-orderness 1 s), Table TUMBLE 10 s, inputs in HBM, one warm-up push then --pushes timed pushes, each
followed by its watermark. Six handles over the same records (--kinds selects some, in the order given; a kind may
be named more than once, which is how alternating runs for a comparison are made):
  base      COUNT + SUM_I64                                      (this build's baseline)
  dup16     COUNT + SUM_I64 + COUNT_DISTINCT, 16 values per key  (duplicates dominate: most probes end at the load)
  unique    COUNT + SUM_I64 + COUNT_DISTINCT, unique 64-bit values (every record inserts: three CASes each)
  dup16sum  dup16 + SUM_DISTINCT_I64 over the same column (FWA_AGG_DISTINCT: the marking pass also writes the value
            column w, one more 8-byte store per record: 72 B + the atomics; the handle then sums three value
            columns, one more than the two-phase ingest carries, so it takes the one-pass ingest and reports its whole
            ingest as "marking")
  cnt16     COUNT + COUNT_DISTINCT, 16 values per key               (one value column: m)
  cnt16sum  cnt16 + SUM_DISTINCT_I64 over the same column           (two value columns, m and w: stays on the two-phase
            ingest, so its marking figure is the 72 B marking pass alone)
Numbers: ms per push of the marking kernel = fwa_stats.ingest_ms - partition_ms - combine_ms (HIP events on the
handle's stream; the handle takes the two-phase ingest, whose two phases are the rest of ingest_ms), the handle's
G rec/s over push + watermark (host clock around calls that end in a synchronise), the set's bytes (32 per slot) and
its rebuilds. Bytes the marking kernel moves per record: reads key 8 + ts 8 + value 8, writes the 0/1 column 8, and
one random 32-byte entry (a probe; a new entry adds three 8-byte CAS round trips) = 64 B + the atomics.
Output: python tools/distinct_cost.py --kinds base,dup16,unique > profiles/<tag>_distinct_cost.txt
        python tools/distinct_cost.py --kinds base,dup16,dup16sum,cnt16,cnt16sum > profiles/<tag>_distinct_sum_cost.txt"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from flink_amd import _abi as A  # noqa: E402
from flink_amd import engine as E  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pushes", type=int, default=8)
ap.add_argument("--batch", type=int, default=1 << 26)
ap.add_argument("--keys", type=int, default=1_000_000)
ap.add_argument("--kinds", default="base,dup16,unique,dup16sum,cnt16,cnt16sum")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("distinct_cost.py measures on the GPU: none found")

B, S = args.batch, args.pushes + 1
dev = torch.device("cuda", 0)
p = A.GenParams(seed_k=0x5eed0001, seed_t=0x5eed0002, seed_v=0x5eed0003, first_index=0, total_records=S * B,
                num_keys=args.keys, t0_ms=1_700_000_000_000, span_ms=S * B * 1_000_000 // 1_000_000_000,
                max_delay_ms=1000, key_dist=0, val_kind=0)
keys = torch.empty(B, dtype=torch.int64, device=dev)
ts = torch.empty_like(keys)
vals = torch.empty_like(keys)
dcol = torch.empty_like(keys)
mix = torch.tensor(-7046029254386353131, dtype=torch.int64, device=dev)   # 0x9E3779B97F4A7C15: odd, so i -> i * mix is 1:1


def batch(b, kind):
    """Batch b of the stream into the buffers; the distinct column: 16 values per key, or a unique value per record."""
    p.first_index = b * B
    E.generate(p, B, keys, ts, vals)
    if kind in ("dup16", "dup16sum", "cnt16", "cnt16sum"):
        torch.bitwise_and(vals, 15, out=dcol)
    elif kind == "unique":
        torch.arange(b * B, (b + 1) * B, dtype=torch.int64, device=dev, out=dcol)
        dcol.mul_(mix)
    torch.cuda.synchronize()
    return int(ts.max().item())


def run(kind):
    aggs = [("COUNT", 0)] + ([] if kind.startswith("cnt16") else [("SUM_I64", 0)])
    aggs += [] if kind == "base" else [("COUNT_DISTINCT", 1)]
    if kind.endswith("sum"):
        aggs.append(("SUM_DISTINCT_I64", 1))
    g = E.WindowAggregator(A.make_config(window_kind="TUMBLE", semantics="TABLE", size_ms=10_000, aggs=aggs,
                                         key_capacity=args.keys, output_on_device=1))
    mx, wall, rows = -2**63, 0.0, 0
    for b in range(S):
        mx = max(mx, batch(b, kind))
        cols = [vals] if kind == "base" else [vals, dcol]
        if b == 1:
            g.reset_timers()
        t0 = time.perf_counter()
        g.push(keys, ts, cols)
        rows += g.advance_watermark_raw(mx - 1001).n_rows
        torch.cuda.synchronize()
        if b >= 1:
            wall += time.perf_counter() - t0
    st = g.stats()
    n = args.pushes
    mark = (st.ingest_ms - st.partition_ms - st.combine_ms) / n
    line = ("%-8s %6.2f G rec/s (push + watermark %.2f ms); ingest %.2f ms/push = partition %.2f + combine %.2f + marking "
            "%.2f" % (kind, n * B / wall / 1e9, wall / n * 1e3, st.ingest_ms / n, st.partition_ms / n, st.combine_ms / n, mark))
    if kind != "base":
        slots = g.get_option("distinct_slots")
        bpr = 72 if kind.endswith("sum") else 64
        line += ("; marking %.1f G rec/s, %.0f GB/s of its %d B/record; set %.2f GB (%d slots), %d rebuilds, %d live at "
                 "the last" % (B / mark / 1e6, bpr * B / mark / 1e6, bpr, slots * 32 / 1e9, slots,
                               g.get_option("distinct_rebuilds"), g.get_option("distinct_live")))
    print(line + "; rows %d, late %d" % (rows, st.late_dropped), flush=True)
    g.close()


print("C2 stream, %d timed pushes of %d records after one warm-up, %d keys, TUMBLE 10 s (Table)" % (args.pushes, B, args.keys),
      flush=True)
for kind in args.kinds.split(","):
    run(kind)
