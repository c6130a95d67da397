#!/bin/bash
# HBM-traffic PMC passes (FETCH_SIZE; WRITE_SIZE, one counter per run) over the C2 bench's wire-input leg
# (bench.py --full). Output under $OUT (default: bench_out/pmcw in the repository).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
R=$PWD
OUT=${OUT:-$R/bench_out/pmcw}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
for ctr in FETCH_SIZE WRITE_SIZE; do
  timeout -s KILL 150 rocprofv3 --pmc $ctr -T -d $OUT/$ctr -o run --output-format csv -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-pcie --wire-batches 3 > $OUT/$ctr.log 2>&1; rc=$?
  echo "$ctr rc=$rc"
  if [ $rc -ne 0 ]; then tail -5 $OUT/$ctr.log; exit $rc; fi
done
exit 0
