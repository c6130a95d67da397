#!/bin/bash
# Wire decoder: parity tests, bench C2 line with the wire_input leg (bench.py --full), rocprofv3 kernel stats of the
# same bench. Logs under $OUT (default: bench_out/ in the repository).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
R=$PWD
OUT=${OUT:-$R/bench_out}
mkdir -p $OUT
TAG=${TAG:-wire}
BENCH_ARGS="--full --no-cpu-baseline --no-pcie --steps 4"
timeout -k 10 300 python -u -m pytest tests/test_wire_gpu.py -x -q --timeout 120 --timeout-method thread > $OUT/wtest_$TAG.log 2>&1 || { tail -30 $OUT/wtest_$TAG.log; exit 1; }
tail -2 $OUT/wtest_$TAG.log
timeout -k 10 300 python -u bench.py $BENCH_ARGS > $OUT/wbench_$TAG.log 2>&1 || { tail -20 $OUT/wbench_$TAG.log; exit 1; }
grep '^{' $OUT/wbench_$TAG.log | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print(json.dumps(d['wire_input']))"
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/wprof_$TAG -o run --output-format csv -- python3 $R/bench.py $BENCH_ARGS > $OUT/wprof_$TAG.log 2>&1 || { tail -5 $OUT/wprof_$TAG.log; exit 1; }
f=$(find $OUT/wprof_$TAG -name "*kernel_stats.csv" | head -1); grep -i wire "$f" | cut -d, -f1-4
