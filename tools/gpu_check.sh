#!/bin/bash
# parity tests, the full bench, single-stream kernel profile (used during development);
# results land in $OUT (default bench_out/)
set -o pipefail
export TMPDIR=/tmp
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 600 python -m pytest tests -m gpu -x -q > $OUT/gpu_tests.log 2>&1 || { tail -30 $OUT/gpu_tests.log; exit 1; }
tail -2 $OUT/gpu_tests.log
timeout -k 10 300 python bench.py --full --steps 5 --warmup 1 --cpu-pairs 8 > $OUT/bench.json 2> $OUT/bench.err || { tail -20 $OUT/bench.err; exit 1; }
cat $OUT/bench.json; grep "step:" $OUT/bench.err
if [ "$1" = "prof" ]; then
  FPM_STREAMS=1 timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_1s -o run --output-format csv -- python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $OUT/prof_1s.log 2>&1 || exit 1
fi
