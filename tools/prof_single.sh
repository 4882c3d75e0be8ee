#!/bin/bash
# full bench (graph-build field) + single-stream kernel-trace stats (true per-kernel durations);
# results land in $OUT (default bench_out/)
set -o pipefail
export TMPDIR=/tmp
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 300 python bench.py --full --steps 5 --warmup 1 --cpu-pairs 4 > $OUT/bench.json 2> $OUT/bench.err || { tail -20 $OUT/bench.err; exit 1; }
cat $OUT/bench.json; grep "graph build\|step:" $OUT/bench.err | tail -3
FPM_STREAMS=1 timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_1s -o run --output-format csv -- python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $OUT/prof_1s.log 2>&1 || { tail -20 $OUT/prof_1s.log; exit 1; }
find $OUT/prof_1s -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $OUT/prof_1s_kernel_stats.csv
echo done
