#!/bin/bash
# graph-construction tests + the full GPU suite + the full bench (development check);
# results land in $OUT (default bench_out/)
set -o pipefail
export TMPDIR=/tmp
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 300 python -u -m pytest tests/test_graphs.py -m gpu -x -v --timeout 120 --timeout-method thread > $OUT/graphs_tests.log 2>&1 || { tail -40 $OUT/graphs_tests.log; exit 1; }
tail -3 $OUT/graphs_tests.log
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > $OUT/gpu_tests.log 2>&1 || { tail -30 $OUT/gpu_tests.log; exit 1; }
tail -2 $OUT/gpu_tests.log
timeout -k 10 300 python bench.py --full --steps 5 --warmup 1 --cpu-pairs 8 > $OUT/bench.json 2> $OUT/bench.err || { tail -20 $OUT/bench.err; exit 1; }
cat $OUT/bench.json; grep "step:" $OUT/bench.err | tail -3
