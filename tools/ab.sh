#!/bin/bash
# GPU tests, then the full bench alternating an env switch: VAR=FPM_GNN_PACKED bash tools/ab.sh [a] [b]
# (results land in $OUT, default bench_out/)
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
mkdir -p $OUT
V=${VAR:-FPM_GEMM_PHASE}; A=${1:-1}; Bv=${2:-0}
if [ -z "$NOTEST" ]; then
  timeout -k 10 600 python -m pytest tests -m gpu -x -q > $OUT/gpu_tests.log 2>&1 || { tail -30 $OUT/gpu_tests.log; exit 1; }
  tail -2 $OUT/gpu_tests.log
fi
for z in $A $Bv $A $Bv; do
  env $V=$z timeout -k 10 200 python bench.py --full --steps 8 --warmup 2 --no-cpu-baseline > $OUT/ab$z.json 2> $OUT/ab$z.err || { tail $OUT/ab$z.err; exit 1; }
  python -c "
import json; d=json.load(open('$OUT/ab$z.json')); r=d['roofline']
print('$V=$z', round(d['value']), 'gpu-stage', round(d['gpu_stage_pairs_per_s']), 'lsa_ms', round(d['host_lsa_ms_per_step'],1), 'gemm', round(r['achieved']), round(r['isolated_achieved']))"
done
