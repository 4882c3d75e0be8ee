#!/bin/bash
# Interleaved A/B of the default C3 forward under environment variants, separate processes:
#   TAG=r05q REPS=3 [SHARE=1] bash tools/ab_env.sh "" "FPM_CHUNKS=16" ...
# ("" = the defaults).  Each variant runs REPS times, round-robin; prints value and GPU-stage rate
# (and with SHARE=1 the 128-pair share line's value).
set -o pipefail
export TMPDIR=/tmp
cd "$GRAFT_REPO_ROOT"; mkdir -p gpurun_out
tag=${TAG:-ab}
reps=${REPS:-3}
SL="--no-share-line"; [ "${SHARE:-0}" = 1 ] && SL="--full"      # the share line is one of --full's extras
B="--no-config-lines --no-cpu-baseline --no-f32-line $SL --no-selfcheck --steps 10 $BENCH_ARGS"
for i in $(seq 1 $reps); do
  v=0
  for envs in "$@"; do
    env $envs timeout -k 10 200 python bench.py $B > gpurun_out/${tag}_v${v}_$i.json 2> gpurun_out/${tag}_v${v}_$i.err || exit 1
    v=$((v + 1))
  done
done
python - "$@" <<'PY'
import json, os, sys
tag = os.environ.get("TAG", "ab"); reps = int(os.environ.get("REPS", "3"))
for v, envs in enumerate(sys.argv[1:]):
    rows = []
    for i in range(1, reps + 1):
        d = json.load(open("gpurun_out/%s_v%d_%d.json" % (tag, v, i)))
        sh = d.get("share128_line") or {}
        rows.append((round(d["value"]), round(d.get("gpu_stage_pairs_per_s", 0))) + ((round(sh["value"]),) if sh else ()))
    print("%-40s %s" % (envs or "(defaults)", rows))
PY
