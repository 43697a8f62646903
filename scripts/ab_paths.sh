#!/bin/bash
# A/B of (library, environment) pairs on one box: scripts/ab_paths.sh <reps> "<lib path relative to the repo root> [VAR=value ...]" ...
# EMAT_AB_JSON=<file>: every run's whole result line is appended to it (check.log_G, check.parts_stopped, the roofline's byte counts).
# Every run has a time limit of its own (EMAT_AB_TIMEOUT seconds, default 300), and the first run that fails ends the script: nothing more
# is started on a device after a fault.
set -o pipefail
cd "$(dirname "$0")/.."
REPS=$1; shift
SPECS=("$@")
for r in $(seq $REPS); do
  for spec in "${SPECS[@]}"; do
    words=($spec); lib=${words[0]}
    env "${words[@]:1}" EMAT_LIB_PATH=$PWD/$lib EMAT_ALLOW_STALE_LIB=1 timeout -k 10 ${EMAT_AB_TIMEOUT:-300} python bench.py --full --no-cpu-baseline --no-inclusive --no-decompositions --secondary '' --steps 10 $EMAT_AB_ARGS 2>/dev/null | python3 -c "
import sys, json, os
line = sys.stdin.readline(); d = json.loads(line)
if os.environ.get('EMAT_AB_JSON'): open(os.environ['EMAT_AB_JSON'], 'a').write(json.dumps({'spec': '$spec', 'rep': $r}) + ' ' + line)
print('$spec', '| rep $r', round(d['value'] / 1e6, 1), 'M moves/s', round(d['ms_per_step'], 2), 'ms/step kernel', round(d['roofline']['kernel_ms'], 2))" || { echo "$spec | rep $r: the run failed; stopping" >&2; exit 1; }
  done
done
