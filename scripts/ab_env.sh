#!/bin/bash
# A/B of environment settings on the driver's bench command (timed frames only), alternated.
#   scripts/ab_env.sh STEPS REPS "" "VAR=1" ...
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}" || exit 1
steps=$1; reps=$2; shift 2
log=$(mktemp) && trap 'rm -f "$log"' EXIT
for r in $(seq $reps); do
  for v in "$@"; do
    env $v timeout -k 10 120 python3 -u bench.py --full --steps $steps --warmup 5 --timed-only > "$log" 2>&1 || { echo "run failed: $v"; tail -5 "$log"; exit 1; }
    tail -n 1 "$log" | python3 -c "import sys,json; d=json.loads(sys.stdin.read()); print('${v:-default}', d['value'], d['ms_per_step'], d['verified']['frames'])"
  done
done
