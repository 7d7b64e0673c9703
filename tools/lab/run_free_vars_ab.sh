#!/bin/sh
# A/B of the free-variable tree walk: probe_free_vars_walk.py on a BASELINE tree (a built checkout of the parent commit,
# first argument) and on this tree, alternating, two turns each, every GPU step under its own time limit; a step that
# fails ends the run. Output: $OUT/free_vars_walk_ab.txt (default tools/lab/_out).
#   sh tools/lab/run_free_vars_ab.sh /path/to/built/parent/tree [reps]
set -eu
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/../.." && pwd)
BASE=${1:?the built tree of the parent commit}
REPS=${2:-20}
OUT=${OUT:-$HERE/_out}
mkdir -p "$OUT"
LOG=$OUT/free_vars_walk_ab.txt
: > "$LOG"
echo "# python tools/lab/probe_free_vars_walk.py --reps $REPS --warmup 3; trees alternate, two turns each" >> "$LOG"
for turn in 1 2; do
    (cd "$BASE" && timeout -k 10 420 python "$HERE/probe_free_vars_walk.py" --reps "$REPS" --label parent) >> "$LOG" 2>&1
    (cd "$ROOT" && timeout -k 10 240 python "$HERE/probe_free_vars_walk.py" --reps "$REPS" --label new) >> "$LOG" 2>&1
done
echo "# done" >> "$LOG"
