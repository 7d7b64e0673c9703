#!/bin/sh
# A/B of a projection (tools/lab/probe_lineq_project.py states the sides): the ONE call xpg_lineq_project_batch_packed_rat32
# against what a caller can do without it -- one xpg_lineq_fme_batch_ragged_rat32 call per variable, or one
# xpg_lineq_fme_batch_packed_rat32 call per variable with the intermediates padded on the host. Shapes 16 x 9 eliminating the
# last 2 and the last 4 variables and 40 x 13 eliminating the last 2, at 1024 and 16 384 systems per call (cap_rows 1024; the
# systems are the first 64 of 4096 candidates whose every step fits it). The sides that run must be bit-identical before
# anything is timed; a side the package refuses at a shape is printed as not run. One warm-up, then 5 rounds in which the
# sides alternate: median, min, max, and the device memory of each form.
# One GPU step per line, each under its own time limit, chained with &&: a step that fails ends the run.
# Output: $OUT/lineq_project_ab.txt (default tools/lab/_out; the kept copy is profiles/lineq_project_ab.txt).
#   sh tools/lab/run_lineq_project_ab.sh
set -eu
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/../.." && pwd)
OUT=${OUT:-$HERE/_out}
mkdir -p "$OUT"
LOG=$OUT/lineq_project_ab.txt
P=$HERE/probe_lineq_project.py
: > "$LOG"
echo "# python tools/lab/probe_lineq_project.py: host arrays in, packed rows out, warm-up + 5 alternating rounds, times in ms" >> "$LOG"
cd "$ROOT" &&
timeout -k 10 120 python "$P" --rows 16 --cols 9 --last 2 --nb 1024 >> "$LOG" 2>&1 &&
timeout -k 10 180 python "$P" --rows 16 --cols 9 --last 2 --nb 16384 >> "$LOG" 2>&1 &&
timeout -k 10 120 python "$P" --rows 40 --cols 13 --last 2 --nb 1024 >> "$LOG" 2>&1 &&
timeout -k 10 240 python "$P" --rows 40 --cols 13 --last 2 --nb 16384 >> "$LOG" 2>&1 &&
timeout -k 10 120 python "$P" --rows 16 --cols 9 --last 4 --nb 1024 >> "$LOG" 2>&1 &&
timeout -k 10 300 python "$P" --rows 16 --cols 9 --last 4 --nb 16384 >> "$LOG" 2>&1 &&
echo "# done" >> "$LOG"
