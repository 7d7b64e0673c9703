#!/bin/sh
# A/B of Lineq::calcBound for batches (tools/lab/probe_calc_bound.py states the sides): the fused call
# xpg_lineq_bounds_batch_packed_rat32 -- one launch, the chains' shared prefixes walked once -- against
# xpg_lineq_calc_bound_batch_packed_rat32, which runs every chain as a string of k_fme_batch launches. Triangular loop nests of
# depth 3, 4 and 6 (2 * depth rows) at 1, 1024 and 16 384 systems per call, the default capacity. The sides must be
# bit-identical before anything is timed. One warm-up, then 5 rounds in which the sides alternate: median, min, max, and the
# device memory of each form.
# One GPU step per line, each under its own time limit, chained with &&: a step that fails ends the run.
# Output: $OUT/calc_bound_ab.txt (default tools/lab/_out; the kept copy is profiles/calc_bound_ab.txt).
#   sh tools/lab/run_calc_bound_ab.sh
set -eu
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/../.." && pwd)
OUT=${OUT:-$HERE/_out}
mkdir -p "$OUT"
LOG=$OUT/calc_bound_ab.txt
P=$HERE/probe_calc_bound.py
: > "$LOG"
echo "# python tools/lab/probe_calc_bound.py: host arrays in, packed rows out, warm-up + 5 alternating rounds, times in ms" >> "$LOG"
cd "$ROOT" &&
timeout -k 10 60 python "$P" --depth 3 --nb 1 >> "$LOG" 2>&1 &&
timeout -k 10 60 python "$P" --depth 3 --nb 1024 >> "$LOG" 2>&1 &&
timeout -k 10 90 python "$P" --depth 3 --nb 16384 >> "$LOG" 2>&1 &&
timeout -k 10 60 python "$P" --depth 4 --nb 1 >> "$LOG" 2>&1 &&
timeout -k 10 60 python "$P" --depth 4 --nb 1024 >> "$LOG" 2>&1 &&
timeout -k 10 90 python "$P" --depth 4 --nb 16384 >> "$LOG" 2>&1 &&
timeout -k 10 60 python "$P" --depth 6 --nb 1 >> "$LOG" 2>&1 &&
timeout -k 10 60 python "$P" --depth 6 --nb 1024 >> "$LOG" 2>&1 &&
timeout -k 10 120 python "$P" --depth 6 --nb 16384 >> "$LOG" 2>&1 &&
echo "# done" >> "$LOG"
