#!/bin/sh
# A/B of Lineq::has_solution with is_int_sol = true for a batch (tools/lab/probe_has_solution_int.py states the two sides): 1024
# systems per call, host arrays, is_unique_sol = 1, one warm-up call, median of 5 call times with the spread; the verdicts are
# asserted equal to the CPU checker's first, and the verdict hashes of the two sides must be equal.
#   this tree        xpg_has_solution_int_batch_rat32: objective, both MIP walks and the verdict on the device, one synchronisation
#   the parent       xpg_has_solution_batch_rat32(is_int_sol = 1): two MIP batch calls composed on the host
# on two configurations: "lds" ((5, 2, 5, 1): the LDS-resident walk) and "hbm" (WIDE_HS tiled to 1024: the device-memory walk).
# PARENT names a checkout of the parent commit with its library built (python -m xpoly_amd.build --product there) and the CPU
# checker built in this tree (make -C oracle port). Without PARENT the old side is this tree's own
# xpg_has_solution_batch_rat32(is_int_sol = 1), which this tree leaves as the parent has it.
# One GPU step per line, each under its own time limit, chained with &&: a step that fails ends the run.
# Output: $OUT/has_solution_int_ab.txt (default tools/lab/_out; the kept copy is profiles/has_solution_int_ab.txt).
#   [PARENT=/path/to/parent] sh tools/lab/run_has_solution_int_ab.sh
set -eu
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/../.." && pwd)
OLD=${PARENT:-$ROOT}
OLD=$(cd "$OLD" && pwd)
OUT=${OUT:-$HERE/_out}
mkdir -p "$OUT"
LOG=$OUT/has_solution_int_ab.txt
P=$HERE/probe_has_solution_int.py
: > "$LOG"
echo "# python tools/lab/probe_has_solution_int.py: has_solution(is_int_sol = 1, is_unique_sol = 1), 1024 systems per call, host arrays, warm-up + median of 5" >> "$LOG"
cd "$ROOT" &&
timeout -k 10 120 python "$P" --mode new --config lds --label "this tree: xpg_has_solution_int_batch_rat32" >> "$LOG" 2>&1 &&
timeout -k 10 120 python "$P" --mode old --config lds --root "$OLD" --label "parent: xpg_has_solution_batch_rat32(is_int_sol = 1)" >> "$LOG" 2>&1 &&
timeout -k 10 240 python "$P" --mode new --config hbm --label "this tree: xpg_has_solution_int_batch_rat32" >> "$LOG" 2>&1 &&
timeout -k 10 240 python "$P" --mode old --config hbm --root "$OLD" --label "parent: xpg_has_solution_batch_rat32(is_int_sol = 1)" >> "$LOG" 2>&1 &&
echo "# done" >> "$LOG"
