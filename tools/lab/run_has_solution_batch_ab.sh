#!/bin/sh
# A/B of the batched Lineq::has_solution (is_int_sol = 0): probe_has_solution_batch.py --mode batch (xpg_has_solution_batch_rat32:
# 1024 systems of (12, 3, 12, 2), LDS-resident, and of (60, 4, 62, 2) under max_iter 48, device memory; one launch each)
# against --mode two_calls (what a caller did before: objectives on the host, xpg_six_batch_vc_hbm_rat32 with is_max = 1, the
# open systems compacted on the host, a second call with is_max = 0).
# One GPU step per line, each under its own time limit, chained with &&: a step that fails ends the run.
# Output: $OUT/has_solution_batch_ab.txt (default tools/lab/_out; the kept copy is profiles/has_solution_batch_ab.txt).
#   sh tools/lab/run_has_solution_batch_ab.sh
set -eu
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/../.." && pwd)
OUT=${OUT:-$HERE/_out}
mkdir -p "$OUT"
LOG=$OUT/has_solution_batch_ab.txt
P=$HERE/probe_has_solution_batch.py
: > "$LOG"
echo "# python tools/lab/probe_has_solution_batch.py: one launch per batch against two xpg_six_batch_vc_hbm_rat32 calls with the objectives and the compaction on the host; host arrays on both sides" >> "$LOG"
cd "$ROOT" &&
timeout -k 10 200 python "$P" --mode batch --label "xpg_has_solution_batch_rat32" >> "$LOG" 2>&1 &&
timeout -k 10 200 python "$P" --mode two_calls --label "two xpg_six_batch_vc_hbm_rat32 calls" >> "$LOG" 2>&1 &&
echo "# done" >> "$LOG"
