#!/bin/sh
# A/B of xpoly_amd::has_solution_all on two SCoP-like mixes (tools/lab/probe_has_solution_all.cpp states them: 20 shape classes of
# 8..64 systems under one vc -- "small": 10 variables, all LDS-resident, solves of microseconds; "large": 24 variables, two classes
# past 64 KB of LDS, solves of seconds; host arrays; one warm-up call, median of 5). MIXES picks them (default: both; "large"
# takes about 12 minutes of GPU time in all):
#   this tree's collector and library    ONE xpg_has_solution_batch_ragged_rat32 call, one launch per kernel
#   the parent commit's                  one xpg_has_solution_batch_rat32 call per shape class
#   this tree's on the test-hooks build  the index lists sorted (longest solves first), then in arrival order
#                                        (XPG_HS_RAGGED_ARRIVAL=1) -- the effect of the order, which nobody has measured before
# PARENT names a checkout of the parent commit with its library built (python -m xpoly_amd.build --product there); it is
# needed for its headers and its libxpoly_amd.so alone. The verdict hashes of all four lines must be equal.
# One GPU step per line, each under its own time limit, chained with &&: a step that fails ends the run.
# Output: $OUT/has_solution_ragged_ab.txt (default tools/lab/_out; the kept copy is profiles/has_solution_ragged_ab.txt).
#   PARENT=/path/to/parent [MIXES=small] sh tools/lab/run_has_solution_ragged_ab.sh
set -eu
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/../.." && pwd)
PARENT=$(cd "${PARENT:?PARENT: a checkout of the parent commit with its library built}" && pwd)
OUT=${OUT:-$HERE/_out}
mkdir -p "$OUT"
LOG=$OUT/has_solution_ragged_ab.txt
SRC=$HERE/probe_has_solution_all.cpp
CXX="g++ -std=c++17 -O2 -Wall -Wextra"
$CXX -DPROBE_RAGGED -I "$ROOT/include" "$SRC" -o "$OUT/probe_hs_all_this" -L "$ROOT/xpoly_amd" -lxpoly_amd -lpthread "-Wl,-rpath,$ROOT/xpoly_amd"
$CXX -DPROBE_RAGGED -I "$ROOT/include" "$SRC" -o "$OUT/probe_hs_all_hooks" -L "$ROOT/xpoly_amd" -l:libxpoly_amd_hooks.so -lpthread "-Wl,-rpath,$ROOT/xpoly_amd"
$CXX -I "$PARENT/include" "$SRC" -o "$OUT/probe_hs_all_parent" -L "$PARENT/xpoly_amd" -lxpoly_amd -lpthread "-Wl,-rpath,$PARENT/xpoly_amd"
: > "$LOG"
echo "# tools/lab/probe_has_solution_all.cpp: one has_solution_all call on 20 shape classes under one vc; this tree (one ragged call) against the parent commit (one call per class); then the index lists sorted against arrival order on the test-hooks build" >> "$LOG"
cd "$ROOT"
for MIX in ${MIXES:-small large}; do
timeout -k 10 300 "$OUT/probe_hs_all_this" "this tree: one ragged call" "$MIX" >> "$LOG" 2>&1 &&
timeout -k 10 300 "$OUT/probe_hs_all_parent" "parent commit: one call per shape class" "$MIX" >> "$LOG" 2>&1 &&
timeout -k 10 300 "$OUT/probe_hs_all_hooks" "hooks build, index lists sorted" "$MIX" >> "$LOG" 2>&1 &&
XPG_HS_RAGGED_ARRIVAL=1 timeout -k 10 300 "$OUT/probe_hs_all_hooks" "hooks build, index lists in arrival order" "$MIX" >> "$LOG" 2>&1 || exit $?
done
echo "# done" >> "$LOG"
