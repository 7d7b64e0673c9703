#!/bin/sh
# A/B of the batched LPs with equalities and free variables beyond 64 KB of LDS: probe_six_batch_vc_hbm.py --mode batch
# (xpg_six_batch_vc_hbm_*: 1024 LPs of (60, 4, 62, 2) and of (96, 4, 103, 2), fp64 under max_iter 300 and Rational under 48,
# one launch each) against --mode loop (xpg_six_batch_vc_*, which solves such shapes with one single call per problem: the
# only route they had before; first argument: how many LPs the loop times, default 128).
# One GPU step per line, each under its own time limit, chained with &&: a step that fails ends the run.
# Output: $OUT/six_batch_vc_hbm_ab.txt (default tools/lab/_out; the kept copy is profiles/six_batch_vc_hbm_ab.txt).
#   sh tools/lab/run_six_batch_vc_hbm_ab.sh [loop-count]
set -eu
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/../.." && pwd)
LOOPN=${1:-128}
OUT=${OUT:-$HERE/_out}
mkdir -p "$OUT"
LOG=$OUT/six_batch_vc_hbm_ab.txt
P=$HERE/probe_six_batch_vc_hbm.py
: > "$LOG"
echo "# python tools/lab/probe_six_batch_vc_hbm.py: one launch per batch against the loop of single calls, host arrays on both sides" >> "$LOG"
cd "$ROOT" &&
timeout -k 10 300 python "$P" --mode batch --kinds 0 --label "xpg_six_batch_vc_hbm_f64" >> "$LOG" 2>&1 &&
timeout -k 10 300 python "$P" --mode batch --kinds 1 --label "xpg_six_batch_vc_hbm_rat32" >> "$LOG" 2>&1 &&
timeout -k 10 400 python "$P" --mode loop --kinds 0 --loop-count "$LOOPN" --label "xpg_six_batch_vc_f64: one single call per problem" >> "$LOG" 2>&1 &&
timeout -k 10 400 python "$P" --mode loop --kinds 1 --loop-count "$LOOPN" --label "xpg_six_batch_vc_rat32: one single call per problem" >> "$LOG" 2>&1 &&
echo "# done" >> "$LOG"
