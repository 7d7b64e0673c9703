#!/bin/sh
# A/B of the batched LPs beyond one CU's LDS: probe_batch_hbm.py --mode batch on this tree (xpg_six_batch_hbm_f64_dev, 1024
# fp64 LPs at 100 x 100 and 256 x 256, max_iter 2000) in every thread-count / waves-per-CU variant, and --mode loop on a
# BUILT tree of the parent commit (first argument): the loop of xpg_six_maxm_f64 single calls, the only route those LPs had.
# One GPU step per line, each under its own time limit, chained with &&: a step that fails ends the run.
# Output: $OUT/batch_hbm_ab.txt (default tools/lab/_out; the kept copy is profiles/batch_hbm_ab.txt).
#   sh tools/lab/run_batch_hbm_ab.sh /path/to/built/parent/tree [loop-count]
set -eu
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/../.." && pwd)
BASE=${1:?the built tree of the parent commit}
LOOPN=${2:-1024}
OUT=${OUT:-$HERE/_out}
mkdir -p "$OUT"
LOG=$OUT/batch_hbm_ab.txt
HOOKS=$ROOT/xpoly_amd/libxpoly_amd_hooks.so
P=$HERE/probe_batch_hbm.py
: > "$LOG"
echo "# python tools/lab/probe_batch_hbm.py: batch on this tree (variants through the hooks build), loop of single calls on the parent tree" >> "$LOG"
cd "$ROOT" &&
timeout -k 10 240 python "$P" --mode batch --label "product build (the variant kept)" >> "$LOG" 2>&1 &&
XPG_SO_PATH=$HOOKS XPG_BATCH_HBM_THREADS=256 XPG_BATCH_HBM_WAVES=16 timeout -k 10 240 python "$P" --mode batch --label "256 threads, 4 workgroups per CU" >> "$LOG" 2>&1 &&
XPG_SO_PATH=$HOOKS XPG_BATCH_HBM_THREADS=256 XPG_BATCH_HBM_WAVES=8 timeout -k 10 240 python "$P" --mode batch --label "256 threads, 2 workgroups per CU" >> "$LOG" 2>&1 &&
XPG_SO_PATH=$HOOKS XPG_BATCH_HBM_THREADS=512 XPG_BATCH_HBM_WAVES=16 timeout -k 10 240 python "$P" --mode batch --label "512 threads, 2 workgroups per CU" >> "$LOG" 2>&1 &&
XPG_SO_PATH=$HOOKS XPG_BATCH_HBM_THREADS=512 XPG_BATCH_HBM_WAVES=8 timeout -k 10 240 python "$P" --mode batch --label "512 threads, 1 workgroup per CU" >> "$LOG" 2>&1 &&
XPG_SO_PATH=$HOOKS XPG_BATCH_HBM_THREADS=1024 XPG_BATCH_HBM_WAVES=16 timeout -k 10 240 python "$P" --mode batch --label "1024 threads, 1 workgroup per CU" >> "$LOG" 2>&1 &&
cd "$BASE" &&
timeout -k 10 900 python "$P" --mode loop --loop-count "$LOOPN" --label "parent commit: loop of xpg_six_maxm_f64" >> "$LOG" 2>&1 &&
echo "# done" >> "$LOG"
