#!/bin/sh
# A/B of the MIP tree walk beyond 64 KB of LDS: probe_mip_hbm.py --mode hbm (xpg_mip_batch_vc_hbm_*: 1024 trees of 20 variables, 16
# of them free, over 50 inequalities, fp64 and Rational, both directions, one launch each) against --mode host
# (xpg_mip_batch_vc_* on the same arrays, which walks such trees with the host controller: the only route they had before).
# One GPU step per line, each under its own time limit, chained with &&: a step that fails ends the run.
# Output: $OUT/mip_hbm_ab.txt (default tools/lab/_out; the kept copy is profiles/mip_hbm_ab.txt).
#   sh tools/lab/run_mip_hbm_ab.sh [nb]
set -eu
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/../.." && pwd)
NB=${1:-1024}
OUT=${OUT:-$HERE/_out}
mkdir -p "$OUT"
LOG=$OUT/mip_hbm_ab.txt
P=$HERE/probe_mip_hbm.py
: > "$LOG"
echo "# python tools/lab/probe_mip_hbm.py: one launch per batch against the host controller, host arrays on both sides, $NB trees" >> "$LOG"
cd "$ROOT" &&
timeout -k 10 200 python "$P" --mode hbm --kinds 0 --nb "$NB" --label "xpg_mip_batch_vc_hbm_f64" >> "$LOG" 2>&1 &&
timeout -k 10 200 python "$P" --mode hbm --kinds 1 --nb "$NB" --label "xpg_mip_batch_vc_hbm_rat32" >> "$LOG" 2>&1 &&
timeout -k 10 300 python "$P" --mode host --kinds 0 --nb "$NB" --label "xpg_mip_batch_vc_f64: host controller" >> "$LOG" 2>&1 &&
timeout -k 10 300 python "$P" --mode host --kinds 1 --nb "$NB" --label "xpg_mip_batch_vc_rat32: host controller" >> "$LOG" 2>&1 &&
echo "# done" >> "$LOG"
