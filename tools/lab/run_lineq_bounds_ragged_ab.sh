#!/bin/bash
# A/B of xpg_lineq_bounds_batch_ragged_rat32 against one uniform call per shape class (tools/lab/probe_lineq_bounds_ragged.py):
# a mixed SCoP of 20 shape classes at 64, 692 and 16 384 systems, a batch of one class, then one 60 x 20 nest among 1000 of
# 6 x 5. One device process at a time, each under its own time limit, the chain ends at the first step that fails; the probes
# are single-threaded on the host. OUT defaults to tools/lab/_out; the result is kept as profiles/lineq_bounds_ragged_ab.txt.
set -o pipefail
cd "$(dirname "$0")/../.."
OUT=${OUT:-tools/lab/_out}
mkdir -p "$OUT"
F="$OUT/lineq_bounds_ragged_ab.txt"
: > "$F"
run() { timeout -k 10 "$1" python tools/lab/probe_lineq_bounds_ragged.py "$2" 2>&1 | tee -a "$F"; }
run 90 64 && run 120 692 && run 300 16384 && run 120 one && run 180 wide
