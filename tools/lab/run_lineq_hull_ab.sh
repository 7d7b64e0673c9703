#!/bin/bash
# A/B of xpg_lineq_hull_batch_ragged_rat32 against the two calls it replaces composed on the host (tools/lab/probe_lineq_hull.py):
# the mixed SCoP of 20 shape classes at 64, 692 and 16 384 members, grouped into hulls of 2, 8 and 32 members, and groups of ONE
# member, where the one call has nothing to save but the second upload. One device process at a time, each under its own time
# limit, the chain ends at the first step that fails; the probes are single-threaded on the host. OUT defaults to
# tools/lab/_out; the result is kept as profiles/lineq_hull_ab.txt.
set -o pipefail
cd "$(dirname "$0")/../.."
OUT=${OUT:-tools/lab/_out}
mkdir -p "$OUT"
F="$OUT/lineq_hull_ab.txt"
: > "$F"
run() { timeout -k 10 "$1" python tools/lab/probe_lineq_hull.py "$2" "$3" 2>&1 | tee -a "$F"; }
run 90 64 2 && run 90 64 8 && run 90 64 32 && run 120 692 2 && run 120 692 8 && run 120 692 32 &&
    run 300 16384 2 && run 300 16384 8 && run 300 16384 32 && run 120 692 1
