#!/bin/bash
# A/B of xpg_lineq_levels_batch_packed_rat32 against one xpg_lineq_fme_batch_packed_rat32 call per level
# (tools/lab/probe_lineq_levels.py): nests of depth 3, 4 and 6 at nb = 1, 1024 and 16 384, one device process at a time, each
# under its own time limit, the chain ends at the first step that fails. OUT defaults to tools/lab/_out.
set -o pipefail
cd "$(dirname "$0")/../.."
OUT=${OUT:-tools/lab/_out}
mkdir -p "$OUT"
F="$OUT/lineq_levels_ab.txt"
: > "$F"
run() { timeout -k 10 "$1" python tools/lab/probe_lineq_levels.py "$2" "$3" 2>&1 | tee -a "$F"; }
run 60 3 1 && run 60 4 1 && run 60 6 1 &&
run 90 3 1024 && run 90 4 1024 && run 90 6 1024 &&
run 240 3 16384 && run 240 4 16384 && run 240 6 16384
