"""Call times of Lineq::has_solution(is_int_sol = true) for 1024 systems per call, host arrays, is_unique_sol = 1 (run by
tools/lab/run_has_solution_int_ab.sh):
  --mode new   xpg_has_solution_int_batch_rat32: objective, both walks and the verdict on the device, one synchronisation
  --mode old   xpg_has_solution_batch_rat32(is_int_sol = 1): two MIP batch calls composed on the host
Configurations: "lds" -- has_solution_cases.small_arrays((5, 2, 5, 1)), the LDS-resident walk; "hbm" -- has_solution_int_cases'
WIDE_HS tiled, the device-memory walk. --root names the checkout whose package and library are measured (default: this tree;
the parent commit's for the old side); the systems always come from this tree's tests/. The verdicts are asserted equal to the
CPU checker's for the distinct systems before anything is timed; one warm-up call, then the median of 5 with the spread."""
import argparse
import hashlib
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("new", "old"), required=True)
ap.add_argument("--config", choices=("lds", "hbm"), required=True)
ap.add_argument("--root", default=ROOT)
ap.add_argument("--nb", type=int, default=1024)
ap.add_argument("--label", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.abspath(args.root))
sys.path.append(ROOT)                                            # the CPU checker is this tree's whatever --root says

import numpy as np

import has_solution_cases as hs
import has_solution_int_cases as hi
import xpoly_amd
from xpoly_amd import six

if args.config == "lds":
    distinct = 64
    arrays = hs.small_arrays((5, 2, 5, 1), distinct)
    want = hs.int_answers(("small", (5, 2, 5, 1)), arrays, distinct)
else:
    distinct = hi.WIDE_COUNT
    arrays = hi.wide_hs()
    want = hs.int_answers(("wide",), arrays, distinct)
vc_arr, eq, leq = hi.pick(arrays, np.arange(args.nb) % distinct)
ctx = xpoly_amd.Context(0)


def call():
    if args.mode == "new":
        return six.has_solution_int_batch(ctx, leq, eq, vc_arr, True)
    return six.has_solution_batch(ctx, leq, eq, vc_arr, True, True)


has = call()                                                     # the warm-up call
assert [int(h) for h in has[:distinct]] == [w[1] for w in want], "verdicts differ from the CPU checker's"
assert all(np.array_equal(has[k:k + distinct], has[:min(distinct, args.nb - k)]) for k in range(0, args.nb, distinct))
times = []
for _ in range(5):
    t0 = time.perf_counter()
    call()
    times.append((time.perf_counter() - t0) * 1e3)
times.sort()
route = six.has_solution_int_last_route() if args.mode == "new" else six.has_solution_batch_last_route()
print("%-58s %-4s nb %d  median %8.3f ms  min %8.3f  max %8.3f  verdicts %s  route %s" % (
    args.label or args.mode, args.config, args.nb, times[2], times[0], times[4], hashlib.sha256(has.tobytes()).hexdigest()[:12], route))
ctx.close()
