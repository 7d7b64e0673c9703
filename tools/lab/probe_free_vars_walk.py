"""Times the calls whose trees have free variables: dep_is_empty_batch_symbols_as_vars at (3,2,9) and (4,1,12) with 512 and
4096 polyhedra per call, and the (4,5,2) integer programs of tests/free_var_cases.py at 4096 problems through mip_batch_vc
(a tree that lacks it -- the A/B baseline -- walks the same problems with one MIP.maxm call each: said in the output).
Warm-up, then the median of --reps calls by the host clock; every call ends in a device synchronise inside the library.
One JSON line per leg. The tree under test is the current directory (run_free_vars_ab.sh alternates two trees)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))

import numpy as np  # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="tree")
    a = ap.parse_args()
    import xpoly_amd
    from xpoly_amd import six
    import free_var_cases as fc
    from tools import gen
    ctx = xpoly_amd.Context(0)
    route = getattr(six, "mip_last_route", None)
    for nv, ns, rows in ((3, 2, 9), (4, 1, 12)):
        rng = np.random.default_rng(4242)
        mats = np.stack([gen.random_system(rng, rows, nv + ns) for _ in range(4096)])
        mats[..., 1] = 1
        for nb in (512, 4096):
            m = np.ascontiguousarray(mats[:nb])
            med, lo, hi = timed(lambda: six.dep_is_empty_batch_symbols_as_vars(ctx, m, nv), a.warmup, a.reps)
            print(json.dumps(dict(tree=a.label, leg="dep_symbols_as_vars", shape=[nv, ns, rows], per_call=nb, median_ms=round(med * 1e3, 3),
                                  min_ms=round(lo * 1e3, 3), max_ms=round(hi * 1e3, 3), per_s=round(nb / med), route=route() if route else None)), flush=True)
    shape = (4, 5, 2)
    probs = fc.shape_problems(shape, 4096)
    free = probs[0]["free"]
    for p in probs:                                              # one free set for the whole batch: vc is shared by a call
        lead = p["leq"][:5 + 2]
        p["free"] = free
        lead[5:7] = 0
        for k, j in enumerate(free):
            lead[5 + k, j] = -1; lead[5 + k, 5] = 6
    tg, vc, leq = fc.batch_arrays(probs, list(range(4096)), fc.RAT)
    if hasattr(six, "mip_batch_vc"):
        med, lo, hi = timed(lambda: six.mip_batch_vc(ctx, True, False, tg, vc, leq), a.warmup, a.reps)
        how, nb = "mip_batch_vc, one call", 4096
    else:
        mip, nb = six.MIP(ctx, fc.RAT), 256
        def loop():
            for b in range(nb):
                mip.maxm(tg[b], vc, None, leq[b])
        med, lo, hi = timed(loop, 1, max(3, a.reps // 4))
        how = "a loop of %d MIP.maxm calls (this tree has no mip_batch_vc)" % nb
    print(json.dumps(dict(tree=a.label, leg="mip_free_vars", shape=list(shape), per_call=nb, how=how, median_ms=round(med * 1e3, 3),
                          min_ms=round(lo * 1e3, 3), max_ms=round(hi * 1e3, 3), per_s=round(nb / med), route=route() if route else None)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
