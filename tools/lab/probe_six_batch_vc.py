"""Times six_batch_vc -- LPs with equalities and free variables, reshaped and solved on the device in one launch -- against
the only route such LPs had: a loop of SIX.maxm over the same problems (host reshaping, a launch of one LP and a
synchronise per call). Shapes: the (5,2,5,1) LPs of tests/six_eq_cases.py, and a dependence-test-like system of 32
inequalities over 63 variables (gen.small_lp_batch_f64 family 1) with 2 sparse equalities and its first two variables free.
nb = 64, 1024 and 4096 per call, both kinds, max_iter 10000 on both sides. The batch: warm-up, then the median of --reps
calls by the host clock (every call ends in a device synchronise inside the library). The loop: the median of 3 passes at
nb = 64, one pass at the larger sizes (its time per LP does not depend on nb). Answers of the two are compared on the way.
One JSON line per leg."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))

import numpy as np  # noqa: E402

MAX_ITER = 10000


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def dep_like(nb, kind):
    """(tgtf, vc, eq, leq): 32 x 64 dependence-test-like inequalities, 2 equalities x_a - x_b = d, x_0 and x_1 free."""
    from tools import gen
    leq, tg = gen.small_lp_batch_f64(nb, 32, 64, family=1)
    rng = np.random.default_rng(3264)
    eq = np.zeros((nb, 2, 64))
    for b in range(nb):
        for r in range(2):
            a, c = rng.choice(63, 2, replace=False)
            eq[b, r, a] = 1; eq[b, r, c] = -1; eq[b, r, 63] = rng.integers(0, 4)
    vc = gen.vc_nonneg(63, True, (0, 1))
    if kind == 0:
        return tg, vc, eq, leq
    return tuple(gen.to_rat(x.astype(np.int32)) for x in (tg, vc, eq, leq))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="64,1024,4096")
    a = ap.parse_args()
    import xpoly_amd
    from xpoly_amd import six
    import six_eq_cases as sc
    ctx = xpoly_amd.Context(0)
    sizes = [int(x) for x in a.sizes.split(",")]
    for name in ("(5,2,5,1)", "32x64 dependence-like, 2 equalities, 2 free"):
        for kind in (six.RAT, six.F64):
            if name.startswith("("):
                tg0, vc, eq0, leq0 = sc.shape_arrays((5, 2, 5, 1), kind)
                idx = np.arange(max(sizes)) % sc.PER_SHAPE
                tg0, eq0, leq0 = tg0[idx], eq0[idx], leq0[idx]
            else:
                tg0, vc, eq0, leq0 = dep_like(max(sizes), kind)
            solver = six.SIX(ctx, kind)
            solver.set_param(0, MAX_ITER)
            for nb in sizes:
                tg, eq, leq = (np.ascontiguousarray(x[:nb]) for x in (tg0, eq0, leq0))
                got = six.six_batch_vc(ctx, kind, True, tg, vc, leq, eq, max_iter=MAX_ITER)
                route = six.six_batch_last_route()
                med, lo, hi = timed(lambda: six.six_batch_vc(ctx, kind, True, tg, vc, leq, eq, max_iter=MAX_ITER), a.warmup, a.reps)
                one = []

                def loop():
                    one[:] = [solver.maxm(tg[b], vc, eq[b], leq[b]) for b in range(nb)]
                lmed, llo, lhi = timed(loop, 1 if nb <= 64 else 0, 3 if nb <= 64 else 1)
                same = all(int(got[0][b]) == int(one[b][0]) and got[1][b].tobytes() == np.asarray(one[b][1]).tobytes() and
                           (one[b][0] != 0 or got[2][b].tobytes() == one[b][2].tobytes()) for b in range(nb))
                print(json.dumps(dict(shape=name, kind="rational" if kind == six.RAT else "fp64", per_call=nb, route=route,
                                      batch_median_ms=round(med * 1e3, 3), batch_min_ms=round(lo * 1e3, 3), batch_max_ms=round(hi * 1e3, 3),
                                      batch_lps_per_s=round(nb / med), loop_ms=round(lmed * 1e3, 3), loop_lps_per_s=round(nb / lmed),
                                      loop_us_per_lp=round(lmed / nb * 1e6, 1), speedup=round(lmed / med, 1), same_answers=same,
                                      optimal=int((got[0] == 0).sum()))), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
