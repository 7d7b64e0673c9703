"""Times xpg_six_batch_vc_hbm_* -- LPs with equalities and free variables whose normal form is past 64 KB of LDS, one workgroup
per LP on a slot in device memory -- against the only route such batches had: xpg_six_batch_vc_*, which sends them to one
xpg_six_{maxm,minm}_* call per problem (--mode loop; that entry point and its fallback are unchanged).
LPs: tests/six_vc_hbm_cases.py family "pairs" at --shapes (leq_rows,eq_rows,nv,nfree), 64 distinct LPs cycled to --nb, both
kinds, max_iter --max-iter (fp64) / --max-iter-rat on both sides. The batch: host arrays in, one call, warm-up, then the
median of --reps call times by the host clock (transfers and the one synchronisation included, as in the loop's calls). The
loop: one pass over the first --loop-count LPs. One JSON line per shape and kind."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("batch", "loop"), default="batch")
    ap.add_argument("--shapes", default="60,4,62,2;96,4,103,2")
    ap.add_argument("--kinds", default="0,1")
    ap.add_argument("--nb", type=int, default=1024)
    ap.add_argument("--max-iter", type=int, default=300)
    ap.add_argument("--max-iter-rat", type=int, default=48)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--loop-count", type=int, default=128)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    import xpoly_amd
    from xpoly_amd import six
    import six_vc_hbm_cases as vc
    ctx = xpoly_amd.Context(0)
    for text in a.shapes.split(";"):
        shape = tuple(int(x) for x in text.split(","))
        for kind in (int(k) for k in a.kinds.split(",")):
            cap = a.max_iter if kind == six.F64 else a.max_iter_rat
            tg0, vc_arr, eq0, leq0 = vc.arrays("pairs", shape, kind, True, 64)
            out = dict(label=a.label, mode=a.mode, shape=shape, kind="fp64" if kind == six.F64 else "rational", max_iter=cap)
            if a.mode == "batch":
                pick = np.arange(a.nb) % 64
                tg, eq, leq = (np.ascontiguousarray(x[pick]) for x in (tg0, eq0, leq0))
                run = lambda: six.six_batch_vc_hbm(ctx, kind, True, tg, vc_arr, leq, eq, max_iter=cap)
                for _ in range(a.warmup):
                    run()
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter(); st, _, _ = run(); ts.append(time.perf_counter() - t0)
                med = statistics.median(ts)
                out.update(nb=a.nb, route=six.six_batch_vc_hbm_last_route(),
                           plan=six.six_batch_vc_hbm_plan(kind, vc_arr, shape[0], shape[1], shape[2] + 1, True, a.nb),
                           median_ms=round(med * 1e3, 3), min_ms=round(min(ts) * 1e3, 3), max_ms=round(max(ts) * 1e3, 3),
                           lps_per_s=round(a.nb / med, 1), statuses={int(k): int((st == k).sum()) for k in np.unique(st)})
            else:
                n = min(a.loop_count, a.nb)
                pick = np.arange(n) % 64
                tg, eq, leq = (np.ascontiguousarray(x[pick]) for x in (tg0, eq0, leq0))
                six.six_batch_vc(ctx, kind, True, tg[:1], vc_arr, leq[:1], eq[:1], max_iter=cap)       # warm-up: first-call costs are not the loop's
                t0 = time.perf_counter()
                st, _, _ = six.six_batch_vc(ctx, kind, True, tg, vc_arr, leq, eq, max_iter=cap)
                dt = time.perf_counter() - t0
                out.update(nb=n, route=six.six_batch_last_route(), loop_s=round(dt, 3), lps_per_s=round(n / dt, 2), ms_per_lp=round(dt / n * 1e3, 3),
                           statuses={int(k): int((st == k).sum()) for k in np.unique(st)})
            print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
