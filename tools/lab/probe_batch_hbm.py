"""Times xpg_six_batch_hbm_f64_dev -- fp64 LPs beyond one CU's LDS, one workgroup per LP on a tableau in device memory --
against the only route such LPs had: a loop of xpg_six_maxm_f64 single calls over the same LPs (run it on a build of the
parent commit with --mode loop and XPG_SO_PATH; the batch entry points do not exist there).
LPs: tests/batch_hbm_cases.py mixed_batch (gen.random_problem families 0-2 and the dependence-test-like family, 64 distinct
LPs cycled to --nb), max_iter --max-iter on both sides. The batch: device arrays, warm-up, then the median of --reps
enqueue + synchronise times by the host clock; pivots from out_pivots. The loop: one pass over the first --loop-count LPs.
XPG_BATCH_HBM_THREADS / XPG_BATCH_HBM_WAVES (hooks build) select the variant. One JSON line per size."""
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
    ap.add_argument("--sizes", default="100x100,256x256")
    ap.add_argument("--nb", type=int, default=1024)
    ap.add_argument("--max-iter", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--loop-count", type=int, default=1024)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    import xpoly_amd
    from xpoly_amd import six
    import batch_hbm_cases as hc
    from tools import gen
    ctx = xpoly_amd.Context(0)
    for size in a.sizes.split(","):
        R, V = (int(x) for x in size.split("x"))
        leq0, tg0 = hc.mixed_batch(six.F64, True, R, V, 64, 7)
        pick = np.arange(a.nb) % 64
        out = dict(label=a.label, mode=a.mode, shape=size, nb=a.nb, max_iter=a.max_iter,
                   variant=dict(threads=os.environ.get("XPG_BATCH_HBM_THREADS", "default"), waves_per_cu=os.environ.get("XPG_BATCH_HBM_WAVES", "default")))
        if a.mode == "batch":
            leq, tg = np.ascontiguousarray(leq0[pick]), np.ascontiguousarray(tg0[pick])
            m, cols = leq.shape[1], leq.shape[2]
            d_leq, d_tg = ctx.malloc(leq.nbytes), ctx.malloc(tg.nbytes)
            d_st, d_v, d_sol, d_piv = ctx.malloc(a.nb * 4), ctx.malloc(a.nb * 8), ctx.malloc(a.nb * cols * 8), ctx.malloc(a.nb * 4)
            ctx.upload(d_leq, leq); ctx.upload(d_tg, tg)

            def run():
                ctx.six_batch_hbm_dev(six.F64, True, a.nb, d_tg, d_leq, m, cols, d_st, d_v, d_sol, d_piv, max_iter=a.max_iter)
                ctx.sync()
            for _ in range(a.warmup):
                run()
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter(); run(); ts.append(time.perf_counter() - t0)
            med = statistics.median(ts)
            piv = ctx.download(np.zeros(a.nb, dtype=np.uint32), d_piv)
            st = ctx.download(np.zeros(a.nb, dtype=np.int32), d_st)
            for p in (d_leq, d_tg, d_st, d_v, d_sol, d_piv):
                ctx.free(p)
            out.update(route=six.six_batch_hbm_last_route(), geometry=six.six_batch_hbm_geometry(six.F64, R, V, a.nb),
                       median_ms=round(med * 1e3, 3), min_ms=round(min(ts) * 1e3, 3), max_ms=round(max(ts) * 1e3, 3),
                       lps_per_s=round(a.nb / med, 1), pivots=int(piv.sum()), pivots_per_s=round(int(piv.sum()) / med),
                       us_per_pivot_per_lp=round(med * 1e6 / max(1, int(piv.max())), 3),
                       statuses={int(k): int((st == k).sum()) for k in np.unique(st)})
        else:
            n = min(a.loop_count, a.nb)
            solver = six.SIX(ctx, six.F64)
            solver.set_param(0, a.max_iter)
            vc = gen.vc_nonneg(V, True)
            solver.maxm(tg0[0], vc, None, leq0[0])                    # warm-up: first-call costs are not the loop's
            t0 = time.perf_counter()
            res = [solver.maxm(tg0[pick[b]], vc, None, leq0[pick[b]]) for b in range(n)]
            dt = time.perf_counter() - t0
            st = np.array([r[0] for r in res])
            out.update(loop_lps=n, loop_s=round(dt, 3), lps_per_s=round(n / dt, 2), ms_per_lp=round(dt / n * 1e3, 3),
                       statuses={int(k): int((st == k).sum()) for k in np.unique(st)})
        print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
