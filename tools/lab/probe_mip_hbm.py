"""Times xpg_mip_batch_vc_hbm_* -- MIP trees whose node LPs are past 64 KB of LDS, one workgroup per tree with the node tableaux in
device memory (--mode hbm) -- against the route such batches had: xpg_mip_batch_vc_*, which sends them to the host controller
(--mode host: lock-step rounds, every node normalised on the host; that entry point is unchanged).
Trees: tests/mip_hbm_cases.py WIDE (20 variables of which 16 are free, 50 inequalities, integer branching), its 16 programs cycled
to --nb, kinds --kinds, both directions. Host arrays in, one call, warm-up, then the median of --reps call times by the host
clock (transfers and the synchronisation included on both sides). Both modes must report the same statuses and node count. One
JSON line per kind and direction."""
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
    ap.add_argument("--mode", choices=("hbm", "host"), default="hbm")
    ap.add_argument("--kinds", default="0,1")
    ap.add_argument("--nb", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    import xpoly_amd
    from xpoly_amd import six
    import mip_hbm_cases as mc
    ctx = xpoly_amd.Context(0)
    for kind in (int(k) for k in a.kinds.split(",")):
        tg0, vc, leq0 = mc.wide(kind)
        pick = np.arange(a.nb) % mc.WIDE_COUNT
        tg, leq = np.ascontiguousarray(tg0[pick]), np.ascontiguousarray(leq0[pick])
        for is_max in (True, False):
            if a.mode == "hbm":
                run = lambda: six.mip_batch_vc_hbm(ctx, is_max, False, tg, vc, leq, kind=kind)
            else:
                run = lambda: six.mip_batch_vc(ctx, is_max, False, tg, vc, leq, kind=kind)
            for _ in range(a.warmup):
                run()
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter(); st, _, _, nodes = run(); ts.append(time.perf_counter() - t0)
            med = statistics.median(ts)
            out = dict(label=a.label, mode=a.mode, kind="fp64" if kind == six.F64 else "rational", is_max=is_max, nb=a.nb, nodes=int(nodes),
                       median_ms=round(med * 1e3, 3), min_ms=round(min(ts) * 1e3, 3), max_ms=round(max(ts) * 1e3, 3),
                       trees_per_s=round(a.nb / med, 1), statuses={int(k): int((st == k).sum()) for k in np.unique(st)},
                       mip_route=six.mip_last_route())
            if a.mode == "hbm":
                out.update(route=six.mip_hbm_last_route(),
                           plan=six.mip_hbm_plan(kind, vc, mc.WIDE_ROWS, 0, mc.WIDE_COLS, False, is_max, a.nb))
            print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
