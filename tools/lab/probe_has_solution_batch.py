"""Times xpg_has_solution_batch_rat32 (is_int_sol = 0) -- the feasibility objective, SIX::normalize once, maxm, then minm where
still open, one launch -- against the way a caller had before (--mode two_calls): the objectives built on the host, one
xpg_six_batch_vc_hbm_rat32 call with is_max = 1 on every system, the open systems compacted on the host, a second call with
is_max = 0 on them, the verdicts scattered back. Both sides take host arrays and are timed by the host clock, transfers and
synchronisation included; both must give the same verdicts (checked).
Systems: --small leq_rows,eq_rows,nv,nfree of tests/six_eq_cases.py (LDS-resident, no iteration limit) and --large of
tests/six_vc_hbm_cases.py family "pairs" (device memory, max_iter --max-iter-large on both sides), the distinct systems cycled to
--nb. One JSON line per shape."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))

import numpy as np  # noqa: E402


def two_calls(ctx, six, vc_arr, eq, leq, unique, cap):
    """has_solution's rule on top of two six_batch_vc_hbm calls: (has [nb], systems in the second call)."""
    nb = leq.shape[0]
    nz = (leq[..., 0] != 0).any(axis=1) | (eq[..., 0] != 0).any(axis=1)
    nz[:, -1] = False
    tg = np.zeros((nb, leq.shape[2], 2), dtype=np.int32)
    tg[..., 0] = nz; tg[..., 1] = 1
    has = np.zeros(nb, dtype=np.int32)
    st, _, _ = six.six_batch_vc_hbm(ctx, six.RAT, True, tg, vc_arr, leq, eq, max_iter=cap)
    decided = (st <= 0) | ((st == 1) & (not unique))
    has[decided] = np.where(st[decided] < 0, st[decided], 1)
    open_ = np.flatnonzero(~decided)
    if len(open_):
        st2, _, _ = six.six_batch_vc_hbm(ctx, six.RAT, False, np.ascontiguousarray(tg[open_]), vc_arr, np.ascontiguousarray(leq[open_]),
                                         np.ascontiguousarray(eq[open_]), max_iter=cap)
        has[open_] = np.where(st2 < 0, st2, ((st2 == 0) | ((st2 == 1) & (not unique))).astype(np.int32))
    return has, len(open_)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("batch", "two_calls"), default="batch")
    ap.add_argument("--small", default="12,3,12,2")
    ap.add_argument("--large", default="60,4,62,2")
    ap.add_argument("--nb", type=int, default=1024)
    ap.add_argument("--max-iter-large", type=int, default=48)
    ap.add_argument("--unique", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    import xpoly_amd
    from xpoly_amd import six
    import has_solution_cases as hs
    import six_eq_cases as sc
    ctx = xpoly_amd.Context(0)
    cases = []
    if a.small:
        shape = tuple(int(x) for x in a.small.split(","))
        cases.append((shape, hs.small_arrays(shape, sc.cases_of(shape)), 0xFFFFFFFF))
    if a.large:
        shape = tuple(int(x) for x in a.large.split(","))
        cases.append((shape, hs.hbm_arrays("pairs", shape, True, 64), a.max_iter_large))
    for shape, (vc_arr, eq0, leq0), cap in cases:
        pick = np.arange(a.nb) % leq0.shape[0]
        eq, leq = np.ascontiguousarray(eq0[pick]), np.ascontiguousarray(leq0[pick])
        batch = lambda: six.has_solution_batch(ctx, leq, eq, vc_arr, False, bool(a.unique), max_iter=cap)
        run = batch if a.mode == "batch" else (lambda: two_calls(ctx, six, vc_arr, eq, leq, bool(a.unique), cap)[0])
        for _ in range(a.warmup):
            run()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); has = run(); ts.append(time.perf_counter() - t0)
        med = statistics.median(ts)
        out = dict(label=a.label, mode=a.mode, shape=shape, nb=a.nb, max_iter=cap, unique=a.unique, median_ms=round(med * 1e3, 3),
                   min_ms=round(min(ts) * 1e3, 3), max_ms=round(max(ts) * 1e3, 3), systems_per_s=round(a.nb / med, 1),
                   verdicts={int(k): int((has == k).sum()) for k in np.unique(has)})
        if a.mode == "batch":
            out.update(route=six.has_solution_batch_last_route(), plan=six.has_solution_batch_plan(vc_arr, shape[0], shape[1], shape[2] + 1, a.nb))
        else:
            other = batch()
            out.update(second_call=two_calls(ctx, six, vc_arr, eq, leq, bool(a.unique), cap)[1], same_verdicts=bool((other == has).all()))
        print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
