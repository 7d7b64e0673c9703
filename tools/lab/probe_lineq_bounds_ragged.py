"""A/B of the ragged calcBound call against the parent's way for the same answer, host arrays in, packed rows out:
  one call   one xpg_lineq_bounds_batch_ragged_rat32 call over the whole mix (k_calc_bound_ragged: one upload, one launch)
  per class  one xpg_lineq_bounds_batch_packed_rat32 call per shape class, summed (what calc_bound_all does), at the SAME
             cap_rows as the one call; and once more at each class's own default (cap_rows 0: 4 x its rows + 16), the
             capacity calc_bound_all starts with
on the mixed SCoP of tools/lab/probe_lineq_ragged.py: triangular loop nests of depth 2 .. 6, each depth with 0 .. 3 further
upper bounds -- 20 shape classes -- the systems dealt round robin over the classes. MIX is the number of systems (64, 692,
16384), `one`: 692 systems of ONE class (8 x 5), where no gain is expected, or `wide`: ONE 60 x 20 nest (depth 19) among 1000
nests of 6 x 5, which shows what the envelope costs the small systems.
cap_rows: the one call's default (4 x most rows + 16) where every system answers ok >= 0 with it; else it is raised to the
largest need reported until every system does -- each need is a lower bound, so that is the smallest cap_rows that serves --
and the same cap_rows goes to both sides; the figure used is printed. A capacity the LDS layout refuses ends the mix with a
line that says so.
The two sides are asserted equal bit for bit, verdicts included, before timing. What is timed are the C entry points through
ctypes with their inputs prepared (the flat array of the one call, the stacked array of every class), results read through the
zero-copy view. One warm-up, then 7 alternating rounds; median, min and max in ms.
Usage: python tools/lab/probe_lineq_bounds_ragged.py MIX   (one device process per mix: tools/lab/run_lineq_bounds_ragged_ab.sh)"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tools.lab.probe_lineq_ragged import nest              # noqa: E402


def main():
    mix = sys.argv[1]
    rng = np.random.default_rng(9)
    if mix == "wide":
        shapes = [(19, 22)] + [(4, -2)] * 1000                  # 60 x 20, then 6 x 5: depth 4, the innermost loop unbounded
    elif mix == "one":
        shapes = [(4, 0)] * 692
    else:
        classes = [(d, e) for d in range(2, 7) for e in range(4)]
        shapes = [classes[(7 * b) % 20] for b in range(int(mix))]
    mats = [nest(rng, d, e) for d, e in shapes]
    nvs = [d for d, _ in shapes]
    nb = len(mats)

    import xpoly_amd
    from xpoly_amd._capi import lib, vp, XpgError
    from xpoly_amd.lineq import Lineq
    ctx = xpoly_amd.Context(0)
    lq = Lineq(ctx)
    L = lib()
    by_class = {}
    for b, m in enumerate(mats):
        by_class.setdefault(m.shape[:2], []).append(b)
    stacked = {k: np.ascontiguousarray(np.stack([mats[b] for b in idx])) for k, idx in by_class.items()}

    # ---- the capacity both sides run at
    cap = 4 * max(m.shape[0] for m in mats) + 16
    for _ in range(6):
        try:
            one = lq.bounds_ragged(mats, cap_rows=cap, copy=False)
        except XpgError as e:
            print("mix %s: cap_rows %d is refused (%s): not measured" % (mix, cap, e))
            ctx.close()
            return
        if (one[0] >= 0).all():
            break
        cap = int(-one[0].min())
    else:
        print("mix %s: no cap_rows found in 6 calls (last %d): not measured" % (mix, cap))
        ctx.close()
        return
    route = lq.bounds_ragged_last_route()
    assert route["launches"] == 1

    # ---- the two sides agree, verdicts and rows, before anything is timed
    one = lq.bounds_ragged(mats, cap_rows=cap)
    for own in (False, True):
        for (rows, cols), idx in by_class.items():
            per = lq.bounds_packed(stacked[(rows, cols)], cols - 1, cap_rows=0 if own else cap)
            if own and (per[0] < 0).any():
                continue                                        # (its own default is short: calc_bound_all would call again)
            for i, b in enumerate(idx):
                assert (one[0][b], one[1][b], one[2][b]) == (per[0][i], per[1][i], per[2][i]), (rows, cols, b)
                assert len(one[3][b]) == len(per[3][i]) and all(np.array_equal(x, y) for x, y in zip(one[3][b], per[3][i])), (rows, cols, b)
    n_ok = int((one[0] == 1).sum())
    out_rows = sum(x.shape[0] for per_sys in one[3] for x in per_sys)
    del one, per

    # ---- the timed sides: the C calls alone
    flat = np.ascontiguousarray(np.concatenate([m.reshape(-1, 2) for m in mats]))
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    rows_a, cols_a, rhs_a = i32([m.shape[0] for m in mats]), i32([m.shape[1] for m in mats]), i32(nvs)
    off = np.zeros(nb + 1, dtype=np.int64); off[1:] = np.cumsum(rows_a.astype(np.int64) * cols_a)
    nres = int(rhs_a.sum())
    ooff = np.zeros(nres + 1, dtype=np.int64); orows = np.zeros(nres, dtype=np.int32)
    ok = np.zeros(nb, dtype=np.int32); chain = np.zeros(nb, dtype=np.int32); steps = np.zeros(nb, dtype=np.int32)
    view = C.c_void_p()

    def one_call():
        rc = L.xpg_lineq_bounds_batch_ragged_rat32(ctx._h, C.c_int(nb), vp(flat), vp(rows_a), vp(cols_a), vp(off), vp(rhs_a), C.c_int(cap), C.c_int(0),
                                                   None, C.c_longlong(0), C.byref(view), vp(ooff), vp(orows), vp(ok), vp(chain), vp(steps))
        assert rc == 0

    per_args = []
    for (rows, cols), idx in by_class.items():
        n = len(idx)
        per_args.append((stacked[(rows, cols)], n, rows, cols, np.zeros(n * (cols - 1) + 1, dtype=np.int64), np.zeros(n, dtype=np.int32),
                         np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)))

    def per_class(c):
        for a, n, rows, cols, o, k, ch, s in per_args:
            rc = L.xpg_lineq_bounds_batch_packed_rat32(ctx._h, C.c_int(n), vp(a), C.c_int(rows), C.c_int(cols), C.c_int(cols - 1), C.c_int(c), C.c_int(0),
                                                       None, C.c_longlong(0), C.byref(view), vp(o), vp(k), vp(ch), vp(s))
            assert rc == 0

    sides = {"one call": one_call, "per class": lambda: per_class(cap), "per class, own default": lambda: per_class(0)}
    f = lambda v: "median %9.3f  min %9.3f  max %9.3f ms" % (float(np.median(v)), min(v), max(v))
    print("mix %s: %d systems in %d shape classes (rows x cols %s .. %s), %d results, %d steps, cap_rows %d; %d systems ok, %d rows out; one call: "
          "grid %d, LDS %d B/workgroup, cap_lds %d, seats %d B, output slots %d B"
          % (mix, nb, len(by_class), min(by_class), max(by_class), nres, route["steps"], cap, n_ok, out_rows, route["grid"], route["sys_lds"],
             route["cap_lds"], route["seat_bytes"], route["out_bytes"]))
    t = {k: [] for k in sides}
    names = list(sides)
    for rnd in range(8):                                        # round 0 is the warm-up
        for side in names if rnd % 2 == 0 else names[::-1]:
            t0 = time.perf_counter()
            sides[side]()
            if rnd:
                t[side].append((time.perf_counter() - t0) * 1e3)
    print("   one call                %s" % f(t["one call"]))
    print("   per class               %s   %d calls" % (f(t["per class"]), len(per_args)))
    print("   per class, own default  %s   %d calls" % (f(t["per class, own default"]), len(per_args)))
    ctx.close()


if __name__ == "__main__":
    main()
