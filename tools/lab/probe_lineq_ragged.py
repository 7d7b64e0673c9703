"""A/B of the ragged levels / projection calls against the parent's way for the same answer, host arrays in, packed rows out:
  one call   one xpg_lineq_{levels,project}_batch_ragged_rat32 call over the whole mix (k_fme_chain_ragged: one upload, one launch)
  per class  one xpg_lineq_{levels,project}_batch_packed_rat32 call per shape class, summed (what levels_all / project_all do)
on a mixed SCoP: triangular loop nests 0 <= i0 <= N0, 0 <= ik <= i(k-1) + Nk of depth 2 .. 6, each depth with 0 .. 3 further
upper bounds ik <= Mk -- 20 shape classes of 2 * depth + extra rows -- the systems dealt round robin over the classes, each
eliminating depth-1 .. 1. MIX is the number of systems (1, 64, 692, 16384: below 20 it is also the number of classes), or
`wide`: ONE 60 x 20 nest (depth 19) among 1000 nests of 6 x 5, at cap_rows 256 for the one call and for the wide class (the
default of 60 rows does not fit 160 KB of LDS on either route), which shows what the envelope costs the small systems.
The two sides are asserted equal bit for bit, verdicts included, before timing. What is timed are the C entry points through
ctypes with their inputs prepared (the flat array of the one call, the stacked array of every class), results read through the
zero-copy view. One warm-up, then 7 alternating rounds; median, min and max in ms.
Usage: python tools/lab/probe_lineq_ragged.py MIX   (one device process per mix: tools/lab/run_lineq_ragged_ab.sh)"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tools import gen              # noqa: E402


def nest(rng, depth, extra):
    m = np.zeros((2 * depth + max(extra, 0), depth + 1), dtype=np.int32)
    for k in range(depth):
        m[2 * k, k] = -1                                        # -ik <= 0
        m[2 * k + 1, k] = 1                                     # ik - i(k-1) <= Nk
        if k:
            m[2 * k + 1, k - 1] = -1
        m[2 * k + 1, depth] = rng.integers(4, 100)
    for e in range(extra):                                      # ik <= Mk, k from the innermost loop outwards
        m[2 * depth + e, depth - 1 - e % depth] = 1
        m[2 * depth + e, depth] = rng.integers(4, 100)
    return gen.to_rat(m[: 2 * depth + extra])                   # (extra < 0: the innermost loops lose their bounds)


def main():
    mix = sys.argv[1]
    rng = np.random.default_rng(9)
    if mix == "wide":
        shapes = [(19, 22)] + [(4, -2)] * 1000                  # 60 x 20, then 6 x 5: depth 4, the innermost loop unbounded
        cap_one, cap_of = 256, lambda d: 256 if d == 19 else 0
    else:
        classes = [(d, e) for d in range(2, 7) for e in range(4)]
        shapes = [classes[(7 * b) % 20] for b in range(int(mix))]
        cap_one, cap_of = 0, lambda d: 0
    mats = [nest(rng, d, e) for d, e in shapes]
    nvs = [d for d, _ in shapes]
    elims = [list(range(d - 1, 0, -1)) for d in nvs]
    nb = len(mats)

    import xpoly_amd
    from xpoly_amd._capi import lib, vp
    from xpoly_amd.lineq import Lineq
    ctx = xpoly_amd.Context(0)
    lq = Lineq(ctx)
    L = lib()
    by_class = {}
    for b, m in enumerate(mats):
        by_class.setdefault(m.shape[:2], []).append(b)
    stacked = {k: np.ascontiguousarray(np.stack([mats[b] for b in idx])) for k, idx in by_class.items()}

    # ---- the two sides agree, verdicts and rows, before anything is timed
    for levels in (True, False):
        one = (lq.levels_ragged if levels else lq.project_ragged)(mats, nvs, elims, cap_rows=cap_one)
        route = lq.ragged_last_route()
        assert route["launches"] == 1 and (one[0] == 1).all(), (one[0].min(), route)
        for (rows, cols), idx in by_class.items():
            d = cols - 1
            per = (lq.levels_packed if levels else lq.project_packed)(stacked[(rows, cols)], d, elims[idx[0]], cap_rows=cap_of(d))
            assert (per[0] == 1).all()
            for i, b in enumerate(idx):
                assert one[1][b] == per[1][i]
                if levels:
                    assert len(one[2][b]) == len(per[2][i]) and all(np.array_equal(x, y) for x, y in zip(one[2][b], per[2][i])), (rows, cols, b)
                else:
                    assert np.array_equal(one[2][b], per[2][i]), (rows, cols, b)
        if levels:
            route_levels = route
    del one, per

    # ---- the timed sides: the C calls alone
    flat = np.ascontiguousarray(np.concatenate([m.reshape(-1, 2) for m in mats]))
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    rows_a, cols_a, rhs_a = i32([m.shape[0] for m in mats]), i32([m.shape[1] for m in mats]), i32(nvs)
    off = np.zeros(nb + 1, dtype=np.int64); off[1:] = np.cumsum(rows_a.astype(np.int64) * cols_a)
    eoff = np.zeros(nb + 1, dtype=np.int32); eoff[1:] = np.cumsum([len(e) for e in elims])
    el = i32([u for e in elims for u in e])
    nres = int(eoff[nb])
    ooff = np.zeros(nres + nb + 1, dtype=np.int64); orows = np.zeros(nres + nb, dtype=np.int32)
    ok = np.zeros(nb, dtype=np.int32); steps = np.zeros(nb, dtype=np.int32)
    view = C.c_void_p()

    def one_call(levels):
        fn = L.xpg_lineq_levels_batch_ragged_rat32 if levels else L.xpg_lineq_project_batch_ragged_rat32
        rc = fn(ctx._h, C.c_int(nb), vp(flat), vp(rows_a), vp(cols_a), vp(off), vp(rhs_a), vp(el), vp(eoff), C.c_int(0), C.c_int(cap_one),
                C.c_int(0), None, C.c_longlong(0), C.byref(view), vp(ooff), vp(orows), vp(ok), vp(steps))
        assert rc == 0

    per_args = []
    for (rows, cols), idx in by_class.items():
        e = i32(elims[idx[0]])
        per_args.append((stacked[(rows, cols)], len(idx), rows, cols, e, np.zeros(len(idx) * len(e) + 1, dtype=np.int64),
                         np.zeros(len(idx), dtype=np.int32), np.zeros(len(idx), dtype=np.int32)))

    def per_class(levels):
        fn = L.xpg_lineq_levels_batch_packed_rat32 if levels else L.xpg_lineq_project_batch_packed_rat32
        for a, n, rows, cols, e, o, k, s in per_args:
            rc = fn(ctx._h, C.c_int(n), vp(a), C.c_int(rows), C.c_int(cols), C.c_int(cols - 1), vp(e), C.c_int(e.size), C.c_int(0),
                    C.c_int(cap_of(cols - 1)), C.c_int(0), None, C.c_longlong(0), C.byref(view), vp(o), vp(k), vp(s))
            assert rc == 0

    f = lambda v: "median %9.3f  min %9.3f  max %9.3f ms" % (float(np.median(v)), min(v), max(v))
    print("mix %s: %d systems in %d shape classes (rows x cols %s .. %s), %d levels; one call: grid %d, LDS %d B/system, cap_lds %d, seats %d B, "
          "level slots %d B" % (mix, nb, len(by_class), min(by_class), max(by_class), nres, route_levels["grid"], route_levels["sys_lds"],
                                route_levels["cap_lds"], route_levels["seat_bytes"], route_levels["out_bytes"]))
    for levels in (True, False):
        t = {"one call": [], "per class": []}
        for rnd in range(8):                                    # round 0 is the warm-up
            for side in ("one call", "per class") if rnd % 2 == 0 else ("per class", "one call"):
                t0 = time.perf_counter()
                one_call(levels) if side == "one call" else per_class(levels)
                if rnd:
                    t[side].append((time.perf_counter() - t0) * 1e3)
        what = "levels    " if levels else "projection"
        print("   %s one call   %s" % (what, f(t["one call"])))
        print("   %s per class  %s   %d calls" % (what, f(t["per class"]), len(per_args)))
    ctx.close()


if __name__ == "__main__":
    main()
