"""A/B of the levels call against the parent's route for the same answer, host arrays in, packed rows out:
  new        one xpg_lineq_levels_batch_packed_rat32 call (k_fme_levels_batch: every level in one launch)
  per-level  one xpg_lineq_fme_batch_packed_rat32 call per level, each level's packed rows the next call's input (what
             fme_all does per level); the rows are copied out of the handle's pinned view between two calls, as a caller
             has to: the next packed call stages its input there
on triangular loop nests 0 <= i0 <= N0, 0 <= ik <= i(k-1) + Nk of depth 3, 4 and 6 (2 * depth rows), eliminating
depth-1 .. 1, at nb = 1, 1024 and 16 384. The sides are asserted equal bit for bit before timing and every step's need is first
computed on the CPU against the capacities. What is timed are the C entry points through ctypes, results read through the
zero-copy view: the new side is the one call, the per-level side its calls and the memmove between them -- no per-system
Python objects on either side. One warm-up, then 5 alternating rounds; median, min and max in ms. Device memory is computed
from the shapes and the route view, not measured.
Usage: python tools/lab/probe_lineq_levels.py DEPTH NB   (one device process per shape: tools/lab/run_lineq_levels_ab.sh)"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lineq_project_cases as pc   # noqa: E402
from tools import gen              # noqa: E402


def nests(depth, nb, seed=5):
    rng = np.random.default_rng(seed + depth)
    m = np.zeros((nb, 2 * depth, depth + 1), dtype=np.int32)
    for k in range(depth):
        m[:, 2 * k, k] = -1                                     # -ik <= 0
        m[:, 2 * k + 1, k] = 1                                  # ik - i(k-1) <= Nk
        if k:
            m[:, 2 * k + 1, k - 1] = -1
        m[:, 2 * k + 1, depth] = rng.integers(4, 100, size=nb)
    return np.ascontiguousarray(gen.to_rat(m))


def fme_cap(rows):
    return rows * rows // 4 + rows + 1


def main():
    depth, nb = int(sys.argv[1]), int(sys.argv[2])
    import xpoly_amd
    from xpoly_amd._capi import lib, vp
    from xpoly_amd.lineq import Lineq
    ctx = xpoly_amd.Context(0)
    lq = Lineq(ctx)
    L = lib()
    mats = nests(depth, nb)
    rows, cols = mats.shape[1:3]
    elim = list(range(depth - 1, 0, -1))
    n = len(elim)
    el = np.array(elim, dtype=np.int32)

    # ---- once through the Python mirror: the per-level route's results, their shapes, and the equality of the two sides
    want, cur = [], mats
    for u in elim:
        ok, off, packed = lq.fme_packed(cur, depth, u)
        r = int(off[1])
        assert ok.all() and r > 0 and (np.diff(off) == r).all()   # one shape per level: the next call's input as it stands
        cur = np.ascontiguousarray(packed.reshape(nb, r, cols, 2))
        want.append(cur)
    level_rows = [w.shape[1] for w in want]
    # the CPU's word on the capacities: every step's need of system 0 (all systems share its sign pattern) and every level
    cap, cap_out = fme_cap(rows), min(fme_cap(rows), 4 * rows + 16)
    cur = mats[0]
    for k, u in enumerate(elim):
        need = pc.step_need(cur, u)
        assert need <= cap and need <= fme_cap(cur.shape[0]) and level_rows[k] <= cap_out, (k, need, level_rows)
        cur = want[k][0]
    ok, steps, levels = lq.levels_packed(mats, depth, elim)
    route = lq.levels_last_route()
    assert (ok == 1).all() and (steps == n).all() and route["launches"] == 1
    for b in range(nb):
        for k in range(n):
            assert np.array_equal(levels[b][k], want[k][b]), (b, k)
    del levels

    # ---- the timed sides: the C calls alone
    off_new = np.zeros(nb * n + 1, dtype=np.int64); ok_new = np.zeros(nb, dtype=np.int32); st_new = np.zeros(nb, dtype=np.int32)
    view = C.c_void_p()

    def new():
        rc = L.xpg_lineq_levels_batch_packed_rat32(ctx._h, C.c_int(nb), vp(mats), C.c_int(rows), C.c_int(cols), C.c_int(depth), vp(el), C.c_int(n),
                                                   C.c_int(0), C.c_int(0), C.c_int(0), None, C.c_longlong(0), C.byref(view), vp(off_new),
                                                   vp(ok_new), vp(st_new))
        assert rc == 0

    bufs = [np.empty((nb, r, cols, 2), dtype=np.int32) for r in level_rows]
    off_lv = np.zeros(nb + 1, dtype=np.int64); ok_lv = np.zeros(nb, dtype=np.int32)

    def per_level():
        cur, r_in = mats, rows
        for k, u in enumerate(elim):
            rc = L.xpg_lineq_fme_batch_packed_rat32(ctx._h, C.c_int(nb), vp(cur), C.c_int(r_in), C.c_int(cols), C.c_int(depth), C.c_int(u),
                                                    C.c_int(0), C.c_int(0), None, C.c_longlong(0), C.byref(view), vp(off_lv), vp(ok_lv))
            assert rc == 0 and off_lv[nb] == nb * level_rows[k]
            C.memmove(bufs[k].ctypes.data, view.value, bufs[k].nbytes)
            cur, r_in = bufs[k], level_rows[k]

    per_level()
    assert all(np.array_equal(bufs[k], want[k]) for k in range(n))
    new()
    assert off_new[nb * n] == nb * sum(level_rows) and (ok_new == 1).all()
    flat = np.frombuffer((C.c_int32 * (int(off_new[nb * n]) * cols * 2)).from_address(view.value), dtype=np.int32)
    assert np.array_equal(flat, np.concatenate([w.reshape(nb, -1) for w in want], axis=1).ravel())   # system-major, level after level

    t = {"new": [], "per-level": []}
    for rnd in range(6):                                        # round 0 is the warm-up
        for side in ("new", "per-level") if rnd % 2 == 0 else ("per-level", "new"):
            t0 = time.perf_counter()
            new() if side == "new" else per_level()
            if rnd:
                t[side].append((time.perf_counter() - t0) * 1e3)
    f = lambda v: "median %8.3f  min %8.3f  max %8.3f ms" % (float(np.median(v)), min(v), max(v))
    mem_new = mats.nbytes + route["level_bytes"] + route["seat_bytes"] + nb * n * 12 + nb * 8
    ins = [rows] + level_rows[:-1]
    mem_lv = max(nb * r * cols * 8 + nb * fme_cap(r) * cols * 8 + nb * 16 for r in ins)
    print("depth %d  %2d x %d  nb %5d  levels %d  rows per level %s" % (depth, rows, cols, nb, n, level_rows))
    print("   new        %s   1 launch, grid %d, LDS %d B/system, cap_lds %d, seats %d B, level slots %d B; device memory %.1f KB"
          % (f(t["new"]), route["grid"], route["sys_lds"], route["cap_lds"], route["seat_bytes"], route["level_bytes"], mem_new / 1024.0))
    print("   per-level  %s   %d calls; device memory of the largest call %.1f KB" % (f(t["per-level"]), n, mem_lv / 1024.0))
    print("   (device memory from the shapes and the route view, not measured)")
    ctx.close()


if __name__ == "__main__":
    main()
