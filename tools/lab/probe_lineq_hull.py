"""A/B of the hull call against the parent's way for the same answer, host arrays in, rows out:
  one call   one xpg_lineq_hull_batch_ragged_rat32 call over all groups (k_calc_bound_ragged, then k_group_reduce: one
             upload, two launches, one synchronisation before the rows travel)
  composed   xpg_lineq_bounds_batch_ragged_rat32 over all members (zero-copy view), the bounds of every group concatenated
             behind a zero row in numpy (vectorised: a group's bounds are contiguous in the packed result), then
             xpg_lineq_reduce_batch_ragged_rat32 over the groups -- entry points this work does not touch
on the mixed SCoP of tools/lab/probe_lineq_ragged.py: triangular loop nests of depth 2 .. 6, each depth with 0 .. 3 further
upper bounds -- 20 shape classes. MEMBERS (64, 692, 16384) systems are grouped into hulls of GROUP (1, 2, 8, 32) members of one
depth (their rows differ), the union's bounding hull (is_intersect 0). cap_rows: raised to the largest need reported until every
member answers, the same on both sides; cap_hull_rows: the call's default.
The two sides are asserted equal bit for bit, verdicts included, before timing. One warm-up, then 7 alternating rounds; median,
min and max in ms, and the bytes of payload that cross the link on each side (systems, descriptors and counts up; rows, offsets
and verdicts down).
Usage: python tools/lab/probe_lineq_hull.py MEMBERS GROUP   (one device process per run: tools/lab/run_lineq_hull_ab.sh)"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tools.lab.probe_lineq_ragged import nest              # noqa: E402


def main():
    nb, per = int(sys.argv[1]), int(sys.argv[2])
    rng = np.random.default_rng(9)
    ng = (nb + per - 1) // per
    sizes = [min(per, nb - g * per) for g in range(ng)]
    depth = [2 + (g % 5) for g in range(ng)]
    groups = [[nest(rng, depth[g], (g + i) % 4) for i in range(sizes[g])] for g in range(ng)]
    mats = [m for g in groups for m in g]

    import xpoly_amd
    from xpoly_amd._capi import lib, vp
    from xpoly_amd.lineq import Lineq
    ctx = xpoly_amd.Context(0)
    lq = Lineq(ctx)
    L = lib()

    cap = 4 * max(m.shape[0] for m in mats) + 16
    for _ in range(6):
        one = lq.hull_ragged(groups, depth, False, cap_rows=cap)
        if (one[0] >= 0).all():
            break
        cap = int(-one[0].min())
    else:
        print("members %d group %d: no cap_rows found in 6 calls (last %d): not measured" % (nb, per, cap))
        ctx.close()
        return
    route = lq.hull_ragged_last_route()
    assert route["producer_launches"] == 1 and route["launches"] == 1

    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    flat = np.ascontiguousarray(np.concatenate([m.reshape(-1, 2) for m in mats]))
    rows_a, cols_a = i32([m.shape[0] for m in mats]), i32([m.shape[1] for m in mats])
    rhs_a = i32([d for g in range(ng) for d in [depth[g]] * sizes[g]])
    off = np.zeros(nb + 1, dtype=np.int64); off[1:] = np.cumsum(rows_a.astype(np.int64) * cols_a)
    goff = np.zeros(ng + 1, dtype=np.int32); goff[1:] = np.cumsum(sizes)
    gcols, grhs = i32([d + 1 for d in depth]), i32(depth)
    first = np.zeros(nb + 1, dtype=np.int64); first[1:] = np.cumsum(rhs_a)
    nres = int(first[nb])
    view = C.c_void_p()
    h_off = np.zeros(ng + 1, dtype=np.int64); h_rows = np.zeros(ng, dtype=np.int32)
    h_v = [np.zeros(ng, dtype=np.int32) for _ in range(4)]
    b_off = np.zeros(nres + 1, dtype=np.int64); b_rows = np.zeros(nres, dtype=np.int32)
    b_v = [np.zeros(nb, dtype=np.int32) for _ in range(3)]
    r_rows = np.zeros(ng, dtype=np.int32); r_ok = np.zeros(ng, dtype=np.int32)
    link = {}

    def one_call():
        rc = L.xpg_lineq_hull_batch_ragged_rat32(ctx._h, C.c_int(ng), vp(goff), C.c_int(nb), vp(flat), vp(rows_a), vp(cols_a), vp(off), vp(rhs_a),
                                                 C.c_int(0), C.c_int(cap), C.c_int(0), C.c_int(0), None, C.c_longlong(0), C.byref(view), vp(h_off),
                                                 vp(h_rows), vp(h_v[0]), vp(h_v[1]), vp(h_v[2]), vp(h_v[3]))
        assert rc == 0
        link["one call"] = (flat.nbytes + 40 * (nb + ng), int(h_off[ng]) * 8 + 8 * (ng + 1) + 24 * ng)
        return int(h_off[ng])

    def composed():
        rc = L.xpg_lineq_bounds_batch_ragged_rat32(ctx._h, C.c_int(nb), vp(flat), vp(rows_a), vp(cols_a), vp(off), vp(rhs_a), C.c_int(cap), C.c_int(0),
                                                   None, C.c_longlong(0), C.byref(view), vp(b_off), vp(b_rows), vp(b_v[0]), vp(b_v[1]), vp(b_v[2]))
        assert rc == 0
        total = int(b_off[nres])
        src = np.frombuffer((C.c_int32 * (total * 2)).from_address(view.value), dtype=np.int32).reshape(total, 2) if total else np.zeros((0, 2), np.int32)
        # a group's bounds are the cells [b_off[first[m0]], b_off[first[m1]]) of the packed result: shifted by the lead rows before them
        ends = b_off[first[goff]]
        cells = np.diff(ends)
        lead_before = np.cumsum(gcols.astype(np.int64))
        cat = np.empty((total + int(lead_before[-1]), 2), dtype=np.int32)
        cat[:, 0] = 0; cat[:, 1] = 1
        cat[np.arange(total, dtype=np.int64) + np.repeat(lead_before, cells)] = src
        c_off = np.zeros(ng + 1, dtype=np.int64); c_off[1:] = ends[1:] + lead_before
        c_rows = i32((cells + gcols) // gcols)
        rc = L.xpg_lineq_reduce_batch_ragged_rat32(ctx._h, C.c_int(ng), vp(cat), vp(c_rows), vp(gcols), vp(c_off), vp(grhs), C.c_int(0), vp(r_rows),
                                                   vp(r_ok))
        assert rc == 0
        link["composed"] = (flat.nbytes + 40 * nb + cat.nbytes, total * 8 + 8 * (nres + 1) + 4 * nres + 12 * nb
                            + int((r_rows.astype(np.int64) * gcols).sum()) * 8 + 8 * ng)
        return cat, c_off

    # ---- the two sides agree, verdicts and rows, before anything is timed
    cat, c_off = composed()
    for g in range(ng):
        failed = [i for i in range(goff[g], goff[g + 1]) if b_v[0][i] <= 0]
        if failed:
            assert one[1][g] == failed[0] - goff[g] and one[0][g] == b_v[0][failed[0]], g
            continue
        assert one[0][g] == r_ok[g] and one[4][g].shape[0] == r_rows[g], (g, one[0][g], r_ok[g])
        assert np.array_equal(one[4][g].reshape(-1, 2), cat[c_off[g]: c_off[g] + int(r_rows[g]) * int(gcols[g])]), g
    out_cells = one_call()
    n_ok = int((one[0] == 1).sum())
    del one

    sides = {"one call": one_call, "composed": composed}
    f = lambda v: "median %9.3f  min %9.3f  max %9.3f ms" % (float(np.median(v)), min(v), max(v))
    print("members %d in %d groups of %d (depth 2 .. 6), cap_rows %d; %d groups ok, %d cells out, %d rows gathered; one call: grid %d, LDS %d B/workgroup, "
          "groups in LDS %d / in a device slot %d, seats %d B, slots %d B, output slots %d B"
          % (nb, ng, per, cap, n_ok, out_cells, route["gathered_rows"], route["grid"], route["lds"], route["groups_lds"], route["groups_device"],
             route["seat_bytes"], route["slot_bytes"], route["out_bytes"]))
    t = {k: [] for k in sides}
    names = list(sides)
    for rnd in range(8):                                        # round 0 is the warm-up
        for side in names if rnd % 2 == 0 else names[::-1]:
            t0 = time.perf_counter()
            sides[side]()
            if rnd:
                t[side].append((time.perf_counter() - t0) * 1e3)
    for side in names:
        print("   %-9s %s   link: %d B up, %d B down" % (side, f(t[side]), link[side][0], link[side][1]))
    ctx.close()


if __name__ == "__main__":
    main()
