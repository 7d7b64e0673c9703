"""What tests/test_lineq_hull_host.py and tests/test_gpu_lineq_hull.py share: Lineq::ConvexHullUnionAndIntersect
(src/com/linsys.cpp:283-336) and the projected union of PolyTran::step_4 (src/eng/poly.cpp:4802-4823) composed line for line
from the checkers' fme chains and reduce (oracle/checker.py, through tests/lineq_bounds_cases.py chains and
tests/lineq_project_cases.py stepped, which stop as the device kernels stop), a restatement of the plan of a hull call
(lineq_hull_host.hip.h hull_plan), and the batch of groups the GPU tests run."""
import ctypes as C

import numpy as np

import lineq_bounds_cases as bc
import lineq_bounds_ragged_cases as brc
import lineq_project_cases as pc
import lineq_ragged_cases as lrc
from lineq_project_cases import XPG_ERR_SHAPE, XPG_ERR_UNSUPPORTED, rows_equal   # noqa: F401 (re-exported)

PLAN_KEYS = ("producer_launches", "launches", "grid", "lds", "groups_lds", "groups_device", "seat_bytes", "slot_bytes", "out_bytes",
             "cap", "cap_out", "cap_hull", "lds_rows", "cols")
ROUTE_KEYS = PLAN_KEYS[:9]
HOME_NONE, HOME_LDS, HOME_DEVICE = -1, 0, 1
# (rows, nv) of the classes the members come from: depth 1 .. 5, at most 9 rows (tests/lineq_bounds_ragged_cases.py CLASSES)
CLASSES = [(r, nv) for r, nv, _ in brc.CLASSES]


def _empty(cols):
    return np.zeros((0, cols, 2), dtype=np.int32)


def _finish(chk, res, cols, rhs, is_intersect, gathered):
    """linsys.cpp:325-335: reduce over the lot; an inconsistent intersection is cleaned."""
    ok, rows = chk.reduce(res, rhs, is_intersect)
    if not ok and is_intersect:
        rows = _empty(cols)
    return (1 if ok else 0), -1, -1, 0, rows, gathered


def hull(chk, members, rhs, is_intersect, cap_rows=None, cap_out_rows=None, cap_hull=None):
    """(ok, member, chain, steps, rows, gathered) of one list as xpg_lineq_hull_batch_ragged_rat32 answers it."""
    members = [np.asarray(m) for m in members]
    if not members:                                          # linsys.cpp:289-292
        return 1, -1, -1, 0, _empty(0), 0
    cols = members[0].shape[1]
    each = [bc.chains(chk, m, rhs, cap_rows, cap_out_rows) for m in members]
    for i, (ok, chain, steps, _) in enumerate(each):         # the stated deviation: the lowest failing member answers
        if ok <= 0:
            return ok, i, chain, steps, _empty(cols), 0
    res = [np.zeros((1, cols, 2), dtype=np.int32)]           # res.reinit(1, cols): one row of 0/1
    res[0][..., 1] = 1
    for _, _, _, bounds in each:                             # the members in list order
        assert len(bounds) == rhs
        for t in bounds:                                     # the variables 0 .. rhs-1
            if t.shape[0] != 0:                              # t->size() != 0
                res.append(t)
    res = np.concatenate(res)
    if cap_hull and res.shape[0] > cap_hull:
        return -res.shape[0], -1, -1, 0, _empty(cols), 0
    return _finish(chk, res, cols, rhs, is_intersect, res.shape[0])


def project_union(chk, members, rhs, elims, is_intersect=False, dark=False, cap_rows=None, cap_out_rows=None, cap_hull=None):
    """The same for the step_4 shape: every member projected by its list, the results concatenated, one reduce. No lead row."""
    members = [np.asarray(m) for m in members]
    if not members:
        return 1, -1, -1, 0, _empty(0), 0
    cols = members[0].shape[1]
    each = [pc.stepped(chk, m, rhs, e, dark, cap_rows, cap_out_rows) for m, e in zip(members, elims)]
    for i, (ok, steps, _, _) in enumerate(each):
        if ok <= 0:
            return ok, i, -1, steps, _empty(cols), 0
    res = np.concatenate([_empty(cols)] + [rows for _, _, rows, _ in each if rows.shape[0] != 0])
    if cap_hull and res.shape[0] > cap_hull:
        return -res.shape[0], -1, -1, 0, _empty(cols), 0
    if res.shape[0] == 0:                                    # nothing gathered: reduce of no rows is true and empty
        return 1, -1, -1, 0, _empty(cols), 0
    return _finish(chk, res, cols, rhs, is_intersect, res.shape[0])


def want(chk, groups, rhss, is_intersect, **caps):
    return [hull(chk, g, r, is_intersect, **caps) for g, r in zip(groups, rhss)]


def same(got, wanted, what=""):
    """got: Lineq.hull_ragged's five; wanted: [hull(...)]. Bit for bit, the shape of every result included."""
    ok, member, chain, steps, rows = got
    assert len(ok) == len(wanted) == len(rows), what
    for g, w in enumerate(wanted):
        assert (ok[g], member[g], chain[g], steps[g]) == w[:4], (what, g, ok[g], member[g], chain[g], steps[g], w[:4])
        assert rows_equal(rows[g], w[4]), (what, g, rows[g].shape, w[4].shape)
        assert rows[g].shape[1:] == (w[4].shape[1], 2), (what, g)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
def plan(group_sizes, rows, cols, rhs=None, elims=None, cap_rows=0, cap_out_rows=0, cap_hull_rows=0):
    """(the fourteen figures of xpg_test_lineq_hull_plan, homes, gcaps), or the error code. group_sizes partitions the members;
    elims None: the hull, else one list per member (the projected union)."""
    ng, nb = len(group_sizes), len(rows)
    if ng <= 0 or sum(group_sizes) != nb or min(group_sizes) < 0:
        return XPG_ERR_SHAPE
    union = elims is not None
    rr = [cols[b] - 1 if rhs is None else rhs[b] for b in range(nb)]
    cap = cap_out = ecols = 0
    seat = out = 0
    if nb:
        ecols, erows = max(cols), max(rows)
        if union:
            for b in range(nb):
                if rows[b] <= 0 or cols[b] <= 1 or not 1 <= rr[b] < cols[b] or len(elims[b]) == 0 or any(not 0 <= u < rr[b] for u in elims[b]):
                    return XPG_ERR_SHAPE
            if any(len(e) > pc.CHAIN_MAX for e in elims):
                return XPG_ERR_UNSUPPORTED
            cap = erows * erows // 4 + erows + 1 if cap_rows <= 0 else cap_rows
        else:
            for b in range(nb):
                if rows[b] <= 0 or cols[b] <= 1 or not 1 <= rr[b] < cols[b]:
                    return XPG_ERR_SHAPE
            cap = 4 * erows + 16 if cap_rows <= 0 else cap_rows
        cap = max(cap, erows)
        cap_out = cap if cap_out_rows <= 0 or cap_out_rows > cap else cap_out_rows
        if cap > 32767:
            return XPG_ERR_UNSUPPORTED
        _, lds = pc.fme_lds(cap, cap, ecols)
        if lds > 160 * 1024:
            return XPG_ERR_UNSUPPORTED
        seat = min(nb, 4096) * (2 if union else 3) * cap * ecols * 8
        out = sum((1 if union else rr[b]) * cols[b] for b in range(nb)) * cap_out * 8
    lead = 0 if union else 1
    first, wanted, shapes = 0, 1, []
    for n in group_sizes:
        if n:
            if any(cols[b] != cols[first] or rr[b] != rr[first] for b in range(first, first + n)):
                return XPG_ERR_SHAPE
            wanted = max(wanted, lead + 2 * rr[first] * n)
            out += lead * cap_out * cols[first] * 8
            shapes.append((n, cols[first], n * (1 if union else rr[first])))
        else:
            shapes.append((0, 0, 0))
        first += n
    if cap_hull_rows > 32767:
        return XPG_ERR_UNSUPPORTED
    cap_hull = cap_hull_rows if cap_hull_rows > 0 else min(wanted, 32767)
    if nb == 0:
        return dict(zip(PLAN_KEYS, (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, cap_hull, 0, 0))), [HOME_NONE] * ng, [0] * ng
    lds_rows = min(cap_hull, max(32 * 1024 // (ecols * 8), 1))
    lds = lds_rows * ecols * 8 + (pc.lineq_lds_bytes(cap_hull, 1) - cap_hull * 8) + 16
    lds = (lds + 15) & ~15
    if lds > 160 * 1024:
        return XPG_ERR_UNSUPPORTED
    homes, gcaps = [], []
    for n, c, slots in shapes:
        if n == 0:
            homes.append(HOME_NONE); gcaps.append(0)
            continue
        gcap = min(cap_hull, lead + slots * cap_out)
        homes.append(HOME_LDS if gcap * c <= lds_rows * ecols else HOME_DEVICE); gcaps.append(gcap)
    grid = min(ng, 4096)
    slot = 0
    if HOME_DEVICE in homes:
        one = cap_hull * ecols * 8
        grid = min(grid, max((1 << 30) // one, 1))
        slot = grid * one
    figures = (1, 1, grid, lds, homes.count(HOME_LDS), homes.count(HOME_DEVICE), seat, slot, out, cap, cap_out, cap_hull, lds_rows, ecols)
    return dict(zip(PLAN_KEYS, figures)), homes, gcaps


def plan_view(group_sizes, rows, cols, rhs=None, elims=None, cap_rows=0, cap_out_rows=0, cap_hull_rows=0, goff=None, nb=None):
    """xpg_test_lineq_hull_plan (host only): the same triple, or the error code."""
    from xpoly_amd._capi import lib
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    ng = len(group_sizes)
    if goff is None:
        goff = np.concatenate([[0], np.cumsum(group_sizes)])
    el = eoff = None
    if elims is not None:
        eoff = i32(np.concatenate([[0], np.cumsum([len(e) for e in elims])]))
        el = i32([u for e in elims for u in e] or [0])
    out = np.zeros(14, dtype=np.int64); homes = np.full(max(ng, 1), 9, dtype=np.int32); gcaps = np.full(max(ng, 1), -9, dtype=np.int32)
    r, c, h, g = i32(rows if len(rows) else [0]), i32(cols if len(cols) else [0]), i32(rhs), i32(goff)
    rc = lib().xpg_test_lineq_hull_plan(C.c_int(ng), vp(g), C.c_int(len(rows) if nb is None else nb), vp(r), vp(c), vp(h), vp(el), vp(eoff),
                                        C.c_int(cap_rows), C.c_int(cap_out_rows), C.c_int(cap_hull_rows), vp(out), C.c_int(14), vp(homes), vp(gcaps))
    return rc if rc != 0 else (dict(zip(PLAN_KEYS, (int(x) for x in out))), homes[:ng].tolist(), gcaps[:ng].tolist())


def shapes_of(groups, rhss=None):
    """(group_sizes, rows, cols, rhs per member) of a list of groups."""
    sizes = [len(g) for g in groups]
    rows = [m.shape[0] for g in groups for m in g]
    cols = [m.shape[1] for g in groups for m in g]
    rhs = None if rhss is None else [r for g, r in zip(groups, rhss) for _ in g]
    return sizes, rows, cols, rhs


# ---- the systems ------------------------------------------------------------------------------------------------------------------
def rat(rows):
    a = np.asarray(rows, dtype=np.int32)
    out = np.ones(a.shape + (2,), dtype=np.int32)
    out[..., 0] = a
    return out


def box(xlo, xhi, ylo, yhi):
    """xlo <= x <= xhi, ylo <= y <= yhi as rows a x + b y <= c."""
    return rat([[1, 0, xhi], [-1, 0, -xlo], [0, 1, yhi], [0, -1, -ylo]])


BOX_A, BOX_B, BOX_FAR = box(0, 10, 0, 10), box(5, 20, -3, 7), box(30, 40, 0, 10)
# x, y and a symbol n behind the constant column (rhs_idx 2): 0 <= x <= n, 0 <= y <= 5 / 1 <= x <= n + 2, 0 <= y <= 7; and n >= 0
SYM_A = rat([[1, 0, 0, 1], [-1, 0, 0, 0], [0, 1, 5, 0], [0, -1, 0, 0], [0, 0, 0, 1]])
SYM_B = rat([[1, 0, 2, 1], [-1, 0, -1, 0], [0, 1, 7, 0], [0, -1, 0, 0], [0, 0, 0, 1]])
SYM_A[0, 3] = (1, 1); SYM_B[0, 3] = (1, 1)


def pools(chk, per=40):
    """Per class of CLASSES: (the systems calcBound succeeds on, those it finds inconsistent), in the generator's order."""
    good, bad = [], []
    for r, nv in CLASSES:
        ms = lrc.class_batch(r, nv, per)
        v = [bc.chains(chk, m, nv)[0] for m in ms]
        good.append([m for m, o in zip(ms, v) if o == 1]); bad.append([m for m, o in zip(ms, v) if o == 0])
    return good, bad


SIZES = (2, 3, 1, 17, 0, 2, 5, 3)
NG = 40


def hull_batch(chk):
    """NG groups: (groups, rhss, names). The handmade lists first -- the boxes of the issue's table, the symbols -- then
    groups of SIZES members drawn class after class from the pools (every member's calcBound succeeds), among them a group
    with the constant in column cols - 2 and one that repeats a member."""
    good, _ = pools(chk)
    groups = [[BOX_A, BOX_B], [BOX_A, BOX_B, BOX_A], [BOX_A, BOX_FAR], [SYM_A, SYM_B], []]
    rhss = [2, 2, 2, 2, 1]
    names = ["overlap", "aba", "disjoint", "symbols", "empty"]
    at = [0] * len(CLASSES)
    for i in range(32):
        c, n = i % len(CLASSES), SIZES[i % len(SIZES)]
        pool = good[c]
        groups.append([pool[(at[c] + k) % len(pool)] for k in range(n)]); at[c] += n
        rhss.append(CLASSES[c][1]); names.append("c%d x%d" % (c, n))
    c = 3                                                    # the (6, 4) class with its constant in column cols - 2
    groups.append(good[c][:3]); rhss.append(CLASSES[c][1] - 1); names.append("rhs cols-2")
    a, b = good[2][0], good[2][1]
    groups.append([a, b, a]); rhss.append(CLASSES[2][1]); names.append("repeat")
    groups.append([good[3][5], good[5][5], good[3][6]]); rhss.append(4); names.append("mixed rows")   # 6 and 9 rows, both 5 wide
    return groups, rhss, names
