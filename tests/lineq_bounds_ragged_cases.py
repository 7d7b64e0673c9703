"""What tests/test_lineq_bounds_ragged_host.py and tests/test_gpu_lineq_bounds_ragged.py share: a restatement of the plan of a
ragged calcBound call (lineq_host.hip.h bounds_ragged_plan: every system under bounds_plan's shape rules, then the ENVELOPE --
the widest system's columns, the most rows -- under bounds_plan's capacity rules as tests/lineq_bounds_cases.py restates them,
three slots per seat, the output slots following each system's own columns), the mixed batch of the GPU tests, and the chain
checker of the uniform tests applied per system at the call's capacities."""
import numpy as np

import lineq_bounds_cases as bc
import lineq_project_cases as pc
from lineq_bounds_cases import XPG_ERR_SHAPE, XPG_ERR_UNSUPPORTED, rows_equal   # noqa: F401 (re-exported)
from lineq_ragged_cases import class_batch

PLAN_KEYS = ("launches", "grid", "groups", "sys_lds", "cap_lds", "seat_bytes", "out_bytes", "steps", "cap", "cap_out", "cols", "rows")
ROUTE_KEYS = PLAN_KEYS[:8]
# (rows, nv, systems): the widest system (cols 6) is (4, 5), the tallest (9 rows) is (9, 4) -- the envelope is split
CLASSES = [(3, 1, 12), (4, 2, 12), (5, 3, 12), (6, 4, 12), (4, 5, 12), (9, 4, 48)]
# tests/test_gpu_lineq_bounds.py's ABOVE_ZERO: chains 0 and 1 run, chain 2 needs 651 rows at its last step
ABOVE_ZERO = (9, 4, [4242, 9, 1037], (-651, 2, 2))


def plan(rows, cols, rhs=None, cap_rows=0, cap_out_rows=0):
    """The twelve figures of xpg_test_lineq_bounds_ragged_plan, or the error code. rhs None: the last column of each system."""
    nb = len(rows)
    if nb <= 0:
        return XPG_ERR_SHAPE
    rr = [cols[b] - 1 if rhs is None else rhs[b] for b in range(nb)]
    for b in range(nb):
        if rows[b] <= 0 or cols[b] <= 1 or rr[b] < 1 or rr[b] >= cols[b]:
            return XPG_ERR_SHAPE
    ecols, erows = max(cols), max(rows)
    if erows > 32767:
        return XPG_ERR_UNSUPPORTED
    cap = 4 * erows + 16 if cap_rows <= 0 else cap_rows
    cap = max(cap, erows)
    cap_out = cap if cap_out_rows <= 0 or cap_out_rows > cap else cap_out_rows
    if cap > 32767:
        return XPG_ERR_UNSUPPORTED
    cap_lds, lds = pc.fme_lds(cap, cap, ecols)
    if lds > 160 * 1024:
        return XPG_ERR_UNSUPPORTED
    sys_lds = (lds + 15) & ~15
    grid = min(nb, 4096)                                     # fme takes the whole wave: one system per workgroup
    cells = sum(rr[b] * cols[b] for b in range(nb))
    steps = sum((r - 1) * (r + 2) // 2 for r in rr)
    return dict(zip(PLAN_KEYS, (1, grid, 1, sys_lds, cap_lds, grid * 3 * cap * ecols * 8, cells * cap_out * 8, steps, cap, cap_out, ecols, erows)))


def plan_view(rows, cols, rhs=None, cap_rows=0, cap_out_rows=0, nb=None):
    """xpg_test_lineq_bounds_ragged_plan (host only): the same dict, or the error code."""
    import ctypes as C
    from xpoly_amd._capi import lib
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    r, c, h = i32(rows), i32(cols), i32(rhs)
    out = np.zeros(12, dtype=np.int64)
    rc = lib().xpg_test_lineq_bounds_ragged_plan(C.c_int(len(rows) if nb is None else nb), vp(r), vp(c), vp(h), C.c_int(cap_rows),
                                                 C.c_int(cap_out_rows), vp(out), C.c_int(12))
    return rc if rc != 0 else dict(zip(PLAN_KEYS, (int(x) for x in out)))


def mixed_batch():
    """The six classes interleaved, 108 systems: (mats, nvs, cls) with cls[b] the index into CLASSES. Round i takes the i-th
    system of every class that still has one, so the first 12 rounds hold all six classes and the last 36 systems are (9, 4)."""
    classes = [class_batch(r, nv, n) for r, nv, n in CLASSES]
    mats, nvs, cls = [], [], []
    for i in range(max(n for _, _, n in CLASSES)):
        for c, (_, nv, n) in enumerate(CLASSES):
            if i < n:
                mats.append(classes[c][i]); nvs.append(nv); cls.append(c)
    return mats, nvs, cls


def above_zero():
    from tools import gen
    rows, nv, seed, _ = ABOVE_ZERO
    return gen.random_system(np.random.default_rng(seed), rows, nv)


def collector_calls(port, mats, nvs):
    """The calls xpoly_amd::calc_bound_each makes for these systems, replayed on the CPU with the checker: the capacities start
    at 4 * (most rows) + 16 for both and are raised as the collector raises them. Returns the number of calls (9: never)."""
    most = max(m.shape[0] for m in mats)
    cap = cap_out = 4 * most + 16
    for call in range(1, 9):
        oks = [bc.chains(port, mats[b], nvs[b], cap, cap_out)[0] for b in range(len(mats))]
        need_cap = max([-o for o in oks if -o > cap] or [0])
        need_out = max([-o for o in oks if 0 < -o <= cap] or [0])
        if not need_cap and not need_out:
            return call
        if need_cap:
            cap = cap_out = need_cap
        else:
            cap_out = need_out
    return 9


def want(port, mats, nvs, cap_rows=None, cap_out_rows=None):
    """[(ok, chain, steps, bounds)] as xpg_lineq_bounds_batch_ragged_rat32 answers: lineq_bounds_cases.chains per system, at the
    CALL's capacities."""
    return [bc.chains(port, mats[b], nvs[b], cap_rows, cap_out_rows) for b in range(len(mats))]
