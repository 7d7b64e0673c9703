"""What tests/test_lineq_project_host.py and tests/test_gpu_lineq_project.py share: a restatement of the plan of a projection
call (lineq_host.hip.h project_plan, fme_lds; ctx.hip.h lineq_geom), the rows an elimination step needs before it is reduced,
and the stepped checker -- oracle/checker.py's fme applied variable after variable, stopping as k_fme_chain_batch stops."""
import numpy as np

XPG_ERR_SHAPE = -3
XPG_ERR_UNSUPPORTED = -4
CHAIN_MAX = 64
PLAN_KEYS = ("launches", "grid", "groups", "sys_lds", "cap_lds", "seat_bytes", "cap", "cap_out")


def lineq_lds_bytes(cap, cols):
    b = cap * cols * 8 + (cap + 1) * 4 + 16 + ((cap + 1) & ~1) * 4 + ((cap + 3) & ~3)
    return (b + 15) & ~15


def fme_lds(cap, cap_in, cols):
    """(cap_lds, LDS bytes of one system): the whole result in LDS while everything fits 12 KB, else one factor per input row."""
    capx = max(cap, cap_in)
    scratch = lineq_lds_bytes(capx, cols) - capx * cols * 8 + 16
    tmp = cap_in * cols * 8
    full = cap * cols * 8 + tmp + scratch
    if full <= 12 * 1024:
        return cap, full
    cap_lds = min((cap_in + cols - 1) // cols, cap)
    return cap_lds, cap_lds * cols * 8 + tmp + scratch


def plan(nb, rows, cols, cap_rows=0, cap_out_rows=0):
    """The eight figures of xpg_test_lineq_project_plan, or the error code."""
    if nb <= 0 or rows <= 0 or cols <= 1:
        return XPG_ERR_SHAPE
    cap = rows * rows // 4 + rows + 1 if cap_rows <= 0 else cap_rows
    cap = max(cap, rows)
    cap_out = cap if cap_out_rows <= 0 or cap_out_rows > cap else cap_out_rows
    if cap > 32767:
        return XPG_ERR_UNSUPPORTED
    cap_lds, lds = fme_lds(cap, cap, cols)
    if lds > 160 * 1024:
        return XPG_ERR_UNSUPPORTED
    sys_lds = (lds + 15) & ~15
    groups = 1                                               # fme takes the whole wave: one system per workgroup
    grid = min((nb + groups - 1) // groups, 4096)
    return dict(zip(PLAN_KEYS, (1, grid, groups, sys_lds, cap_lds, grid * groups * 2 * cap * cols * 8, cap, cap_out)))


def plan_view(nb, rows, cols, cap_rows=0, cap_out_rows=0):
    """xpg_test_lineq_project_plan (host only): the same dict, or the error code."""
    import ctypes as C
    from xpoly_amd._capi import lib
    out = np.zeros(8, dtype=np.int64)
    rc = lib().xpg_test_lineq_project_plan(C.c_int(nb), C.c_int(rows), C.c_int(cols), C.c_int(cap_rows), C.c_int(cap_out_rows),
                                           out.ctypes.data_as(C.c_void_p), C.c_int(8))
    return rc if rc != 0 else dict(zip(PLAN_KEYS, (int(x) for x in out)))


def _sign(cell):
    return int(np.sign(int(cell[0]) * int(cell[1])))


def has_bad_row(mat, nv):
    """A row without variables whose constant is negative (cols == nv + 1: no symbols): fme stops there, inconsistent."""
    return any(not mat[i, :nv, 0].any() and _sign(mat[i, nv]) < 0 for i in range(mat.shape[0]))


def step_need(mat, u):
    """Rows of the step's result before it is reduced: the rows without u, plus every (positive, negative) pair -- the one
    row itself where u has a single row."""
    s = [_sign(mat[i, u]) for i in range(mat.shape[0])]
    p, n, free = s.count(1), s.count(-1), s.count(0)
    return free + (1 if p + n == 1 else p * n)


def stepped(port, mat, nv, elim, dark=False, cap_rows=None, cap_out_rows=None):
    """(ok, steps, rows, needs): the checker's fme step after step. needs[k] is step k's need where the step was entered with
    rows and without an inconsistent constant row (else None)."""
    cur = np.asarray(mat)
    empty = np.zeros((0, cur.shape[1], 2), dtype=np.int32)
    needs = []
    for k, u in enumerate(elim):
        if cur.shape[0] == 0:                                # fme of an empty system: true and empty, to the end of the list
            return 1, len(elim), empty, needs
        need = None if has_bad_row(cur, nv) else step_need(cur, u)
        needs.append(need)
        if need is not None and cap_rows and need > cap_rows:
            return -need, k, empty, needs
        ok, res = port.fme(cur, nv, u, dark)
        if not ok:
            return 0, k, empty, needs
        cur = res
    if cap_out_rows and cur.shape[0] > cap_out_rows:
        return -cur.shape[0], len(elim), empty, needs
    return 1, len(elim), cur, needs


def rows_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape[0] == 0 and b.shape[0] == 0:
        return True
    return a.shape == b.shape and np.array_equal(a, b)
