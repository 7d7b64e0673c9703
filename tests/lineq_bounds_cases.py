"""What tests/test_lineq_bounds_host.py and tests/test_gpu_lineq_bounds.py share: a restatement of the plan of a fused calcBound
call (lineq_host.hip.h bounds_plan; fme_lds and the geometry as tests/lineq_project_cases.py restates them), and the chain
checker -- for every variable j the stepped checker over the other variables, inner to outer, folded into the call's answer by
the rule of the lowest failing chain (the one Lineq::calcBound, linsys.cpp:1047-1078, meets first)."""
import numpy as np

import lineq_project_cases as pc
from lineq_project_cases import XPG_ERR_SHAPE, XPG_ERR_UNSUPPORTED, rows_equal   # noqa: F401 (re-exported)

PLAN_KEYS = ("launches", "grid", "groups", "sys_lds", "cap_lds", "seat_bytes", "steps", "cap", "cap_out")


def plan(nb, rows, cols, rhs, cap_rows=0, cap_out_rows=0):
    """The nine figures of xpg_test_lineq_bounds_plan, or the error code."""
    if nb <= 0 or rows <= 0 or cols <= 1 or rhs < 1 or rhs >= cols:
        return XPG_ERR_SHAPE
    cap = 4 * rows + 16 if cap_rows <= 0 else cap_rows
    cap = max(cap, rows)
    cap_out = cap if cap_out_rows <= 0 or cap_out_rows > cap else cap_out_rows
    if cap > 32767:
        return XPG_ERR_UNSUPPORTED
    cap_lds, lds = pc.fme_lds(cap, cap, cols)
    if lds > 160 * 1024:
        return XPG_ERR_UNSUPPORTED
    sys_lds = (lds + 15) & ~15
    groups = 1                                               # fme takes the whole wave: one system per workgroup
    grid = min((nb + groups - 1) // groups, 4096)
    steps = (rhs - 1) * (rhs + 2) // 2                       # rhs - 1 prefix steps and rhs (rhs - 1) / 2 tail steps
    return dict(zip(PLAN_KEYS, (1, grid, groups, sys_lds, cap_lds, grid * groups * 3 * cap * cols * 8, steps, cap, cap_out)))


def plan_view(nb, rows, cols, rhs, cap_rows=0, cap_out_rows=0):
    """xpg_test_lineq_bounds_plan (host only): the same dict, or the error code."""
    import ctypes as C
    from xpoly_amd._capi import lib
    out = np.zeros(9, dtype=np.int64)
    rc = lib().xpg_test_lineq_bounds_plan(C.c_int(nb), C.c_int(rows), C.c_int(cols), C.c_int(rhs), C.c_int(cap_rows), C.c_int(cap_out_rows),
                                          out.ctypes.data_as(C.c_void_p), C.c_int(9))
    return rc if rc != 0 else dict(zip(PLAN_KEYS, (int(x) for x in out)))


def chain_list(nv, j):
    """Chain j's eliminations: every variable but j, inner to outer."""
    return [i for i in range(nv - 1, -1, -1) if i != j]


def chain(port, mat, nv, j, cap_rows=None, cap_out_rows=None):
    """(ok, steps, rows, needs) of chain j alone, as lineq_project_cases.stepped; an empty list gives the input itself."""
    elim = chain_list(nv, j)
    mat = np.asarray(mat)
    if elim:
        return pc.stepped(port, mat, nv, elim, False, cap_rows, cap_out_rows)
    if cap_out_rows and mat.shape[0] > cap_out_rows:
        return -mat.shape[0], 0, mat[:0], []
    return 1, 0, mat, []


def chains(port, mat, nv, cap_rows=None, cap_out_rows=None):
    """(ok, chain, steps, bounds) as xpg_lineq_bounds_batch_packed_rat32 answers: (1, -1, 0, [rows of every j]), or the
    verdict, index and step of the lowest failing chain with every bound empty."""
    mat = np.asarray(mat)
    each = [chain(port, mat, nv, j, cap_rows, cap_out_rows) for j in range(nv)]
    for j, (ok, steps, _, _) in enumerate(each):
        if ok <= 0:
            return ok, j, steps, [mat[:0]] * nv
    return 1, -1, 0, [e[2] for e in each]


def step_needs(port, mat, nv):
    """{(j, k): need} of every step entered in every chain of a system run without a capacity, and the needs of the PREFIX
    steps among them -- step k of chain j with k < nv - 1 - j eliminates a variable above j, and chain 0's steps are all
    prefix steps."""
    needs, prefix = {}, []
    for j in range(nv):
        for k, n in enumerate(chain(port, mat, nv, j)[3]):
            if n is not None:
                needs[(j, k)] = n
                if j == 0:
                    prefix.append(n)
    return needs, prefix
