"""What tests/test_lineq_levels_host.py and tests/test_gpu_lineq_levels.py share: a restatement of the plan of a levels call
(lineq_host.hip.h levels_plan: the projection's plan as tests/lineq_project_cases.py restates it, the default of a level's slot
and the bytes of the level slots), and the stepped checker that RECORDS EVERY INTERMEDIATE -- oracle/checker.py's fme applied
variable after variable, stopping as k_fme_levels_batch stops."""
import numpy as np

import lineq_project_cases as pc
from lineq_project_cases import XPG_ERR_SHAPE, XPG_ERR_UNSUPPORTED, rows_equal, CHAIN_MAX   # noqa: F401 (re-exported)

PLAN_KEYS = ("launches", "grid", "groups", "sys_lds", "cap_lds", "seat_bytes", "level_bytes", "cap", "cap_out")


def plan(nb, rows, cols, n_elim, cap_rows=0, cap_out_rows=0):
    """The nine figures of xpg_test_lineq_levels_plan, or the error code."""
    if n_elim <= 0:
        return XPG_ERR_SHAPE
    if n_elim > CHAIN_MAX:
        return XPG_ERR_UNSUPPORTED
    p = pc.plan(nb, rows, cols, cap_rows, cap_out_rows)
    if not isinstance(p, dict):
        return p
    cap_out = min(p["cap"], 4 * rows + 16) if cap_out_rows <= 0 else p["cap_out"]
    return dict(zip(PLAN_KEYS, (1, p["grid"], p["groups"], p["sys_lds"], p["cap_lds"], p["seat_bytes"],
                                nb * n_elim * cap_out * cols * 8, p["cap"], cap_out)))


def plan_view(nb, rows, cols, n_elim, cap_rows=0, cap_out_rows=0):
    """xpg_test_lineq_levels_plan (host only): the same dict, or the error code."""
    import ctypes as C
    from xpoly_amd._capi import lib
    out = np.zeros(9, dtype=np.int64)
    rc = lib().xpg_test_lineq_levels_plan(C.c_int(nb), C.c_int(rows), C.c_int(cols), C.c_int(n_elim), C.c_int(cap_rows),
                                          C.c_int(cap_out_rows), out.ctypes.data_as(C.c_void_p), C.c_int(9))
    return rc if rc != 0 else dict(zip(PLAN_KEYS, (int(x) for x in out)))


def stepped_levels(port, mat, nv, elim, dark=False, cap_rows=None, cap_out_rows=None):
    """(ok, steps, levels, needs, sizes): the checker's fme step after step, every intermediate kept. levels[k] is the system
    with elim[0 .. k] eliminated; a system with ok <= 0 has every level empty. needs[k] as lineq_project_cases.stepped; sizes[k]
    is the row count of level k as far as the walk got (whatever the verdict)."""
    cur = np.asarray(mat)
    empty = np.zeros((0, cur.shape[1], 2), dtype=np.int32)
    n = len(elim)
    levels, needs, sizes = [], [], []
    for k, u in enumerate(elim):
        if cur.shape[0] == 0:                                # fme of an empty system: true and empty, to the end of the list
            break
        need = None if pc.has_bad_row(cur, nv) else pc.step_need(cur, u)
        needs.append(need)
        if need is not None and cap_rows and need > cap_rows:
            return -need, k, [empty] * n, needs, sizes
        ok, res = port.fme(cur, nv, u, dark)
        if not ok:
            return 0, k, [empty] * n, needs, sizes
        cur = np.asarray(res)
        if cur.shape[0] == 0:
            cur = empty
        sizes.append(cur.shape[0])
        if cap_out_rows and cur.shape[0] > cap_out_rows:
            return -cur.shape[0], k, [empty] * n, needs, sizes
        levels.append(cur)
    levels += [empty] * (n - len(levels))
    return 1, n, levels, needs, sizes
