"""Shared by tests/test_has_solution_batch_host.py and tests/test_gpu_has_solution_batch.py: a Python restatement of the route
rule of xpg_has_solution_batch_* (csrc/has_solution_batch.hip.h: hs_plan, on top of six_vc_hbm_cases.plan for each direction),
the systems the GPU cases are made of and the checker's answers. Importing it needs no GPU and no library.

Systems: those of six_eq_cases.shape_arrays and six_vc_hbm_cases.arrays without their tgtf -- Lineq::has_solution builds its
own objective (SIX::reviseTargetFunc on all ones: 1 in every column that some row mentions).

Checker: the CPU restatement, non-strict wherever a variable is free. Per system (has[u = 0], has[u = 1], maxm status, minm
status): the verdicts from port.has_solution, the statuses from port.six_solve on the feasibility objective; the minm status is
computed wherever maxm did not end 0 or negative (it is what is_unique_sol = 1 needs behind a maxm status 1). Under a max_iter
(the device-memory shapes: uncapped, the restatement does not finish them) port.has_solution has no such argument and the
verdicts are the reference's rule on the two statuses, which the small shapes show equal to port.has_solution."""
import numpy as np

import batch_hbm_cases as hc
import six_eq_cases as sc
import six_vc_hbm_cases as vc
from free_var_cases import RAT, non_strict
from tools import gen

NOT_RUN = 0x7FFFFFFF
NO_LIMIT = 0xFFFFFFFF
ROUTE_LDS, ROUTE_HBM, ROUTE_OTHER = 0, 1, 2
FIELDS = ("route", "nfree", "Rmax", "lds", "slot", "ld", "threads", "grid", "scratch")

# route 0, (shape, systems): the six small shapes, two sizes that run 128 and 256 threads per system, and more inequality rows
# than columns (lpsol.h:1232 leaves the row: -7)
LDS_CASES = tuple((s, 128) for s in sc.SHAPES) + (((20, 2, 20, 1), 32), ((30, 2, 30, 2), 16), ((9, 2, 4, 0), 128))
HBM_COUNT, HBM_CAP = vc.RAT_COUNT, vc.RAT_CAP


# ---- mirror of hs_plan ----------------------------------------------------------------------------------------------------
def plan(pattern, nfree, leq_rows, eq_rows, cols, nb, cus=256):
    """hs_plan<R32> as the dict xpoly_amd.six.has_solution_batch_plan returns. nfree < 0: the _dev form."""
    a = vc.plan(RAT, pattern, nfree, leq_rows, eq_rows, cols, True, nb, cus)
    b = vc.plan(RAT, pattern, nfree, leq_rows, eq_rows, cols, False, nb, cus)
    tgc = (cols + 31) & ~31
    out = dict(nfree=a["nfree"], Rmax=max(a["Rmax"], b["Rmax"]))
    if a["route"] == vc.ROUTE_LDS and b["route"] == vc.ROUTE_LDS:
        slot = a["slot"] + tgc * 8
        grid = min(a["grid"], b["grid"])
        if grid > vc.SCRATCH_MAX // slot:
            grid = max(vc.SCRATCH_MAX // slot, 1)
        out.update(route=ROUTE_LDS, lds=max(a["lds"], b["lds"]), slot=slot, ld=a["ld"], threads=max(a["threads"], b["threads"]), grid=grid,
                   scratch=grid * slot)
        return out
    cap = nfree if nfree >= 0 else cols - 1
    lds = max(hc.side_bytes(RAT, a["Rmax"], a["Vmax"]), hc.side_bytes(RAT, b["Rmax"], b["Vmax"]))
    ld = (a["Vmax"] + a["Rmax"] + 2 + 1) & ~1
    slot = (vc.slot_cells(leq_rows, eq_rows, cols, cap, out["Rmax"], ld) + tgc) * 8
    out.update(lds=lds, slot=slot, ld=ld, threads=vc.THREADS)
    if vc.ROUTE_OTHER in (a["route"], b["route"]) or lds + vc.LDS_STATIC > vc.LDS_MAX or slot > vc.SCRATCH_MAX:
        out.update(route=ROUTE_OTHER, grid=0, scratch=0)
        return out
    per_cu = max(1, min(vc.WAVES_PER_CU * 64 // vc.THREADS, vc.LDS_MAX // (lds + vc.LDS_STATIC)))
    grid = max(1, min(cus * per_cu, vc.SCRATCH_MAX // slot, nb))
    out.update(route=ROUTE_HBM, grid=grid, scratch=grid * slot)
    return out


def plan_of_shape(shape, nb, cus=256, dev=False):
    m, me, nv, nfree = shape
    return plan(True, -1 if dev else nfree, m, me, nv + 1, nb, cus)


# ---- the systems ------------------------------------------------------------------------------------------------------------
def small_arrays(shape, count):
    """(vc, eq [count, eq_rows, cols, 2] or None, leq [count, leq_rows, cols, 2] or None) of a six_eq_cases shape."""
    _, vc_arr, eq, leq = sc.shape_arrays(shape, RAT, count)
    return vc_arr, eq, leq


def hbm_arrays(family, shape, is_max, count=HBM_COUNT):
    """The same of a six_vc_hbm_cases case (is_max only names the case: its inequalities were drawn for that direction)."""
    _, vc_arr, eq, leq = vc.arrays(family, shape, RAT, is_max, count)
    return vc_arr, eq, leq


def feasibility_objective(leq, eq):
    """SIX::reviseTargetFunc on all ones (lpsol.h:2053-2074, linsys.cpp:851-862) for one system: [cols, 2]."""
    nz = np.zeros(leq.shape[1], dtype=bool)
    for a in (leq, eq):
        if a is not None and len(a):
            nz |= (a[..., 0] != 0).any(axis=0)
    nz[-1] = False
    return gen.to_rat(nz.astype(np.int32))


def verdict(st0, st1, unique):
    """Lineq::has_solution's rule (linsys.cpp:864-876) on the two statuses: (has, the minm status as reported)."""
    for k, st in enumerate((st0, st1)):
        if st < 0:
            return st, (NOT_RUN if k == 0 else st1)
        if st == 0 or (st == 1 and not unique):
            return 1, (NOT_RUN if k == 0 else st1)
    return 0, st1


_answers = {}


def oracle_answers(key, arrays, count, max_iter=NO_LIMIT):
    """[(has under u = 0, has under u = 1, maxm status, minm status or None where maxm ended 0 or negative)] for the first
    `count` systems of arrays = (vc, eq, leq), computed once per key and shared."""
    have = _answers.setdefault((key, int(max_iter)), [])
    if len(have) < count:
        port = hc._port()
        vc_arr, eq, leq = arrays
        rhs = vc_arr.shape[0]
        with non_strict(port):
            for i in range(len(have), count):
                e = None if eq is None else eq[i]
                tg = feasibility_objective(leq[i], e)
                st0 = int(port.six_solve(RAT, True, tg, vc_arr, e, leq[i], max_iter)[0])
                st1 = None if st0 <= 0 else int(port.six_solve(RAT, False, tg, vc_arr, e, leq[i], max_iter)[0])
                if max_iter == NO_LIMIT:
                    has = tuple(int(port.has_solution(leq[i], e, vc_arr, rhs, False, u)) for u in (False, True))
                else:
                    has = tuple(verdict(st0, st1, u)[0] for u in (False, True))
                have.append((has[0], has[1], st0, st1))
    return have[:count]


def expected(want, unique):
    """(has [n], status [n, 2]) a batch call must return for oracle_answers' list under is_unique_sol = unique."""
    has = np.array([w[1 if unique else 0] for w in want], dtype=np.int32)
    st = np.array([[w[2], verdict(w[2], w[3], unique)[1]] for w in want], dtype=np.int64).astype(np.int32)
    return has, st


def int_answers(key, arrays, count):
    """[(has under u = 0, has under u = 1)] of port.has_solution(..., True, u), computed once per key."""
    have = _answers.setdefault((key, "int"), [])
    if len(have) < count:
        port = hc._port()
        vc_arr, eq, leq = arrays
        with non_strict(port):
            for i in range(len(have), count):
                e = None if eq is None else eq[i]
                have.append(tuple(int(port.has_solution(leq[i], e, vc_arr, vc_arr.shape[0], True, u)) for u in (False, True)))
    return have[:count]
