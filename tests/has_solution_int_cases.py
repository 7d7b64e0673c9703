"""Shared by tests/test_has_solution_int_host.py and tests/test_gpu_has_solution_int.py: a Python restatement of the route rule
of xpg_has_solution_int_batch_* (csrc/has_solution_int.hip.h: hs_int_plan, on top of the view of mip_hbm_plan for each
direction), the systems the GPU cases are made of and the checker's answers. Importing it needs no GPU.

Systems past the LDS walk: the 16 programs of free_var_cases.wide_lp_f64 (50 x 21, 16 free variables) without their objective
-- Lineq::has_solution builds its own -- as int32, changed so that the two walks end in every way has_solution tells apart:
WIDE_HS     system b by b % 4 --  0: as drawn;  1: row 49 := x0 <= -5;  2: row 1 := 0 <= 1 and column 1 zeroed in rows 36..49
            (a variable no row mentions: its objective entry is 0);  3: row 48 := 2 x2 <= 1, row 49 := -2 x2 <= -1 (x2 = 1/2:
            feasible over the rationals, not over the integers).
WIDE_HS_EQ  the same with two equalities at the root, x18 + x19 = 2 and x18 - x19 = c (c = 0 for b < 8, else 1: no integer
            solution); columns 18 and 19 are zeroed in rows 36..49 and rows 0 <-> 18, 1 <-> 19 swapped, so that the only
            inequalities that mention the substituted variables have row indices inside the equalities' rows (lpsol.h:1232
            reads the leading value at the INEQUALITY's row index).

Checker: the CPU restatement, non-strict (free variables). Per system (has[u = 0], has[u = 1], maxm status, minm status): the
verdicts from port.has_solution(..., True, u) (has_solution_cases.int_answers), the statuses from port.mip_solve on the
feasibility objective; the minm status is computed wherever maxm did not end 0 or negative."""
import numpy as np

import free_var_cases as fc
import has_solution_cases as hs
from free_var_cases import RAT, non_strict
from tools import gen

ROUTE_LDS, ROUTE_HBM, ROUTE_HOST = 0, 1, 2
LDS_STATIC = 800                      # has_solution_int.hip.h HS_INT_HBM_LDS_STATIC = mip_tree_hbm.hip.h MIP_HBM_LDS_STATIC
LDS_MAX = 160 * 1024
SCRATCH_MAX = 256 << 20
THREADS, WAVES_PER_CU = 256, 16       # mip_tree_hbm.hip.h MIP_HBM_THREADS, MIP_HBM_WAVES_PER_CU
WIDE_SHAPE = (50, 0, 20, 16)          # (inequalities, equalities, variables, free variables), as has_solution_cases names shapes
WIDE_EQ_SHAPE = (50, 2, 20, 16)
WIDE_COUNT = 16
LDS_SHAPES = ((4, 1, 4, 0), (5, 2, 5, 1))
NEGATIVE_SHAPE = (9, 2, 4, 0)         # more inequality rows than columns: lpsol.h:1232 leaves the row, -7


# ---- mirror of hs_int_plan --------------------------------------------------------------------------------------------------
def plan(vc, leq_rows, eq_rows, cols, nb, cus=256):
    """hs_int_plan<R32> as the dict xpoly_amd.six.has_solution_int_plan returns, from mip_hbm_plan's view of each direction."""
    from xpoly_amd.six import mip_hbm_plan
    a, b = (mip_hbm_plan(RAT, vc, leq_rows, eq_rows, cols, False, d, nb, cus) for d in (True, False))
    out = dict(free=a["free"], rmax=a["R"], lds_max=a["lds"], lds_min=b["lds"], threads_max=a["threads"], threads_min=b["threads"],
               grid_max=a["grid"], grid_min=b["grid"], help_max=0, help_min=0, slot=0, ld_max=a["ld"], ld_min=b["ld"], ws_words=a["ws_words"],
               obj_word=0, scratch=0)
    if a["route"] == ROUTE_LDS and b["route"] == ROUTE_LDS:
        # helper workgroups by mip_batch_device's rule, per pass: no root equalities, one tree per walker, the chip under-filled
        helpers = [cus if eq_rows == 0 and g["grid"] == nb and nb <= 8 * cus else 0 for g in (a, b)]
        out.update(route=ROUTE_LDS, help_max=helpers[0], help_min=helpers[1],
                   scratch=max(a["grid"] + helpers[0], b["grid"] + helpers[1]) * a["ws_words"] * 8)
        return out
    if a["route"] != ROUTE_HBM or b["route"] != ROUTE_HBM:
        out.update(route=ROUTE_HOST, grid_max=0, grid_min=0)
        return out
    lds, slot = max(a["lds"], b["lds"]), max(a["slot"], b["slot"])
    ws_words = a["ws_words"] + ((cols + 1) & ~1)
    each = slot + ws_words * 8
    per_cu = max(1, min(WAVES_PER_CU * 64 // THREADS, LDS_MAX // (lds + LDS_STATIC)))
    grid = max(1, min(cus * per_cu, SCRATCH_MAX // each, nb))
    out.update(route=ROUTE_HBM, lds_max=lds, lds_min=lds, threads_max=THREADS, threads_min=THREADS, grid_max=grid, grid_min=grid, slot=slot,
               ws_words=ws_words, obj_word=a["ws_words"], scratch=grid * each)
    return out


def vc_of(nv, nfree):
    return gen.to_rat(gen.vc_nonneg(nv, False, range(nfree)))


# ---- the systems --------------------------------------------------------------------------------------------------------------
_cache = {}


def wide_hs():
    """(vc, None, leq [16, 50, 21, 2])"""
    if "wide" not in _cache:
        _, _, leq = fc.wide_lp_f64()
        leq = leq.astype(np.int32)
        nv = leq.shape[2] - 1
        for b in range(WIDE_COUNT):
            k = b % 4
            if k == 1:
                leq[b, 49] = 0; leq[b, 49, 0] = 1; leq[b, 49, nv] = -5
            elif k == 2:
                leq[b, 1] = 0; leq[b, 1, nv] = 1
                leq[b, 36:50, 1] = 0
            elif k == 3:
                leq[b, 48] = 0; leq[b, 48, 2] = 2; leq[b, 48, nv] = 1
                leq[b, 49] = 0; leq[b, 49, 2] = -2; leq[b, 49, nv] = -1
        _cache["wide"] = (vc_of(nv, WIDE_SHAPE[3]), None, gen.to_rat(leq))
    return _cache["wide"]


def wide_hs_eq():
    """(vc, eq [16, 2, 21, 2], leq [16, 50, 21, 2])"""
    if "wide_eq" not in _cache:
        vc_arr, _, leq = wide_hs()
        leq = leq[..., 0].copy()
        nv = leq.shape[2] - 1
        leq[:, 36:50, 18] = 0; leq[:, 36:50, 19] = 0
        leq[:, [0, 18]] = leq[:, [18, 0]]
        leq[:, [1, 19]] = leq[:, [19, 1]]
        eq = np.zeros((WIDE_COUNT, 2, nv + 1), dtype=np.int32)
        eq[:, 0, 18] = 1; eq[:, 0, 19] = 1; eq[:, 0, nv] = 2
        eq[:, 1, 18] = 1; eq[:, 1, 19] = -1; eq[8:, 1, nv] = 1
        _cache["wide_eq"] = (vc_arr, gen.to_rat(eq), gen.to_rat(leq))
    return _cache["wide_eq"]


def wide_negative():
    """(vc, eq, leq) of the WIDE_HS_EQ shape that end negative: WIDE_HS's inequalities as they lie under x5 = 1, x6 = 1 -- both
    variables are mentioned by inequalities whose row index is past the equalities' rows, so the reference is undefined at the
    root (lpsol.h:1232) and maxm ends -7 on all 16 (test_gpu_has_solution_int asserts it of the checker)."""
    if "wide_neg" not in _cache:
        vc_arr, _, leq = wide_hs()
        nv = leq.shape[2] - 1
        eq = np.zeros((WIDE_COUNT, 2, nv + 1), dtype=np.int32)
        eq[:, 0, 5] = 1; eq[:, 0, nv] = 1
        eq[:, 1, 6] = 1; eq[:, 1, nv] = 1
        _cache["wide_neg"] = (vc_arr, gen.to_rat(eq), leq)
    return _cache["wide_neg"]


def pick(arrays, idx):
    """The systems idx of arrays = (vc, eq, leq), in that order."""
    vc_arr, eq, leq = arrays
    idx = np.asarray(idx)
    return vc_arr, None if eq is None else np.ascontiguousarray(eq[idx]), np.ascontiguousarray(leq[idx])


def reuse_pick(nb, grid, count=WIDE_COUNT, shift=5):
    """mip_hbm_cases.reuse_pick: system i of a batch of nb is i % count rotated by `shift` from one round of `grid` systems to
    the next, so that a workgroup does not meet the same system twice in a row."""
    i = np.arange(nb)
    return (i + shift * (i // grid)) % count


# ---- the checker's answers ----------------------------------------------------------------------------------------------------
def answers(key, arrays, count):
    """[(has under u = 0, has under u = 1, maxm status, minm status or None where maxm ended 0 or negative)] of the first
    `count` systems of arrays = (vc, eq, leq), computed once per key and shared."""
    have = _cache.setdefault(("answers", key), [])
    if len(have) < count:
        port = hs.hc._port()
        vc_arr, eq, leq = arrays
        verdicts = hs.int_answers(key, arrays, count)
        with non_strict(port):
            for i in range(len(have), count):
                e = None if eq is None else eq[i]
                tg = hs.feasibility_objective(leq[i], e)
                st0 = int(port.mip_solve(RAT, True, False, tg, vc_arr, e, leq[i])[0])
                st1 = None if st0 <= 0 else int(port.mip_solve(RAT, False, False, tg, vc_arr, e, leq[i])[0])
                have.append((verdicts[i][0], verdicts[i][1], st0, st1))
    return have[:count]


def expected(want, unique):
    """(has [n], status [n, 2]) a call must return for answers()' list under is_unique_sol = unique."""
    return hs.expected(want, unique)
