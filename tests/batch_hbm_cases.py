"""Shared by tests/test_batch_hbm_host.py and tests/test_gpu_batch_hbm.py: a Python restatement of the route rule of
xpg_six_batch_hbm_* (csrc/batch_hbm.hip.h: batch_hbm_geometry, hbm_side_bytes), the LP batches the GPU cases are made of and
their answers from the CPU restatement of the reference (oracle.checker.Port, computed once per case and shared). Importing
it needs no GPU and no library."""
import functools

import numpy as np

import batch_geometry as bg
from tools import gen

F64, RAT = bg.F64, bg.RAT
LDS_MAX = bg.LDS_MAX
SCRATCH_MAX = 256 << 20
THREADS, WAVES_PER_CU = 256, 16         # batch_hbm.hip.h: BATCH_HBM_THREADS, BATCH_HBM_WAVES_PER_CU
ROUTE_LDS, ROUTE_HBM, ROUTE_REFUSED = 0, 1, 2
NO_LIMIT = 0xFFFFFFFF


# ---- mirror of the host rule ----------------------------------------------------------------------------------------------
def side_bytes(kind, R, V):
    """hbm_side_bytes: every array of small_lds_bytes but the tableau, rows padded to 16 bytes, plus the constant column's
    mirror."""
    wmax = V + 1 + R + 1
    nmax = wmax - 1
    pw = (nmax + 31) // 32
    b = ((wmax + 1) & ~1) * 8 * 3           # obj, e, x
    b += ((R + 1) & ~1) * 8 * 2             # k, bcol
    b += 16 * bg.SIZEOF_CAND[kind]          # sh_c
    b += nmax * 4 * 3                       # bv2eq, rowcnt, colcnt
    b += R * 4                              # eq2bv
    b += nmax * pw * 4                      # ppt
    b += 16 * 4 + 8 * 4                     # sh_i, sh_w
    b += ((nmax + 3) & ~3) * 2              # nv, bv
    return (b + 15) & ~15


def geometry(kind, R, V, nb, cus=256):
    """batch_hbm_geometry<S>(R, V, nb, num_cus) as the dict xpoly_amd.six.six_batch_hbm_geometry returns."""
    if bg.lds_fits(kind, R, V):
        g = bg.geometry(kind, R, V, nb, cus)
        return dict(route=ROUTE_LDS, lds=g.lds, slot=0, ld=V + R + 2, threads=g.threads, grid=g.grid, scratch=0)
    ld = (V + R + 2 + 1) & ~1
    lds = side_bytes(kind, R, V)
    slot = (R * ld * 8 + 255) & ~255
    if lds + bg.SMALL_LDS_STATIC > LDS_MAX or slot > SCRATCH_MAX:
        return dict(route=ROUTE_REFUSED, lds=lds, slot=slot, ld=ld, threads=THREADS, grid=0, scratch=0)
    per_cu = max(1, min(WAVES_PER_CU * 64 // THREADS, LDS_MAX // (lds + bg.SMALL_LDS_STATIC)))
    grid = max(1, min(cus * per_cu, SCRATCH_MAX // slot, nb))
    return dict(route=ROUTE_HBM, lds=lds, slot=slot, ld=ld, threads=THREADS, grid=grid, scratch=grid * slot)


# ---- the GPU cases --------------------------------------------------------------------------------------------------------
# Shapes as SOLVED (R rows x V variables; under minm the caller hands over V x (R + 1) arrays and the kernel solves the dual):
# the first shape past LDS, a wide and a tall one, and one of odd widest width V + R + 2 (a padded column through stage 1).
# 100 x 100 has an even widest width, so its width after stage 1 has dropped the auxiliary column is odd.
# 40 x 300 itself still fits one CU's LDS (138 264 bytes in fp64): the wide shape on the HBM route is 40 x 400 (177 040), and
# 40 x 300 stays as a case of its own in both readings -- solved 40 x 300, which the rule sends to the LDS kernel (LDS_SHAPES),
# and solved 300 x 40, what minm makes of a caller's 40 x 300 arrays, which it sends to the HBM one.
SHAPES = {"first": (100, 100), "wide": (40, 400), "tall": (260, 48), "odd": (101, 100), "wide300": (40, 300), "wide300dual": (300, 40)}
LDS_SHAPES = ("wide300",)                 # route 0 in both kinds; every other shape of SHAPES is past the LDS limit
SEEDS = {"wide300dual": 1}                # mixed_batch seeds other than 0, chosen with the restatement: the cap of 300 cuts two
                                          # of this batch's LPs in their own loop under minm (one with seed 0)
FITS = (32, 63)                           # an LDS-resident shape: route 0


def _kind_arrays(kind, leq, tgtf):
    if kind == F64:
        return np.ascontiguousarray(leq, dtype=np.float64), np.ascontiguousarray(tgtf, dtype=np.float64)
    return gen.to_rat(np.asarray(leq).astype(np.int32)), gen.to_rat(np.asarray(tgtf).astype(np.int32))


@functools.lru_cache(maxsize=None)
def mixed_batch(kind, is_max, R, V, count, seed):
    """count LPs of caller shape for an R x V solve, cycling through gen.random_problem(plain=True) families 0, 1, 2 and the
    dependence-test-like family of gen.small_lp_batch_f64 (integer data, so the same LPs exist in both kinds).
    Returns (leq [count, m, cols], tgtf [count, cols]) of `kind`."""
    m, cols = bg.caller_shape(is_max, R, V)
    rng = np.random.default_rng([20261017, seed, R, V, int(is_max)])
    dl, dt = gen.small_lp_batch_f64((count + 3) // 4, m, cols, family=1, seed=gen.XS_SEED + seed + 1)
    leqs, tgs = [], []
    for i in range(count):
        if i % 4 == 3:
            leq, tg = dl[i // 4], dt[i // 4]
        else:
            p = gen.random_problem(rng, RAT, i % 4, m, cols - 1, plain=True)      # (kind RAT: integer data in every family)
            leq, tg = p["leq"][..., 0], p["tgtf"][..., 0]
        leqs.append(np.asarray(leq, dtype=np.float64)); tgs.append(np.asarray(tg, dtype=np.float64))
    leq, tg = _kind_arrays(kind, np.stack(leqs), np.stack(tgs))
    leq.setflags(write=False); tg.setflags(write=False)
    return leq, tg


# Block seeds that end SIX_SUCC (a prefix of tests/golden/g12_end_states.json's; the callers check the status again with the
# restatement): 96 x 102 cells under maxm, 101 x 97 under minm (solved 96 x 101), both past the LDS limit. Rotations of the
# list give LPs of one shape.
SUCC_SEEDS = (0, 2, 3, 4, 6, 7, 10, 11, 12, 14, 15, 16, 18, 19, 20, 22)


@functools.lru_cache(maxsize=None)
def succ_batch(is_max, count):
    """count fp64 LPs that end SIX_SUCC: gen.block_lp_f64 (maxm) / gen.cover_lp_f64 (minm) of rotations of SUCC_SEEDS."""
    seeds = list(SUCC_SEEDS)
    make = gen.block_lp_f64 if is_max else gen.cover_lp_f64
    pairs = [make(seeds[i:] + seeds[:i]) for i in range(count)]
    leq = np.ascontiguousarray(np.stack([p[0] for p in pairs])); tg = np.ascontiguousarray(np.stack([p[1] for p in pairs]))
    leq.setflags(write=False); tg.setflags(write=False)
    return leq, tg


@functools.lru_cache(maxsize=None)
def _port():
    from oracle.checker import Port
    return Port()


def oracle_one(kind, is_max, leq, tgtf, max_iter=NO_LIMIT):
    """(status, v, sol, pivots) of the CPU restatement for one LP with vc = -I."""
    port = _port()
    nv = leq.shape[1] - 1
    vc = gen.vc_nonneg(nv, kind == F64)
    p0 = port.pivot_count()
    st, v, sol = port.six_solve(kind, is_max, tgtf, vc, None, leq, max_iter)
    return int(st), v, sol, int(port.pivot_count() - p0)


_answers = {}


def oracle_answers(key, kind, is_max, leq, tgtf, max_iter=NO_LIMIT):
    """The restatement's answers for a batch, computed once per (key, kind, direction, max_iter) and shared."""
    k = (key, kind, bool(is_max), int(max_iter))
    if k not in _answers:
        _answers[k] = [oracle_one(kind, is_max, leq[i], tgtf[i], max_iter) for i in range(leq.shape[0])]
    return _answers[k]


def same_answer(got_st, got_v, got_sol, want):
    """Exact: status, the optimum's bits, and on success the solution's bits."""
    if int(got_st) != int(want[0]):
        return False
    if np.asarray(got_v).tobytes() != np.asarray(want[1]).tobytes():
        return False
    return int(want[0]) != 0 or np.asarray(got_sol).tobytes() == np.asarray(want[2]).tobytes()
