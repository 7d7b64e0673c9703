"""Inputs of tests/test_gpu_mip_hbm.py -- batches of MIP trees whose node LPs are past the 64 KB of LDS the device tree walk
has, so that xpg_mip_batch_vc_hbm_* walks them with the node tableaux in device memory -- and the checker's answers for
them, computed once per process. The checker is the CPU restatement in non-strict mode (free_var_cases.non_strict: the real
reference is undefined with a free variable).

WIDE  free_var_cases.wide_lp_f64: 20 variables of which 16 are free, 50 inequalities, integer branching; as fp64 and, the data
      being integral, as Rational. The oracle decides all 16 in both directions and both kinds (no -7), statuses 0 and 2, trees
      of 1 to 19 nodes; every Rational tree takes it under 0.1 s of CPU time.
IND   a rational_indicator with flags on the free variables 0, 3 and 7: the `allow` branch of is_satisfying; it changes the
      node counts of 8 of the 32 fp64 trees.
EQ    0-1 branching with two equalities at the root, 12 variables, 52 inequalities: 52 is the smallest m_leq at which the LDS
      walk refuses mip_eq_cases.random_mip_eq(rng, m_leq, 2, 12, True) (test_gpu_mip_hbm asserts it). 32 programs of two kinds
      (those draws of the generator without the 12 upper-bound rows and without an indicator, so that the batch has one shape):
        raw     every fourth program (0, 4, ..., 28): the generator's draws at m_leq = 52 as they come. The reference reads the
                leading value of a substitution at the INEQUALITY's row index (lpsol.h:1232): with more than cols = 13 dense
                inequalities every such draw is undefined at its root -- the oracle returns -7 for all of them in both
                directions and both kinds, with every seed tried (0 .. 7). They carry the "-7 alone" property: the device must
                end them -7, as the host controller does, and the trees around and after them must not notice.
        padded  the other 24: draws at m_leq = 2 (every row index inside an equality's row: the reference is defined) followed
                by 50 rows 0.x <= b, b in [0, 8]: rows that constrain nothing and make the node LP as large as a raw one's.
                With seed 9 the oracle decides 24 of 24 (no -7) in both directions and both kinds, each tree in milliseconds;
                fp64: statuses {1, 2} maximising and {0, 2} minimising, trees of up to 3 and 5 nodes; Rational: {0, 1, 2} and
                {0, 2}, up to 21 and 7 nodes. (With 4 or more drawn inequalities every fp64 root LP is infeasible and nothing
                branches: the search over m_leq and the seed was made on the CPU oracle alone.)
      So the oracle leaves out 8 of 32 = 25 %, the cap the batch may skip."""
import numpy as np

import free_var_cases as fc
import mip_eq_cases
from free_var_cases import F64, RAT
from tools import gen

WIDE_COUNT, WIDE_ROWS, WIDE_COLS, WIDE_FREE = 16, 50, 21, 16
IND = np.zeros(WIDE_COLS, dtype=np.uint8)
IND[[0, 3, 7]] = 1
EQ_NV, EQ_ROWS, EQ_M_LEQ, EQ_SEED, EQ_COUNT = 12, 2, 52, 9, 32
EQ_DRAWN, EQ_RAW_EVERY = 2, 4                # inequalities a padded program draws; every fourth program is a raw draw

_cache = {}


def wide(kind):
    """(tgtf [16, 21(,2)], vc, leq [16, 50, 21(,2)])"""
    tg, vc, leq = fc.wide_lp_f64()
    if kind == RAT:
        return gen.to_rat(tg.astype(np.int32)), gen.to_rat(vc.astype(np.int32)), gen.to_rat(leq.astype(np.int32))
    return tg, vc, leq


def wide_oracle(port, kind, is_max, ind=None):
    """[(status, v, sol, nodes)] of the 16 WIDE programs."""
    key = ("wide", kind, is_max, ind is not None)
    if key not in _cache:
        tg, vc, leq = wide(kind)
        out = []
        with fc.non_strict(port):
            for b in range(WIDE_COUNT):
                stats = {}
                w = port.mip_solve(kind, is_max, False, tg[b], vc, None, leq[b], ind, stats)
                out.append((w[0], w[1], w[2], stats["nodes"]))
        _cache[key] = out
    return _cache[key]


def _eq_draws():
    if "eq" not in _cache:
        rng = np.random.default_rng(EQ_SEED)
        n_raw = EQ_COUNT // EQ_RAW_EVERY
        raw, padded = [], []
        while len(padded) < EQ_COUNT - n_raw:
            p = mip_eq_cases.random_mip_eq(rng, EQ_DRAWN, EQ_ROWS, EQ_NV, True)
            if p["leq"].shape[0] != EQ_DRAWN or "ind" in p:
                continue
            pad = np.zeros((EQ_M_LEQ - EQ_DRAWN, EQ_NV + 1), dtype=np.int32)
            pad[:, EQ_NV] = rng.integers(0, 9, size=EQ_M_LEQ - EQ_DRAWN)
            p["leq"] = np.concatenate([p["leq"], gen.to_rat(pad)], axis=0)
            padded.append(p)
        while len(raw) < n_raw:
            p = mip_eq_cases.random_mip_eq(rng, EQ_M_LEQ, EQ_ROWS, EQ_NV, True)
            if p["leq"].shape[0] == EQ_M_LEQ and "ind" not in p:
                raw.append(p)
        raw, padded = iter(raw), iter(padded)
        _cache["eq"] = [next(raw) if i % EQ_RAW_EVERY == 0 else next(padded) for i in range(EQ_COUNT)]
    return _cache["eq"]


def eq_batch(kind):
    """(tgtf [32, 13(,2)], vc, eq [32, 2, 13(,2)], leq [32, 52, 13(,2)]): every fourth entry a raw draw, the others padded."""
    ps = _eq_draws()
    tg, eq, leq = (np.stack([p[k] for p in ps]) for k in ("tgtf", "eq", "leq"))
    vc = ps[0]["vc"]
    if kind == F64:
        return fc.as_f64(tg), fc.as_f64(vc), fc.as_f64(eq), fc.as_f64(leq)
    return tg, vc, eq, leq


def eq_oracle(port, kind, is_max):
    """[(status, v, sol, nodes)] of the 32 EQ programs."""
    key = ("eqo", kind, is_max)
    if key not in _cache:
        tg, vc, eq, leq = eq_batch(kind)
        out = []
        with fc.non_strict(port):
            for b in range(EQ_COUNT):
                stats = {}
                w = port.mip_solve(kind, is_max, True, tg[b], vc, eq[b], leq[b], None, stats)
                out.append((w[0], w[1], w[2], stats["nodes"]))
        _cache[key] = out
    return _cache[key]


REUSE_SHIFT = 5


def reuse_pick(nb, grid, count=WIDE_COUNT, shift=REUSE_SHIFT):
    """Which of the `count` programs tree i of a batch of nb is: np.arange(nb) % count rotated by `shift` from one round of
    `grid` trees to the next -- grid is a multiple of 16 and of 32 on every device, so without the rotation a workgroup
    would walk the same program again and again."""
    i = np.arange(nb)
    return (i + shift * (i // grid)) % count
