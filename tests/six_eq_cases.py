"""Inputs of the batched SIX tests with equalities and free variables (tests/test_six_batch_vc_host.py,
tests/test_gpu_six_batch_vc.py): LPs as SIX::maxm / minm is called with them -- inequalities, equalities, and a vc that is a
sign pattern whose free variables are the FIRST nfree, so one vc serves a whole batch -- and the checker's answers.

Checker: the CPU restatement (port.six_solve). Strict where nothing is free; for the other shapes it runs between
orc_set_strict(0) and orc_set_strict(1), because the real reference is undefined with a free variable (tests/free_var_cases.py
explains). Status counts of this generator over the 512 solves of each shape (maxm and minm), from the restatement:

    shape        Rational                          fp64
    (4,1,4,0)    {0:153, 1:162, 2:189, 3:8}        {0:58, 1:84, 2:309, 3:61}
    (5,2,5,1)    {0:137, 1:164, 2:195, 3:16}       {0:38, 1:26, 2:421, 3:27}
    (3,3,6,2)    {0:177, 1:169, 2:163, 3:3}        {0:96, 1:60, 2:323, 3:33}
    (6,2,6,0)    {0:125, 1:122, 2:252, 3:13}       {0:18, 1:36, 2:413, 3:45}
    (2,1,3,3)    {0:17, 1:224, 2:271}              {0:6, 1:173, 2:310, 3:23}
    (12,3,12,2)  {0:95, 1:142, 2:269, 3:6}         {0:9, 1:14, 2:475, 3:13, -7:1}
"""
import numpy as np

from free_var_cases import F64, RAT, as_f64, non_strict
from tools import gen

SHAPES = ((4, 1, 4, 0), (5, 2, 5, 1), (3, 3, 6, 2), (6, 2, 6, 0), (2, 1, 3, 3), (12, 3, 12, 2))   # (leq_rows, eq_rows, nv, nfree)
PER_SHAPE = 256
# from the same generator, for the batch-against-single-calls test: no inequalities at all; more inequality rows than
# columns, where convertEq2Ineq's leading value (lpsol.h:1232, read at the inequality's row index) leaves the row for some LPs;
# and two sizes at which the batch runs 128 and 256 threads per LP (the shapes above all run 64)
EXTRA_SHAPES = ((0, 2, 4, 1), (9, 2, 4, 0), (20, 2, 20, 1), (30, 2, 30, 2))
# 66 equalities, so that the choice of the substitutions (wave-wide ballots, 64 equalities a time) meets a second chunk:
# column 0 is nonzero in equality 65 alone and column 1 in equality 64 alone -- both are substituted, from behind the first
# 64 --, the other 64 stay as pairs. 64 problems, minm only: maximising, the largest normal form (135 rows) needs 163 552 B
# of LDS and takes the per-problem fallback; minimising it needs 14 320 B (fp64; 14 256 B Rational) and runs on the device.
# Rational: the solutions are compared (oracle_answers holds at least 8 of the 64 to status 0); fp64 ends almost all of
# them 2 and checks statuses and the normal form's path only.
WIDE_EQ = (3, 66, 4, 1)


def cases_of(shape):
    return 64 if shape == WIDE_EQ else PER_SHAPE


def directions(shape):
    """is_max of the batch calls a shape is tested with."""
    return (False,) if shape == WIDE_EQ else (True, False)


def one_problem(rng, m, me, nv, nfree):
    """Integer arrays of one LP. The equalities hold at a point xs (non-negative but for the free variables), moved off it
    by a 0/1 vector one time in four."""
    A = rng.integers(-3, 4, size=(m, nv))
    b = rng.integers(-4, 10, size=m)
    xs = rng.integers(0, 4, size=nv)
    xs[:nfree] = rng.integers(-3, 4, size=nfree)
    Ae = rng.integers(-2, 3, size=(me, nv))
    be = Ae @ xs
    if rng.random() < 0.25:
        be = be + rng.integers(0, 2, size=me)
    c = rng.integers(-2, 6, size=nv)
    leq = np.concatenate([A, b[:, None]], axis=1).astype(np.int32)
    eq = np.concatenate([Ae, be[:, None]], axis=1).astype(np.int32)
    tgtf = np.concatenate([c, [0]]).astype(np.int32)
    return tgtf, eq, leq, xs


def wide_eq_problem(rng):
    """one_problem of WIDE_EQ with columns 0 and 1 made private to equalities 65 and 64; the constants are the equalities at
    xs again, so the 66 of them stay consistent."""
    m, me, nv, nfree = WIDE_EQ
    tgtf, eq, leq, xs = one_problem(rng, m, me, nv, nfree)
    for col, row in ((0, 65), (1, 64)):
        keep = eq[row, col] if eq[row, col] != 0 else 1
        eq[:, col] = 0
        eq[row, col] = keep
    eq[:, nv] = eq[:, :nv] @ xs
    return tgtf, eq, leq, xs


_problem_cache = {}


def shape_arrays(shape, kind, count=None):
    """(tgtf [count, cols(,2)], vc [nv, cols(,2)], eq [count, eq_rows, cols(,2)] or None, leq [count, leq_rows, cols(,2)] or None)."""
    m, me, nv, nfree = shape
    count = cases_of(shape) if count is None else count
    if shape not in _problem_cache:
        rng = np.random.default_rng(6100 + 10 * nv + nfree)
        make = (lambda: wide_eq_problem(rng)) if shape == WIDE_EQ else (lambda: one_problem(rng, m, me, nv, nfree))
        probs = [make() for _ in range(cases_of(shape))]
        tg = gen.to_rat(np.stack([p[0] for p in probs]))
        eq = gen.to_rat(np.stack([p[1] for p in probs])) if me else None
        leq = gen.to_rat(np.stack([p[2] for p in probs])) if m else None
        vc = gen.to_rat(gen.vc_nonneg(nv, False, range(nfree)))
        for a in (tg, eq, leq, vc):
            if a is not None:
                a.setflags(write=False)
        _problem_cache[shape] = (tg, vc, eq, leq)
    tg, vc, eq, leq = _problem_cache[shape]
    cut = lambda a: None if a is None else a[:count]
    if kind == F64:
        return as_f64(cut(tg)), as_f64(vc), as_f64(cut(eq)), as_f64(cut(leq))
    return cut(tg), vc, cut(eq), cut(leq)


_oracle_cache = {}


def oracle_answers(port, shape, kind, is_max, count=None):
    """[(status, v, sol)] of the first `count` problems of the shape from the CPU restatement, computed once."""
    count = cases_of(shape) if count is None else count
    key = (shape, kind, is_max)
    have = _oracle_cache.setdefault(key, [])
    if len(have) < count:
        tg, vc, eq, leq = shape_arrays(shape, kind)
        solve = lambda i: port.six_solve(kind, is_max, tg[i], vc, None if eq is None else eq[i], None if leq is None else leq[i])
        if shape[3] == 0:
            for i in range(len(have), count):
                have.append(solve(i))
        else:
            with non_strict(port):
                for i in range(len(have), count):
                    have.append(solve(i))
        if shape == WIDE_EQ and kind == RAT and count == cases_of(shape):
            assert sum(a[0] == 0 for a in have) >= 8, [a[0] for a in have]     # a changed seed must not empty the comparison
    return have[:count]


def small_lds_bytes(R, V, kind=F64):
    """small_lds_bytes of batch_kernels.hip.h restated: the LDS arrays of one LP with R rows and V variables. The one term
    that depends on the scalar is the reduction scratch, 16 x sizeof(Cand<S>): value + row index, 16 bytes around a double,
    12 around a rational."""
    Wmax = V + 1 + R + 1
    nmax = Wmax - 1
    pw = (nmax + 31) // 32
    b = R * Wmax * 8 + Wmax * 8 * 3 + ((R + 1) & ~1) * 8 + 16 * (16 if kind == F64 else 12)
    b += nmax * 4 * 3 + R * 4 + nmax * pw * 4 + 16 * 4 + 8 * 4 + ((nmax + 3) & ~3) * 2
    return (b + 15) & ~15


def plan_bytes(leq_rows, eq_rows, nv, nfree, is_max, kind=F64):
    """LDS bytes of the largest normal form of a shape: leq_rows + 2 eq_rows inequalities, nv + nfree variables; minm solves
    the dual, so rows and variables swap."""
    rows, n = leq_rows + 2 * eq_rows, nv + nfree
    return small_lds_bytes(rows, n, kind) if is_max else small_lds_bytes(n, rows, kind)


def dense_square(nv, count=4, seed=6400):
    """fp64, dense positive: nv inequalities over nv variables, A in [1,9], b in [nv,5nv], c in [1,9], one equality x0 - x1 = 0.
    Returns (tgtf [count, cols], vc, eq [count, 1, cols], leq [count, nv, cols])."""
    rng = np.random.default_rng(seed)
    leq = np.zeros((count, nv, nv + 1)); eq = np.zeros((count, 1, nv + 1)); tg = np.zeros((count, nv + 1))
    for b in range(count):
        leq[b, :, :nv] = rng.integers(1, 10, size=(nv, nv))
        leq[b, :, nv] = rng.integers(nv, 5 * nv + 1, size=nv)
        tg[b, :nv] = rng.integers(1, 10, size=nv)
        eq[b, 0, 0] = 1; eq[b, 0, 1] = -1
    return tg, gen.vc_nonneg(nv, True), eq, leq


def plan_view(vc, kind, leq_rows, eq_rows, is_max, vc_rows=None):
    """xpg_test_six_batch_vc_plan (host only): (rc, [device route, free variables, rows, variables, LDS bytes])."""
    import ctypes as C
    from xpoly_amd import build, _capi
    build.build()
    nv = vc.shape[0]
    a = np.ascontiguousarray(vc, dtype=np.float64) if kind == F64 else gen.to_rat(vc)
    out = (C.c_longlong * 5)(*([-99] * 5))
    rc = _capi.lib().xpg_test_six_batch_vc_plan(C.c_int(kind), a.ctypes.data_as(C.c_void_p), C.c_int(nv if vc_rows is None else vc_rows),
                                                C.c_int(leq_rows), C.c_int(eq_rows), C.c_int(nv + 1), C.c_int(int(is_max)), out, C.c_int(5))
    return rc, [int(x) for x in out]


def largest_square(is_max, eq_rows=1, nfree=0, kind=F64):
    """The largest nv for which nv inequalities over nv variables (and eq_rows equalities) fit 64 KB, by the restated formula."""
    nv = 2
    while plan_bytes(nv + 1, eq_rows, nv + 1, nfree, is_max, kind) <= 64 * 1024:
        nv += 1
    return nv
