"""Seeded, tiny case families for the warm-started branch and bound, shared by the batch and the single-tree tests and by the
host tests that hold the two exact references (tests/warm_mip_ref.py) against each other.

Every number is an integer, or k + 1/2 in b; |a_ij| <= 5 and at most 4 rows of a case are not unit rows, so every minor of A
is below 10^4 and a fractional vertex coordinate is at least about 5e-5 from an integer: 50 times the kernel's int_tol of
1e-6, so rounding a returned point is never ambiguous.

A case is kept only where exact_bb's deepest path is at most half of the depth_cap its launch gets (the kernel may choose
another of several equal optima and walk a little deeper): outside `deep`'s large U no tree may end XPG_ERR_UNSUPPORTED.
"""
import ctypes as C
import random
from collections import namedtuple
from fractions import Fraction

import numpy as np

import warm_mip_ref as ref

Case = namedtuple("Case", "family name c A b is_bin")
Want = namedtuple("Want", "status optimum deepest root by")

HALF = Fraction(1, 2)
BOX_LIMIT = 3000                                             # points brute enumerates per case, at most
GEOMETRY_FIELDS = ("lds", "refused", "depth_cap", "mcap", "wcap", "snap_stride", "tree_stride", "chunk", "launches")


def geometry(rows, cols, is_bin, nb=1):
    """xpg_test_warm_batch_geometry (host only, no device): what xpg_mip_warm_batch_f64 launches with."""
    from xpoly_amd import _capi
    out = (C.c_longlong * 9)()
    rc = _capi.lib().xpg_test_warm_batch_geometry(C.c_int(rows), C.c_int(cols), C.c_int(int(is_bin)), C.c_int(nb), out, C.c_int(9))
    assert rc == 0, rc
    return dict(zip(GEOMETRY_FIELDS, [int(x) for x in out]))


def depth_cap(case):
    return geometry(len(case.A), len(case.c) + 1, case.is_bin)["depth_cap"]


def arrays(cases):
    """(tgtf [nb, cols], leq [nb, rows, cols]) in fp64: every number of a case is exact there."""
    tg = np.array([[float(v) for v in k.c] + [0.0] for k in cases])
    leq = np.array([[[float(v) for v in row] + [float(bi)] for row, bi in zip(k.A, k.b)] for k in cases])
    return tg, leq


_solved = {}


def solved(case, is_max):
    """(exact_bb's answer, brute's answer or None where the box cannot be enumerated), computed once."""
    key = (case.name, bool(is_max))
    if key not in _solved:
        bb = ref.exact_bb(case.c, case.A, case.b, is_max)
        br = None
        if bb.root != "unbounded" and ref.enumerable(case.A, case.b, case.is_bin, BOX_LIMIT):
            br = ref.brute(case.c, case.A, case.b, case.is_bin, is_max)
        _solved[key] = (bb, br)
    return _solved[key]


def want(case, is_max):
    """The exact answer: brute's wherever the box can be enumerated, exact_bb's elsewhere; the depth is exact_bb's."""
    bb, br = solved(case, is_max)
    if br is not None:
        return Want(br.status, br.optimum, bb.deepest, bb.root, "brute")
    return Want(bb.status, bb.optimum, bb.deepest, bb.root, "exact_bb")


def shallow(case, senses=(True, False)):
    """The condition of retention: at most half of the launch's depth_cap, in every sense the case runs in."""
    cap = depth_cap(case)
    return all(2 * want(case, s).deepest <= cap for s in senses)


def _unit_rows(n0):
    return [[int(i == j) for j in range(n0)] for i in range(n0)], [1] * n0


def _pad(A, b, rows):
    """Up to `rows` rows by repeating the rows there are (duplicate rows: ties in the leaving row's arg-min)."""
    k = len(A)
    assert k <= rows
    return A + [list(A[i % k]) for i in range(rows - k)], b + [b[i % k] for i in range(rows - k)]


def _mixed_one(rng, n0, m0, is_bin):
    groups = 1 if (m0 == 1 or n0 == 1 or rng.random() < 0.5) else 2
    cut = rng.randint(1, n0 - 1) if groups == 2 else n0
    A, b = [], []
    for g in range(groups):
        members = range(0, cut) if g == 0 else range(cut, n0)
        A.append([rng.randint(1, 5) if j in members else 0 for j in range(n0)])
        b.append(rng.randint(2, 9) + (HALF if rng.random() < 0.4 else 0))
    for _ in range(m0 - groups):
        A.append([rng.choice((-5, -3, -2, -1, 0, 0, 0, 1, 2, 3, 4, 5)) for _ in range(n0)])
        kind = rng.choice(("pos", "zero", "neg", "half"))
        b.append({"pos": rng.randint(1, 8), "zero": 0, "neg": -rng.randint(1, 3), "half": rng.randint(0, 6) + HALF}[kind])
    if m0 - groups >= 1 and rng.random() < 0.3:              # a duplicate row
        src = rng.randrange(m0 - 1)
        A[-1], b[-1] = list(A[src]), b[src]
    c = [rng.choice((-6, -4, -3, -1, 0, 0, 1, 2, 3, 5, 6)) for _ in range(n0)]
    if n0 >= 2 and rng.random() < 0.3:                       # a duplicate column
        j, k = rng.sample(range(n0), 2)
        for row in A:
            row[k] = row[j]
        c[k] = c[j]
    if is_bin:
        ua, ub = _unit_rows(n0)
        A, b = A + ua, b + ub
    return c, A, b


def mixed(n0, m0, is_bin, count, rows=None):
    """`count` retained cases of n0 variables and m0 rows that are not unit rows (rows: padded to that many by duplicates)."""
    out, seed = [], 0
    while len(out) < count:
        rng = random.Random("mixed %d %d %d %d" % (n0, m0, is_bin, seed))
        c, A, b = _mixed_one(rng, n0, m0, is_bin)
        if rows is not None:
            A, b = _pad(A, b, rows)
        k = Case("mixed", "mixed-%d-%d-%d-s%d" % (n0, len(A), is_bin, seed), c, A, b, int(is_bin))
        seed += 1
        assert seed < 40 * count + 200, "the generator retains too few cases"
        if not ref.enumerable(A, b, is_bin, BOX_LIMIT) or not shallow(k):
            continue
        out.append(k)
    return out


def integral_root(n0, rows, count):
    """Interval matrices (consecutive ones in every row: totally unimodular) with integer b >= 0: the relaxation's vertices
    are integral, the root is the answer."""
    out = []
    for seed in range(count):
        rng = random.Random("tu %d %d %d" % (n0, rows, seed))
        A, b = [[1] * n0], [rng.randint(1, 4)]
        for _ in range(rows - 1):
            lo = rng.randrange(n0)
            hi = rng.randint(lo, n0 - 1)
            A.append([int(lo <= j <= hi) for j in range(n0)])
            b.append(rng.randint(0, 3))
        c = [rng.randint(-6, 6) for _ in range(n0)]
        out.append(Case("integral_root", "tu-%d-%d-s%d" % (n0, rows, seed), c, A, b, 0))
    return out


def unbounded(n0, rows):
    """x_0 has c_0 > 0 and no positive entry in its column; the others sit under a capacity row. The second case carries
    -x_1 <= -1, which the root has to repair before it can see the ray."""
    assert n0 >= 2 and rows >= 3
    cap = [0] + [2] * (n0 - 1)
    A1, b1 = _pad([cap, [-1] + [1] * (n0 - 1), [0] * n0], [7, 2, 0], rows)
    A2, b2 = _pad([cap, [-2] + [1] * (n0 - 1), [0, -1] + [0] * (n0 - 2)], [7, 3, -1], rows)
    c = [3] + [1] * (n0 - 1)
    return [Case("unbounded", "ray-%d-%d" % (n0, rows), c, A1, b1, 0), Case("unbounded", "ray-repair-%d-%d" % (n0, rows), c, A2, b2, 0)]


def root_infeasible(n0, rows):
    """sum a_j x_j <= -1 with every a_j >= 0: phase one ends without an entering column. And 2 x_0 = 1 inside a box: the
    relaxation is feasible, no integer point is."""
    assert n0 >= 2 and rows >= 4
    A1, b1 = _pad([[3] * n0, [1, 2] + [0] * (n0 - 2)], [9, -1], rows)
    A2, b2 = _pad([[2] + [0] * (n0 - 1), [-2] + [0] * (n0 - 1), [1] * n0, [0, 1] + [0] * (n0 - 2)], [1, -1, 3, 3], rows)
    c = [1] * n0
    return [Case("root_infeasible", "phase-one-%d-%d" % (n0, rows), c, A1, b1, 0), Case("root_infeasible", "two-x-is-one-%d-%d" % (n0, rows), c, A2, b2, 0)]


def deep(U):
    """2x - 2y <= 1, -2x + 2y <= -1 (x - y = 1/2), x <= U, y <= U: feasible for the relaxation, no integer point, and a
    path that is the longer the larger U."""
    return Case("deep", "deep-U%d" % U, [1, 1], [[2, -2], [-2, 2], [1, 0], [0, 1]], [1, -1, U, U], 0)


DEEP_SMALL_U, DEEP_LARGE_U = 2, 14          # exact_bb's deepest path: at most 6 / more than 24 (depth_cap = 2 * 2 + 8 = 12)
TRIVIAL = Case("mixed", "trivial-2-4", [1, 1], [[1, 0], [0, 1], [1, 0], [0, 1]], [1, 1, 1, 1], 0)


def wide_n0():
    """The most variables of a general integer program of two rows that still gets depth_cap >= 12."""
    n0 = 257
    while geometry(2, n0 + 2, 0)["depth_cap"] >= 12:
        n0 += 1
    return n0


def wide_active(n0):
    return [0, 63, 64, 255, 256, n0 - 1]


WIDE_SEEDS = (0, 1, 2, 5, 7, 8, 9, 11)      # chosen on the CPU: exact_bb's deepest path <= 6 = depth_cap / 2 (asserted by the host test)


def wide(n0, seeds=WIDE_SEEDS, active=None):
    """Two rows, n0 general integers, six of them `active` (c_j > 0); every other column has A >= 0 and c_j <= 0, so that
    setting it to zero never lowers the optimum of the maximisation: the optimum is brute's over the six. The other columns
    cost strictly less than nothing (c_j < 0): several hundred columns of cost zero, many of them equal, span a face of
    equally good vertices through which ANY branch and bound that meets one of them fractional can be led one bound row per
    column, so that exact_bb's depth would say nothing about another walk's, however it is halved."""
    active = wide_active(n0) if active is None else active
    out = []
    for seed in seeds:
        rng = random.Random("wide %d %d" % (n0, seed))
        A = [[rng.choice((0, 0, 0, 1, 2, 3)) for _ in range(n0)] for _ in range(2)]
        c = [-rng.choice((1, 1, 2, 3, 4, 6)) for _ in range(n0)]
        for j in active:
            A[0][j] = rng.randint(2, 5); A[1][j] = rng.randint(0, 5); c[j] = rng.randint(1, 6)
        b = [rng.randint(5, 9) + HALF * rng.randint(0, 1), rng.randint(4, 9)]
        out.append(Case("wide", "wide-%d-s%d" % (n0, seed), c, A, b, 0))
    return out


def wide_want(case, active):
    """brute over the active variables alone."""
    return ref.brute([case.c[j] for j in active], [[row[j] for j in active] for row in case.A], case.b, False, True)


def lds_edge_n0():
    """The most 0-1 variables of a knapsack of two capacity rows (plus its x_j <= 1 rows) whose LDS block keeps the full
    depth_cap = n0 + 2."""
    n0 = 8
    while geometry(n0 + 3, n0 + 2, 1)["depth_cap"] == n0 + 3:
        n0 += 1
    return n0


EDGE_SEEDS = (0, 1, 11)                      # chosen on the CPU: at most 60 nodes and a deepest path <= (n0 + 2) / 2 for exact_bb


def lds_edge(n0, seeds=EDGE_SEEDS):
    """Real 0-1 knapsacks of two capacity rows at the largest LDS block; too wide to enumerate: the reference is exact_bb."""
    out = []
    for seed in seeds:
        rng = random.Random("edge %d %d" % (n0, seed))
        A = [[rng.randint(1, 5) for _ in range(n0)] for _ in range(2)]
        c = [rng.randint(1, 6) for _ in range(n0)]
        b = [sum(A[0]) // 2 + HALF, sum(A[1]) * 2 // 3]
        ua, ub = _unit_rows(n0)
        out.append(Case("lds_edge", "edge-%d-s%d" % (n0, seed), c, A + ua, b + ub, 1))
    return out


def refusal_rows():
    """Two general integers: the most rows xpg_mip_warm_batch_f64 still takes (the shrinking loop ends at depth 4)."""
    m0 = 8
    while not geometry(m0 + 1, 3, 0)["refused"]:
        m0 += 1
    return m0


def tall(rows):
    """Two variables under `rows` rows that repeat four: every ratio test is a tie of some twenty rows."""
    A, b = _pad([[2, 1], [1, 3], [1, 0], [0, 1]], [5, 7 + HALF, 2, 2], rows)
    return Case("tall", "tall-%d" % rows, [3, 2], A, b, 0)


MIXED_SHAPES = ((1, 2, 0), (2, 1, 0), (3, 2, 1), (5, 4, 0), (6, 3, 1), (6, 4, 0))       # (n0, rows that are not unit rows, 0-1)
CYCLE_SHAPE = (4, 3, 0)                                                      # the 64-problem set that is cycled to 257

_memo = {}


def memo(fn, *a):
    key = (fn.__name__,) + a
    if key not in _memo:
        _memo[key] = fn(*a)
    return _memo[key]
