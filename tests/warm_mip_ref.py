"""Exact references for the warm-started branch and bound (xpg_mip_warm_f64, xpg_mip_warm_batch_f64):
    maximise (minimise) c . x   subject to   A x <= b,  x >= 0,  x integer.
Plain Python on int and fractions.Fraction: no numpy float, no scipy. c and A are integers, b integers or half-integers.

brute     enumerates the integer box that the rows with no negative coefficient span.
exact_bb  is a textbook branch and bound: every node is the root's rows plus its path's bound rows, solved from the slack
          form by a dual simplex (to a feasible basis) and a primal simplex, both under Bland's rule, in exact arithmetic;
          depth first, lowest fractional variable, floor child first, pruned by the incumbent. Not the kernel's rules (most
          negative constant, Dantzig's column, warm starts): the two share only the mathematics.
"""
import itertools
from collections import namedtuple
from fractions import Fraction

SUCC, UNBOUND, NO_SOL = 0, 1, 2          # XPG_IP_SUCC, XPG_IP_UNBOUND, XPG_IP_NO_PRI_FEASIBLE_SOL

Brute = namedtuple("Brute", "status optimum points")
BB = namedtuple("BB", "status optimum deepest root nodes point")


def box(A, b, is_bin=False):
    """Upper bounds of the integer box from the rows whose coefficients are all >= 0 (None for a variable no such row
    holds); an empty list when such a row has a negative constant (no point at all)."""
    n = len(A[0])
    ub = [None] * n
    for row, bi in zip(A, b):
        if any(a < 0 for a in row) or not any(a > 0 for a in row):
            continue
        if bi < 0:
            return []
        for j, a in enumerate(row):
            if a > 0:
                assert (2 * Fraction(bi)).denominator == 1, "b must be an integer or a half-integer"
                u = (2 * Fraction(bi)).numerator // (2 * a)
                ub[j] = u if ub[j] is None else min(ub[j], u)
    if is_bin:
        ub = [None if u is None else min(u, 1) for u in ub]
    return ub


def enumerable(A, b, is_bin=False, limit=200000):
    ub = box(A, b, is_bin)
    if ub == []:
        return True
    if any(u is None for u in ub):
        return False
    size = 1
    for u in ub:
        size *= u + 1
    return size <= limit


def brute(c, A, b, is_bin, is_max=True):
    """(status, exact optimum, list of optimal points) by enumeration; every variable needs a bounding row."""
    ub = box(A, b, is_bin)
    if ub == []:
        return Brute(NO_SOL, None, [])
    assert all(u is not None for u in ub), "a variable without a bounding row: not enumerable"
    A2 = [[2 * a for a in row] for row in A]
    b2 = [(2 * Fraction(bi)).numerator for bi in b]
    best, points = None, []
    for x in itertools.product(*[range(u + 1) for u in ub]):
        if any(sum(a * xj for a, xj in zip(row, x)) > bi for row, bi in zip(A2, b2)):
            continue
        v = sum(cj * xj for cj, xj in zip(c, x))
        if best is None or (v > best if is_max else v < best):
            best, points = v, [x]
        elif v == best:
            points.append(x)
    if best is None:
        return Brute(NO_SOL, None, [])
    return Brute(SUCC, best, points)


def _pivot(T, z, basis, r, e):
    p = T[r][e]
    T[r] = [v / p for v in T[r]]
    pr = T[r]
    nz = [j for j, v in enumerate(pr) if v != 0]
    for i, row in enumerate(T):
        if i != r and row[e] != 0:
            f = row[e]
            for j in nz:
                row[j] -= f * pr[j]
    if z is not None and z[e] != 0:
        f = z[e]
        for j in nz:
            z[j] -= f * pr[j]
    basis[r] = e


def lp(c, A, b):
    """maximise c . x over A x <= b, x >= 0, exactly: ('optimal', value, x) | ('infeasible',) | ('unbounded',)."""
    m, n = len(A), len(c)
    T = [[Fraction(v) for v in A[i]] + [Fraction(int(i == k)) for k in range(m)] + [Fraction(b[i])] for i in range(m)]
    basis = [n + i for i in range(m)]
    for _ in range(100000):                                  # to a feasible basis: dual simplex, zero objective, Bland
        neg = [(basis[i], i) for i in range(m) if T[i][-1] < 0]
        if not neg:
            break
        r = min(neg)[1]
        ent = [j for j in range(n + m) if T[r][j] < 0]
        if not ent:
            return ("infeasible",)
        _pivot(T, None, basis, r, ent[0])
    else:
        raise RuntimeError("phase one did not end")
    cc = [Fraction(v) for v in c] + [Fraction(0)] * m
    z = [sum(cc[basis[i]] * T[i][j] for i in range(m)) - (cc[j] if j < n + m else 0) for j in range(n + m + 1)]
    for _ in range(100000):                                  # primal simplex, Bland
        ent = [j for j in range(n + m) if z[j] < 0]
        if not ent:
            break
        e = ent[0]
        rows = [(T[i][-1] / T[i][e], basis[i], i) for i in range(m) if T[i][e] > 0]
        if not rows:
            return ("unbounded",)
        _pivot(T, z, basis, min(rows)[2], e)
    else:
        raise RuntimeError("phase two did not end")
    x = [Fraction(0)] * n
    for i in range(m):
        if basis[i] < n:
            x[basis[i]] = T[i][-1]
    return ("optimal", z[-1], x)


def exact_bb(c, A, b, is_max=True, node_limit=20000):
    """(status, exact optimum, deepest path, the root relaxation's verdict, nodes, an optimal point). The deepest path
    counts the bound rows of the deepest node that was solved, feasible or not."""
    n = len(c)
    cc = list(c) if is_max else [-v for v in c]
    root = lp(cc, A, b)
    if root[0] == "infeasible":
        return BB(NO_SOL, None, 0, "infeasible", 0, None)
    if root[0] == "unbounded":
        return BB(UNBOUND, None, 0, "unbounded", 0, None)
    best, best_x, deepest, nodes = None, None, 0, 0
    stack = [([], [], root)]                                 # bound rows, their constants, the solved relaxation
    while stack:
        rows, rhs, sol = stack.pop()
        nodes += 1
        assert nodes <= node_limit, "exact_bb: too many nodes"
        value, x = sol[1], sol[2]
        if best is not None and value <= best:
            continue
        frac = [j for j in range(n) if x[j].denominator != 1]
        if not frac:
            best, best_x = value, [int(v) for v in x]
            continue
        j = frac[0]
        lo = x[j].numerator // x[j].denominator
        kids = []
        for sign, d in ((1, lo), (-1, -(lo + 1))):
            row = [0] * n
            row[j] = sign
            deepest = max(deepest, len(rows) + 1)
            child = lp(cc, A + rows + [row], list(b) + rhs + [d])
            assert child[0] != "unbounded"
            if child[0] == "optimal":
                kids.append((rows + [row], rhs + [d], child))
        stack.extend(reversed(kids))                          # the floor child is taken up first
    if best is None:
        return BB(NO_SOL, None, deepest, "optimal", nodes, None)
    return BB(SUCC, best if is_max else -best, deepest, "optimal", nodes, best_x)
