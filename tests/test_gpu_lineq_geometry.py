"""The row-elimination kernels (lineq_kernels.hip.h) at every launch geometry the host code can choose, each case checked three
ways: bit for bit against Port (our C++ restatement), bit for bit against the real reference when oracle/_ref/ is built, and
against exact arithmetic (stdlib fractions / Python ints) wherever the reference's Rational never took its float32 rescue.

The case table is derived from a Python mirror of the launch rules (lineq_geom, the Gauss width rule and the LDS formulas of
lineq_host.hip.h / ctx.hip.h); test_case_table_covers_every_launch_branch checks without a GPU that the table reaches every
(lanes per system, systems per wave) pair each entry point can take, a system above 64 KB of LDS, the largest accepted shape
and the first refused one."""
import math
import zlib
from collections import namedtuple
from fractions import Fraction

import numpy as np
import pytest

from tools import gen

XPG_ERR_REF_UNDEFINED = -7
LDS_MAX, LDS_WAVE = 160 * 1024, 64 * 1024


# ---- mirror of the host launch rules ------------------------------------------------------------------------------------
def _r16(x):
    return (x + 15) & ~15


def lineq_geom(nb, width, sys_lds):
    """ctx.hip.h lineq_geom: (L lanes per system, G systems per wave, workgroups in the grid)."""
    L = 16 if width <= 16 else (32 if width <= 32 else 64)
    sys_lds = _r16(sys_lds)
    while L < 64 and sys_lds * (64 // L) > LDS_WAVE:
        L *= 2
    G = 64 // L
    return L, G, min((nb + G - 1) // G, 4096)


def lineq_lds_bytes(cap, cols):
    b = cap * cols * 8 + (cap + 1) * 4 + 16 + ((cap + 1) & ~1) * 4 + ((cap + 3) & ~3)
    return _r16(b)


def fme_lds(cap, cap_in, cols):
    capx = max(cap, cap_in)
    scratch = lineq_lds_bytes(capx, cols) - capx * cols * 8 + 16
    tmp = cap_in * cols * 8
    full = cap * cols * 8 + tmp + scratch
    if full <= 12 * 1024:
        return full
    cap_lds = min((cap_in + cols - 1) // cols, cap)
    return cap_lds * cols * 8 + tmp + scratch


GAUSS_OP = {"rank": 0, "det": 1, "inv": 2, "basis": 3, "null": 4}


def fme_cap(rows):
    """lineq_fme_batch_packed's default cap_rows (Lineq.fme passes none)."""
    return max(rows, rows * rows // 4 + rows + 1)


def calc_cap(rows, cap_rows):
    return cap_rows or max(16, rows * rows)          # Lineq.calcBound's default


def launch(entry, rows, cols, nb=1, cap_rows=None):
    """(L, G, grid, lds of one system) of a call, or None where the host refuses it (XPG_ERR_UNSUPPORTED)."""
    if entry in GAUSS_OP:                                               # gauss_batch
        op = GAUSS_OP[entry]
        lds = _r16(rows * cols * 8 * (2 if op == 2 else 1)) + _r16(rows * 13)
        if lds > LDS_MAX:
            return None
        width = 64 if rows * cols > 256 else (2 * cols if op == 2 else cols)
        return lineq_geom(nb, width, lds) + (lds,)
    if entry == "hnf":                                                  # int_hnf_batch: one 64-lane wave per matrix
        lds = _r16((rows + cols) * cols * 4)
        return None if lds > LDS_MAX else (64, 1, min(nb, 4096), lds)
    if entry == "gcd":                                                  # k_int_gcd_batch: one thread per row, no LDS
        return (1, 256, (nb * rows + 255) // 256, 0)
    if entry in ("reduce", "iden"):                                     # lineq_reduce_batch_dev
        lds = lineq_lds_bytes(rows, cols)
        if lds > LDS_MAX or rows > 32767:
            return None
        return lineq_geom(nb, max(rows, cols), lds) + (lds,)
    if entry == "fme":                                                  # lineq_fme_batch_dev, the whole wave
        cap = fme_cap(rows)
        lds = fme_lds(cap, rows, cols)
        return None if lds > LDS_MAX or cap > 32767 else lineq_geom(nb, 64, lds) + (lds,)
    if entry == "calc":                                                 # lineq_calc_bound_batch
        cap = calc_cap(rows, cap_rows)
        lds = fme_lds(cap, cap, cols)
        return None if lds > LDS_MAX or cap > 32767 else lineq_geom(nb, 64, lds) + (lds,)
    raise KeyError(entry)


# the family of shapes along which "largest accepted" / "first refused" is taken: k -> (rows, cols, cap_rows)
FAMILY = {
    "rank": lambda k: (k, k, None), "det": lambda k: (k, k, None), "inv": lambda k: (k, k, None),
    "basis": lambda k: (k, k, None), "null": lambda k: (k, k, None), "hnf": lambda k: (k, k, None),
    "reduce": lambda k: (k, 17, None), "iden": lambda k: (k, 17, None),
    "fme": lambda k: (k, 17, None), "calc": lambda k: (6, 4, k),
}
LDS_ENTRIES = tuple(FAMILY)


def largest_accepted(entry):
    def ok(k):
        rows, cols, cap = FAMILY[entry](k)
        return launch(entry, rows, cols, cap_rows=cap) is not None
    k = 8
    while ok(k * 2):
        k *= 2
    hi = k * 2
    while hi - k > 1:                                                   # ok(k), not ok(hi)
        mid = (k + hi) // 2
        k, hi = (mid, hi) if ok(mid) else (k, mid)
    return k


# ---- the case table -----------------------------------------------------------------------------------------------------
# entry, label (the branch it is meant to hit), rows, cols, nb, input kind, extra (calcBound's cap_rows, else None)
Case = namedtuple("Case", "entry label rows cols nb kind extra")


def _cases():
    c = []
    add = lambda *a: c.append(Case(*a))
    R = {e: largest_accepted(e) for e in LDS_ENTRIES}
    # rank: widths 1, 15/16/17, 31/32/33, 63/64/65, > 100; both sides of 256 cells; rows > 64 and > 128
    for rows, cols, lab in ((8, 1, "w1"), (200, 1, "w1 rows>128"), (12, 15, "w15"), (16, 16, "w16 at 256"),
                            (15, 17, "w17"), (8, 31, "w31"), (8, 32, "w32"), (7, 33, "w33"), (17, 16, "257+ cells"),
                            (4, 63, "w63"), (4, 64, "w64"), (3, 65, "w65 column lanes"), (20, 65, "w65 cells"),
                            (10, 120, "w120"), (80, 9, "rows>64"), (150, 12, "rows>128"), (96, 96, "lds>64K")):
        add("rank", lab, rows, cols, 64 if rows * cols <= 2048 else 8, "mix", None)
    add("rank", "largest", R["rank"], R["rank"], 2, "blocks", None)
    add("rank", "refused", R["rank"] + 1, R["rank"] + 1, 1, "zero", None)
    add("rank", "grid stride", 4, 4, 4096 * 4 + 37, "rand4", None)
    add("rank", "wave packing", 4, 4, 64 + 3, "packing", None)
    # det and inv: n x n, inv on the n x 2n augmented matrix
    for n, lab in ((4, "n4"), (16, "n16"), (17, "n17 cells"), (24, "n24"), (40, "n40"), (70, "rows>64"), (96, "lds>64K")):
        add("det", lab, n, n, 16 if n <= 24 else 4, "mix", None)
    add("det", "largest", R["det"], R["det"], 2, "ublocks", None)
    add("det", "refused", R["det"] + 1, R["det"] + 1, 1, "zero", None)
    add("det", "wave packing", 4, 4, 64 + 3, "packing", None)
    for n in (6, 7, 10):                               # the sign quirk at n = 2 and 3 mod 4, both anti-triangular forms
        add("det", "anti-triangular zeros above n%d" % n, n, n, 3, "anti", None)
    for n in (6, 7):
        add("det", "anti-triangular zeros below n%d" % n, n, n, 3, "anti2", None)
    for n, lab in ((7, "2n=14"), (8, "2n=16"), (9, "2n=18"), (16, "2n=32"), (17, "2n=34 cells"), (32, "2n=64"),
                   (33, "2n=66"), (48, "2n=96"), (70, "lds>64K")):
        add("inv", lab, n, n, 16 if n <= 17 else 4, "mix", None)
    add("inv", "largest", R["inv"], R["inv"], 2, "unimod", None)
    add("inv", "refused", R["inv"] + 1, R["inv"] + 1, 1, "zero", None)
    add("inv", "wave packing", 3, 3, 64 + 3, "packing", None)
    # rank with basis, null space
    for e in ("basis", "null"):
        for rows, cols, lab in ((7, 7, "w7"), (8, 31, "w31"), (12, 22, "cells"), (40, 17, "rows>32"), (80, 20, "rows>64"),
                                (130, 10, "rows>128"), (10, 70, "w70"), (96, 96, "lds>64K")):
            add(e, lab, rows, cols, 24 if rows * cols <= 4096 else 4, "mix", None)
        add(e, "largest", R[e], R[e], 1, "blocks", None)
        add(e, "refused", R[e] + 1, R[e] + 1, 1, "zero", None)
        add(e, "wave packing", 4, 4, 64 + 3, "packing", None)
    # HNF: rows + cols stacked, one 64-lane wave
    for rows, cols, lab in ((8, 8, "8x8"), (20, 20, "stack 40"), (40, 30, "stack>64"), (120, 12, "stack>128"),
                            (70, 70, "stack>128 square"), (670, 24, "lds>64K"), (100, 100, "lds>64K square")):
        add("hnf", lab, rows, cols, 8 if rows * cols <= 1600 else 2, "int", None)
    add("hnf", "largest", R["hnf"], R["hnf"], 1, "int", None)
    add("hnf", "refused", R["hnf"] + 1, R["hnf"] + 1, 1, "zero", None)
    add("hnf", "cols>rows negative diagonal", 4, 6, 4, "negdiag", None)
    add("gcd", "w70 rows%256", 10, 70, 37, "gcd", None)
    add("gcd", "w130 many rows", 3, 130, 300, "gcd", None)
    # reduce / removeIdenRow / fme / calcBound
    for e in ("reduce", "iden", "fme"):
        for rows, cols, lab in ((12, 9, "w9"), (20, 17, "w17"), (30, 33, "w33"), (40, 65, "w65"), (50, 80, "w80"),
                                (90, 12, "rows>64"), (140, 12, "rows>128")):
            add(e, lab, rows, cols, 12, "bounds", None)
        if e != "fme":
            add(e, "lds>64K", 500, 17, 2, "bounds", None)
            add(e, "wave packing", 10, 9, 64 + 3, "bounds", None)
        else:
            add(e, "lds>64K", 160, 17, 2, "bounds", None)
        add(e, "largest", R[e], 17, 1, "bounds", None)
        add(e, "refused", R[e] + 1, 17, 1, "bounds", None)
    for rows, cols, lab in ((12, 17, "w17"), (16, 33, "w33"), (20, 65, "w65"), (24, 80, "w80")):
        add("calc", lab, rows, cols, 2, "bounds", 4 * rows + 16)
    add("calc", "rows>64", 70, 5, 2, "bounds", 4 * 70 + 16)
    add("calc", "rows>128", 130, 5, 1, "bounds", 4 * 130 + 16)
    add("calc", "lds>64K", 6, 4, 2, "bounds", 1600)
    add("calc", "largest", 6, 4, 2, "bounds", R["calc"])
    add("calc", "refused", 6, 4, 1, "bounds", R["calc"] + 1)
    return c


CASES = _cases()


def case_facts(cs):
    """What the mirror says this case's launch is: (L, G) or 'refused', above 64 KB, largest, ..."""
    fam_k = {"calc": cs.extra}.get(cs.entry, cs.rows)
    geo = launch(cs.entry, cs.rows, cs.cols, cs.nb, cap_rows=cs.extra if cs.entry == "calc" else None)
    facts = set()
    if geo is None:
        facts.add("refused")
        return facts, None
    L, G, grid, lds = geo
    facts.add((L, G))
    if lds > LDS_WAVE:
        facts.add("over64K")
    if cs.entry in LDS_ENTRIES and tuple(FAMILY[cs.entry](fam_k)[:2]) == (cs.rows, cs.cols) or cs.entry == "calc":
        if fam_k == largest_accepted(cs.entry):
            facts.add("largest")
    if cs.nb > 4096 * G:
        facts.add("grid stride")
    return facts, geo


def reachable_geometries(entry):
    seen = set()
    for rows in list(range(1, 70)) + [100, 140]:
        for cols in list(range(1, 70)) + [100, 140]:
            if (entry == "calc" and cols < 2) or (entry in ("det", "inv") and rows != cols):
                continue
            g = launch(entry, rows, cols, 64, cap_rows=max(rows, 16) if entry == "calc" else None)
            if g is not None:
                seen.add(g[:2])
    return seen


def test_case_table_covers_every_launch_branch():
    """CPU only: every (L, G) an entry point can launch with, a system above 64 KB, the largest accepted and the first
    refused shape are in the table for every entry point with an LDS formula, and every label says what the mirror says."""
    assert (largest_accepted("det"), largest_accepted("inv"), largest_accepted("hnf")) == (142, 100, 143)
    for e in LDS_ENTRIES:
        need = reachable_geometries(e) | {"over64K", "largest", "refused"}
        have = set()
        for cs in CASES:
            if cs.entry == e:
                have |= case_facts(cs)[0]
        assert need <= have, (e, need - have)
    assert any("grid stride" in case_facts(cs)[0] for cs in CASES)
    for cs in CASES:
        facts, geo = case_facts(cs)
        for word, fact in (("refused", "refused"), ("largest", "largest"), ("lds>64K", "over64K"), ("grid stride", "grid stride")):
            if word in cs.label:
                assert fact in facts, cs
        if "cells" in cs.label and cs.entry in GAUSS_OP:
            assert cs.rows * cs.cols > 256 and geo[0] == 64, cs
        if "rows>64" in cs.label or "rows>128" in cs.label:
            assert cs.rows > (128 if "128" in cs.label else 64), cs
        if cs.label.startswith("2n="):
            assert 2 * cs.rows == int(cs.label.split()[0][3:]), cs
        if "wave packing" in cs.label:
            assert geo[1] == 4 and cs.nb % 4 != 0, cs
    # the gcd rows: more than 64 columns, a row total that is not a multiple of 256
    assert any(cs.entry == "gcd" and cs.cols > 64 and (cs.nb * cs.rows) % 256 for cs in CASES)
    assert any(cs.entry == "hnf" and cs.rows + cs.cols > 128 for cs in CASES)


# ---- inputs -------------------------------------------------------------------------------------------------------------
def ptri(rng, rows, cols):
    """Rows of an upper trapezoid (diagonal +-1, a few +-2, small entries right of it), rows shuffled."""
    m = np.triu(rng.integers(-1, 2, size=(rows, cols)), 1)
    k = min(rows, cols)
    m[np.arange(k), np.arange(k)] = rng.choice([1, -1, 1, -1, 2, -2], size=k)
    return m[rng.permutation(rows)]


def unimod(rng, n):
    """A product of elementary integer row operations (row_i += +-row_j) and a permutation: det +-1, integer inverse."""
    m = np.eye(n, dtype=np.int64)[rng.permutation(n)]
    for _ in range(2 * n if n > 1 else 0):
        i, j = rng.choice(n, size=2, replace=False)
        m[i] += rng.choice([-1, 1]) * m[j]
    return m


def blockdiag(rng, rows, cols):
    m = np.zeros((rows, cols), dtype=np.int64)
    i = 0
    while i < min(rows, cols):
        s = min(int(rng.integers(2, 5)), rows - i, cols - i)
        m[i:i + s, i:i + s] = rng.integers(-2, 3, size=(s, s))
        i += s
    return m


def blocks(rng, rows, cols, singular=True):
    """Block diagonal, rows shuffled: blocks of 2 to 4 built by elementary row operations (det +-1), every third one made
    singular (a row the sum of two others) when `singular`: elimination never leaves a block, so it stays exact at any size."""
    m = np.zeros((rows, cols), dtype=np.int64)
    i, k = 0, 0
    while i < min(rows, cols):
        s = min(int(rng.integers(2, 5)), rows - i, cols - i)
        blk = unimod(rng, s)
        if singular and k % 3 == 2 and s > 2:
            blk[-1] = blk[0] + blk[1]
        m[i:i + s, i:i + s] = blk
        i += s; k += 1
    return m[rng.permutation(rows)]


def dependent(rng, rows, cols):
    """Rank-deficient: the rows past the first half are integer combinations of earlier rows."""
    m = ptri(rng, rows, cols)
    for i in range(max(1, rows // 2), rows):
        a, b = rng.integers(0, i, size=2)
        m[i] = m[a] + rng.choice([-1, 1]) * m[b]
    return m


def bounds_system(rng, rows, cols, coupled=True):
    """Single-variable bounds (with duplicates), constant rows and sparse multi-variable rows with a non-negative
    constant: the box around the origin holds points of it, and elimination stays inside int32."""
    nv = cols - 1
    m = np.zeros((rows, cols), dtype=np.int64)
    for i in range(rows):
        t = rng.random()
        if t < 0.5 or not coupled:
            j = int(rng.integers(0, nv)); s = int(rng.choice([-2, -1, 1, 2]))
            m[i, j] = s; m[i, -1] = abs(s) * int(rng.integers(0, 3))
        elif t < 0.6 and i > 0:
            m[i] = m[int(rng.integers(0, i))]
        elif t < 0.65:
            m[i, -1] = int(rng.integers(0, 3))
        else:
            js = rng.choice(nv, size=min(nv, int(rng.integers(2, 4))), replace=False)
            m[i, js] = rng.choice([-2, -1, 1, 2], size=len(js)); m[i, -1] = int(rng.integers(0, 5))
    return m


def hermite_perm(rng, n):
    """A square matrix in Hermite normal form (lower triangular, diagonal 1 or 2, 0 <= h_ij < h_ii left of it) with its
    columns shuffled: its HNF is that form, reached without a value leaving int32 at any size."""
    h = np.zeros((n, n), dtype=np.int64)
    for i in range(n):
        h[i, i] = int(rng.integers(1, 3))
        h[i, :i] = rng.integers(0, h[i, i], size=i)
    return h[:, rng.permutation(n)]


def hermite_of_permuted(a):
    """The Hermite form H0 when the square matrix a is H0 with its columns permuted (column j of H0 is the column whose
    first nonzero is in row j), else None."""
    n, m = a.shape
    if n != m:
        return None
    first = [int(np.flatnonzero(a[:, j])[0]) if np.any(a[:, j]) else -1 for j in range(m)]
    if sorted(first) != list(range(n)):
        return None
    h0 = np.zeros_like(a)
    for j, r in enumerate(first):
        h0[:, r] = a[:, j]
    for i in range(n):
        if h0[i, i] <= 0 or not all(0 <= h0[i, j] < h0[i, i] for j in range(i)):
            return None
    return h0


def make_input(cs, rng):
    r, c, nb = cs.rows, cs.cols, cs.nb
    if cs.kind == "zero":
        return np.zeros((nb, r, c), dtype=np.int64)
    if cs.kind in ("rand4", "int"):
        a = rng.integers(-4 if cs.kind == "rand4" else -2, 5 if cs.kind == "rand4" else 3, size=(nb, r, c))
        if cs.kind == "int" and r == c and c > 40:    # HNF, large squares: Hermite forms with shuffled columns (the restatement
            return np.stack([hermite_perm(rng, c) for _ in range(nb)])     # and the reference stay fast and exact on them)
        if cs.kind == "int":                         # HNF: half of them lower triangular with a positive diagonal, columns shuffled
            for b in range(0, nb, 2):
                t = np.tril(rng.integers(-2, 3, size=(r, c)), -1)
                t[np.arange(min(r, c)), np.arange(min(r, c))] = rng.integers(1, 3, size=min(r, c))
                a[b] = t[:, rng.permutation(c)]
        return a
    if cs.kind == "negdiag":
        a = rng.integers(-2, 3, size=(nb, r, c))
        a[:, 0, :] = 0; a[:, 0, 0] = -1
        return a
    if cs.kind == "gcd":
        a = rng.integers(-9, 10, size=(nb, r, c)) * rng.integers(1, 7, size=(nb, r, 1))
        a[0, 0] = 0
        return a
    if cs.kind in ("anti", "anti2"):                  # zero above (anti) or below (anti2) the anti-diagonal
        tri = np.triu if cs.kind == "anti" else np.tril
        return np.stack([np.flipud(tri(rng.integers(1, 3, size=(r, c))) * rng.choice([-1, 1], size=(r, c)))
                         for _ in range(nb)])
    if cs.kind == "packing":                          # systems of one wave that take different branches
        out = []
        for b in range(nb):
            m = rng.integers(-4, 5, size=(r, c))
            k = b % 5
            if k == 0:
                m[-1] = m[0]                                       # singular
            elif k == 1:
                m[:, 0] = rng.integers(2, 5, size=r); m[1, 0] = 1    # a unit pivot early, after a larger candidate
            elif k == 2:
                m = np.triu(m); m[np.arange(r), np.arange(r)] = 1  # triangular
            out.append(m)
        return np.stack(out)
    if cs.kind == "bounds":                           # (calcBound eliminates every other variable: bounds only, or the chain explodes)
        return np.stack([bounds_system(rng, r, c, coupled=cs.entry != "calc") for b in range(nb)])
    gens = {"ptri": [ptri], "unimod": [lambda g, rr, cc: unimod(g, rr)], "blocks": [blocks],
            "ublocks": [lambda g, rr, cc: blocks(g, rr, cc, singular=False)],
            "mix": [blocks, ptri, blockdiag, dependent, lambda g, rr, cc: g.integers(-4, 5, size=(rr, cc))]}[cs.kind]
    if cs.kind == "mix" and r == c:
        gens = gens + [lambda g, rr, cc: unimod(g, rr)]
    return np.stack([gens[b % len(gens)](rng, r, c) for b in range(nb)])


def rat(a):
    out = gen.to_rat(np.asarray(a, dtype=np.int32))
    return out


def nonpositive_denominators(mats, rng):
    """The wave-packing batch: every fifth system gets a column entry n/-d (the sequential pivot scan)."""
    mats = mats.copy()
    for b in range(3, mats.shape[0], 5):
        i = int(rng.integers(0, mats.shape[1]))
        if mats[b, i, 0, 0] != 0:
            mats[b, i, 0] = (-mats[b, i, 0, 0], -1)
    return mats


# ---- exact arithmetic (Python ints and fractions only) -------------------------------------------------------------------
def frac(m):
    return [[Fraction(int(x[0]), int(x[1])) for x in row] for row in m]


def int_rows(m):
    """[r, c, 2] rationals -> (object int matrix with every row scaled to integers, product of the scales)."""
    f = frac(m)
    out, scale = [], 1
    for row in f:
        s = 1
        for x in row:
            s = s * x.denominator // math.gcd(s, x.denominator)
        out.append([int(x * s) for x in row]); scale *= s
    return np.array(out, dtype=object).reshape(len(f), m.shape[1]), scale


def bareiss(M):
    """Fraction-free elimination on Python ints: (rank, det if square else None)."""
    M = np.array(M, dtype=object)
    n, m = M.shape
    prev, r, sign = 1, 0, 1
    for k in range(m):
        if r == n:
            break
        nz = [i for i in range(r, n) if M[i, k] != 0]
        if not nz:
            continue
        p = nz[0]
        if p != r:
            M[[r, p]] = M[[p, r]]; sign = -sign
        if r + 1 < n:
            M[r + 1:, k + 1:] = (M[r + 1:, k + 1:] * M[r, k] - np.outer(M[r + 1:, k], M[r, k + 1:])) // prev
            M[r + 1:, k] = 0
        prev = M[r, k]; r += 1
    det = None
    if n == m:
        det = sign * M[n - 1, n - 1] if r == n else 0
    return r, det


def exact_rank(m):
    return bareiss(int_rows(m)[0])[0]


def is_anti_triangular(m):
    """Zero above the anti-diagonal (w_tri 2 of lineq_kernels.hip.h) or below it (w_tri 3)."""
    n = m.shape[0]
    return (all(m[i, j, 0] == 0 for i in range(n) for j in range(n - 1 - i)) or
            all(m[i, j, 0] == 0 for i in range(n) for j in range(n - i, n)))


def exact_det(m):
    """The determinant, and what the reference returns: for n >= 4 an anti-triangular matrix's anti-diagonal product
    WITHOUT the permutation sign (matt.h det's n >= 4 branch; its n == 3 branch applies it), so -det for n = 2, 3 mod 4."""
    M, scale = int_rows(m)
    d = Fraction(bareiss(M)[1], scale)
    n = m.shape[0]
    quirk = n >= 4 and is_anti_triangular(m) and (n * (n - 1) // 2) % 2 == 1 and not (
        all(m[i, j, 0] == 0 for i in range(n) for j in range(i + 1, n)) or all(m[i, j, 0] == 0 for j in range(n) for i in range(j + 1, n)))
    return d, (-d if quirk else d), quirk


def cols_to_int(x):
    """[r, c, 2] -> (object ints with every COLUMN scaled to integers, the column scales)."""
    f = frac(x)
    scales = []
    for j in range(x.shape[1]):
        s = 1
        for i in range(x.shape[0]):
            s = s * f[i][j].denominator // math.gcd(s, f[i][j].denominator)
        scales.append(s)
    return np.array([[int(f[i][j] * scales[j]) for j in range(x.shape[1])] for i in range(x.shape[0])], dtype=object), scales


def box_points(rng, nv, n=160):
    pts = rng.integers(-2, 3, size=(n, nv))
    pts[0] = 0
    return pts


def satisfies(m, pts):
    """[k] bool: point k satisfies every row a.x <= c of m (rationals, constant in the last column)."""
    A, _ = int_rows(m)
    if A.shape[0] == 0:
        return np.ones(len(pts), dtype=bool)
    lhs = A[:, :-1].dot(np.array(pts, dtype=object).T)
    return np.all(lhs <= A[:, -1:], axis=0)


# ---- one case, three comparisons ----------------------------------------------------------------------------------------
def rows_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return (a.shape[0] == 0 and b.shape[0] == 0) or (a.shape == b.shape and np.array_equal(a, b))


class Tally:
    def __init__(self, ref):
        self.ref, self.n = ref, {"port": 0, "ref": 0, "exact": 0, "appro": 0, "rescued": None}


def _exact_budget(cs):
    return 1 if cs.rows * cs.cols > 4000 else (2 if cs.rows * cs.cols > 600 else 4)


def check_gauss(cs, lq, port, t, mats, rng):
    e, nb = cs.entry, cs.nb
    n_ref = min(nb, 8 if cs.rows * cs.cols > 4000 else 24)
    n_exact = _exact_budget(cs)
    if e == "rank":
        got = lq.rank(mats)
        for b in range(nb):
            assert got[b] == port.rat_rank(mats[b]), (cs, b)
        t.n["port"] += nb
        for b in range(n_ref if t.ref else 0):
            assert got[b] == t.ref.rat_rank(mats[b]), (cs, b); t.n["ref"] += 1
        for b in range(n_exact):
            a0 = port.appro_count(); port.rat_rank(mats[b])
            if port.appro_count() != a0:
                t.n["appro"] += 1; continue
            assert got[b] == exact_rank(mats[b]), (cs, b); t.n["exact"] += 1
    elif e == "det":
        got = lq.det(mats)
        for b in range(nb):
            assert tuple(got[b]) == port.rat_det(mats[b]), (cs, b)
        t.n["port"] += nb
        for b in range(n_ref if t.ref else 0):
            assert tuple(got[b]) == t.ref.rat_det(mats[b]), (cs, b); t.n["ref"] += 1
        quirks = 0
        for b in range(nb if cs.kind in ("anti", "anti2") else n_exact):
            a0 = port.appro_count(); port.rat_det(mats[b])
            if port.appro_count() != a0:
                t.n["appro"] += 1; continue
            d, want, quirk = exact_det(mats[b])
            assert Fraction(int(got[b][0]), int(got[b][1])) == want, (cs, b, tuple(got[b]), d)
            quirks += quirk; t.n["exact"] += 1
        if cs.kind in ("anti", "anti2"):            # the pinned quirk: device == reference == -exact, and exact != 0
            assert quirks == nb, cs
    elif e == "inv":
        ok, inv = lq.inv(mats)
        for b in range(nb):
            wok, winv = port.rat_inv(mats[b])
            assert ok[b] == wok and (not wok or np.array_equal(inv[b], winv)), (cs, b)
        t.n["port"] += nb
        for b in range(n_ref if t.ref else 0):
            wok, winv = t.ref.rat_inv(mats[b])
            assert ok[b] == wok and (not wok or np.array_equal(inv[b], winv)), (cs, b); t.n["ref"] += 1
        for b in range(n_exact):
            a0 = port.appro_count(); port.rat_inv(mats[b])
            if port.appro_count() != a0:
                t.n["appro"] += 1; continue
            if ok[b]:
                A, rs = int_rows(mats[b])
                X, cs_ = cols_to_int(inv[b])
                P = A.dot(X)                        # = diag(row scale i * column scale j) exactly when A . inv = I
                n = cs.rows
                assert all(P[i, j] == (rs_i * cs_[j] if i == j else 0) for i, rs_i in
                           enumerate([int(np.lcm.reduce([int(x[1]) for x in mats[b][i]])) for i in range(n)]) for j in range(n)), (cs, b)
            else:
                assert exact_rank(mats[b]) < cs.rows, (cs, b)
            t.n["exact"] += 1
    elif e == "basis":
        for unit in (True, False):
            rk, basis = lq.rankBasis(mats, unit)
            for b in range(nb):
                wrk, wb = port.rat_rank_basis(mats[b], unit)
                assert rk[b] == wrk and rows_equal(basis[b], wb), (cs, unit, b)
            t.n["port"] += nb
            for b in range(n_ref if t.ref else 0):
                wrk, wb = t.ref.rat_rank_basis(mats[b], unit)
                assert rk[b] == wrk and rows_equal(basis[b], wb), (cs, unit, b); t.n["ref"] += 1
            for b in range(n_exact):
                a0 = port.appro_count(); port.rat_rank_basis(mats[b], unit)
                if port.appro_count() != a0:
                    t.n["appro"] += 1; continue
                r = exact_rank(mats[b])
                nz = np.array([row for row in basis[b] if np.any(row[:, 0] != 0)], dtype=np.int32).reshape(-1, cs.cols, 2)
                assert rk[b] == r and nz.shape[0] == r, (cs, unit, b, rk[b], r, nz.shape)
                if r:                                   # the rows span A's row space
                    assert exact_rank(nz) == r and exact_rank(np.concatenate([mats[b], nz])) == r, (cs, unit, b)
                t.n["exact"] += 1
    elif e == "null":
        ns = lq.null(mats)
        for b in range(nb):
            assert np.array_equal(ns[b], port.rat_null(mats[b])), (cs, b)
        t.n["port"] += nb
        for b in range(n_ref if t.ref else 0):
            assert np.array_equal(ns[b], t.ref.rat_null(mats[b])), (cs, b); t.n["ref"] += 1
        for b in range(n_exact):
            a0 = port.appro_count(); port.rat_null(mats[b])
            if port.appro_count() != a0:
                t.n["appro"] += 1; continue
            A, _ = int_rows(mats[b])
            X, _ = cols_to_int(ns[b])
            live = [j for j in range(cs.cols) if any(X[i, j] != 0 for i in range(cs.cols))]
            assert len(live) == cs.cols - exact_rank(mats[b]), (cs, b)
            assert all(v == 0 for v in A.dot(X[:, live]).flat), (cs, b)
            t.n["exact"] += 1


def check_int(cs, lq, port, t, a, rng):
    nb = cs.nb
    if cs.entry == "gcd":
        g = lq.gcd(a)
        for b in range(nb):
            assert np.array_equal(g[b], port.int_gcd(a[b])), (cs, b)
            if t.ref and b < 32:
                assert np.array_equal(g[b], t.ref.int_gcd(a[b])), (cs, b); t.n["ref"] += 1
            for i in range(cs.rows):                       # every row divided by the gcd of its entries
                row = [int(x) for x in a[b, i]]
                d = math.gcd(*row)
                assert [int(x) for x in g[b, i]] == ([x // d for x in row] if d > 1 else row), (cs, b, i)
            t.n["exact"] += 1
        t.n["port"] += nb
        return
    st, h, u = lq.hnf(a)
    defined = 0
    for b in range(nb):
        wst, wh, wu = port.int_hnf(a[b])
        assert st[b] == wst, (cs, b)
        t.n["port"] += 1
        if wst:
            assert wst == XPG_ERR_REF_UNDEFINED
            continue                                       # (the reference itself is undefined there: not run)
        defined += 1
        assert np.array_equal(h[b], wh) and np.array_equal(u[b], wu), (cs, b)
        if t.ref and b < 8:
            rst, rh, ru = t.ref.int_hnf(a[b])
            assert rst == 0 and np.array_equal(h[b], rh) and np.array_equal(u[b], ru), (cs, b); t.n["ref"] += 1
        A, U, H = a[b].astype(object), u[b].astype(object), h[b].astype(object)
        AU = A.dot(U)
        wrap = np.vectorize(lambda v: ((int(v) + 2 ** 31) % 2 ** 32) - 2 ** 31, otypes=[object])
        assert np.array_equal(wrap(AU), H), (cs, b)        # H = A.U in Z/2^32, always
        assert not np.any(np.triu(h[b], 1)), (cs, b)       # and lower triangular (a cleared cell stays 0 mod 2^32)
        if b < _exact_budget(cs) * 2 and np.array_equal(AU, H):      # nothing wrapped: the HNF properties
            lim = min(cs.rows, cs.cols)
            assert not np.any(np.triu(h[b], 1)), (cs, b)
            for i in range(lim):
                assert h[b, i, i] > 0 and all(0 <= h[b, i, j] < h[b, i, i] for j in range(i)), (cs, b, i)
            assert abs(bareiss(U)[1]) == 1, (cs, b)
            t.n["exact"] += 1
        h0 = hermite_of_permuted(a[b])
        if h0 is not None:                                 # A = H0 P with H0 in Hermite form: the unique HNF is H0
            assert np.array_equal(h[b], h0), (cs, b)
            t.n["exact"] += 1
    if cs.kind == "negdiag":
        assert (st == XPG_ERR_REF_UNDEFINED).all(), st
    else:
        assert defined > 0


def check_rows(cs, lq, port, t, mats, rng):
    e, nb, nv = cs.entry, cs.nb, cs.cols - 1
    n_exact = _exact_budget(cs)
    n_ref = min(nb, 12) if t.ref else 0
    pts = box_points(rng, nv)
    if e == "iden":
        res = lq.removeIdenRow(mats)
        for b in range(nb):
            assert rows_equal(res[b], port.remove_iden_row(mats[b])), (cs, b)
            if b < n_ref:
                assert rows_equal(res[b], t.ref.remove_iden_row(mats[b])), (cs, b); t.n["ref"] += 1
            seen, keep = set(), []
            for row in mats[b]:                           # a row goes iff an earlier row is identical field by field
                k = row.tobytes()
                if k not in seen:
                    seen.add(k); keep.append(row)
            assert rows_equal(res[b], np.array(keep).reshape(-1, cs.cols, 2)), (cs, b)
            t.n["exact"] += 1
        t.n["port"] += nb
        return
    if e == "reduce":
        for inter in (True, False):
            ok, res = lq.reduce(mats, nv, inter)
            for b in range(nb):
                wok, wres = port.reduce(mats[b], nv, inter)
                assert ok[b] == wok and (not wok or rows_equal(res[b], wres)), (cs, inter, b)
                if b < n_ref:
                    rok, rres = t.ref.reduce(mats[b], nv, inter)
                    assert ok[b] == rok and (not rok or rows_equal(res[b], rres)), (cs, inter, b); t.n["ref"] += 1
            t.n["port"] += nb
            for b in range(n_exact):
                a0 = port.appro_count(); port.reduce(mats[b], nv, inter)
                if port.appro_count() != a0:
                    t.n["appro"] += 1; continue
                feas = satisfies(mats[b], pts)
                if not ok[b]:
                    assert not feas.any(), (cs, inter, b)
                else:
                    assert satisfies(res[b], pts[feas]).all(), (cs, inter, b)
                t.n["exact"] += 1
        return
    if e == "fme":
        u = int(rng.integers(0, nv))
        for dark in (False, True):
            ok, res = lq.fme(mats, nv, u, dark)
            for b in range(nb):
                a0 = port.appro_count()
                wok, wres = port.fme(mats[b], nv, u, dark)
                t.n["rescued"] = (t.n["rescued"] or 0) + (port.appro_count() != a0)
                assert ok[b] == wok and rows_equal(res[b], wres), (cs, dark, b)
                if b < n_ref:
                    rok, rres = t.ref.fme(mats[b], nv, u, dark)
                    assert ok[b] == rok and rows_equal(res[b], rres), (cs, dark, b); t.n["ref"] += 1
            t.n["port"] += nb
            for b in range(n_exact if not dark else 0):
                a0 = port.appro_count(); port.fme(mats[b], nv, u, dark)
                if port.appro_count() != a0:
                    t.n["appro"] += 1; continue
                feas = satisfies(mats[b], pts)
                if not ok[b]:
                    assert not feas.any(), (cs, b)
                else:                                    # every point of the input satisfies the output, and u is gone --
                    # except for the pinned quirk: where u appears in ONE input row the reference keeps that row (linsys.cpp
                    # fme: a lone row is copied, not dropped), so the output still names u there, in exactly that row
                    lone = int(np.count_nonzero(mats[b][:, u, 0])) == 1
                    assert int(np.count_nonzero(res[b][:, u, 0])) == (1 if lone else 0), (cs, b, lone)
                    assert satisfies(res[b], pts[feas]).all(), (cs, b)
                t.n["exact"] += 1
        return
    cap = cs.extra
    ok, bounds = lq.calcBound(mats, nv, cap_rows=cap)
    for b in range(nb):
        a0 = port.appro_count()
        wok, wb = port.calc_bound(mats[b], nv, cap_rows=cap)
        t.n["rescued"] = (t.n["rescued"] or 0) + (port.appro_count() != a0)
        assert ok[b] == wok, (cs, b)
        if wok:
            assert all(rows_equal(bounds[b][j], wb[j]) for j in range(nv)), (cs, b)
        if b < n_ref:
            rok, rb = t.ref.calc_bound(mats[b], nv, cap_rows=cap)
            assert ok[b] == rok and (not rok or all(rows_equal(bounds[b][j], rb[j]) for j in range(nv))), (cs, b)
            t.n["ref"] += 1
    t.n["port"] += nb
    for b in range(min(nb, n_exact)):
        a0 = port.appro_count(); port.calc_bound(mats[b], nv, cap_rows=cap)
        if port.appro_count() != a0:
            t.n["appro"] += 1; continue
        feas = satisfies(mats[b], pts)
        if not ok[b]:
            assert not feas.any(), (cs, b)
        else:                                            # variable j's bounds hold on every point of the input (they may still
            for j in range(nv):                          # name a variable of a lone row: the fme quirk above, chained)
                assert satisfies(bounds[b][j], pts[feas]).all(), (cs, b, j)
        t.n["exact"] += 1


def _call_refused(cs, lq, mats):
    e, nv = cs.entry, cs.cols - 1
    return {"rank": lambda: lq.rank(mats), "det": lambda: lq.det(mats), "inv": lambda: lq.inv(mats),
            "basis": lambda: lq.rankBasis(mats, True), "null": lambda: lq.null(mats), "hnf": lambda: lq.hnf(mats),
            "reduce": lambda: lq.reduce(mats, nv, True), "iden": lambda: lq.removeIdenRow(mats),
            "fme": lambda: lq.fme(mats, nv, 0), "calc": lambda: lq.calcBound(mats, nv, cap_rows=cs.extra)}[e]()


@pytest.fixture(scope="module")
def lq(ctx):
    from xpoly_amd.lineq import Lineq
    return Lineq(ctx)


@pytest.fixture(scope="module")
def ref_or_none():
    from oracle.checker import Ref
    return Ref() if Ref.available() else None


def _case_id(cs):
    return "%s-%s-%dx%d-nb%d" % (cs.entry, cs.label.replace(" ", "_"), cs.rows, cs.cols, cs.nb)


@pytest.mark.gpu
@pytest.mark.parametrize("cs", CASES, ids=[_case_id(cs) for cs in CASES])
def test_kernel_at_launch_geometry(cs, lq, port, ref_or_none, ctx):
    from xpoly_amd._capi import XpgError
    rng = np.random.default_rng(zlib.crc32(_case_id(cs).encode()))
    facts, geo = case_facts(cs)
    a = make_input(cs, rng)
    mats = a.astype(np.int32) if cs.entry in ("hnf", "gcd") else rat(a)
    if cs.kind == "packing":
        mats = nonpositive_denominators(mats, rng)
    t = Tally(ref_or_none)
    if geo is None:                                      # refused before any launch, and the handle works on
        with pytest.raises(XpgError, match="XPG_ERR_UNSUPPORTED"):
            _call_refused(cs, lq, mats)
        small = gen.random_square(rng, 5)[None]
        assert lq.rank(small)[0] == port.rat_rank(small[0]) and tuple(lq.det(small)[0]) == port.rat_det(small[0])
        print("%s: refused as XPG_ERR_UNSUPPORTED, next call matches" % _case_id(cs))
        return
    if cs.entry in GAUSS_OP:
        check_gauss(cs, lq, port, t, mats, rng)
    elif cs.entry in ("hnf", "gcd"):
        check_int(cs, lq, port, t, mats, rng)
    else:
        check_rows(cs, lq, port, t, mats, rng)
    # fme and calcBound: the systems of the port count on which the checker approximated at all (nothing is asserted about it:
    # the inputs that are MEANT to approximate are tests/lineq_rescue_cases.py's)
    rescued = "" if t.n["rescued"] is None else ", checker approximated on %d" % t.n["rescued"]
    print("%s L=%d G=%d: port %d, ref %s, exact %d (appro skipped %d)%s" % (
        _case_id(cs), geo[0], geo[1], t.n["port"], t.n["ref"] if ref_or_none else "not built", t.n["exact"], t.n["appro"], rescued))
    assert t.n["port"] > 0
    if cs.kind not in ("rand4", "negdiag"):
        assert t.n["exact"] > 0, "the exact check never ran: %s" % (cs,)


@pytest.mark.gpu
def test_packed_view_survives_in_place_reduce(lq):
    """include/xpoly_amd.h: the out_view of a packed fme stays valid until the next PACKED call. The in-place reduce and
    removeIdenRow forms and the ragged fme are not packed calls: they must leave the view's bytes alone."""
    rng = np.random.default_rng(11)
    one = np.stack([gen.random_system(rng, 10, 4)])
    ok, off, view = lq.fme_packed(one, 4, 1, copy=False)
    assert view.shape[0] > 0
    keep = view.copy()
    # the pinned buffer now holds [offsets, flags | the input (400 B) | the slots (36 rows x 5 x 8 B)] and has room for
    # 1.25x that + 4 KB: four systems of the same shape staged in place (offsets, 1.6 KB in, 1.6 KB out) fit without a
    # reallocation and, staged through that buffer, would land on the view
    four = np.stack([gen.random_system(rng, 10, 4) for _ in range(4)])
    lq.reduce_inplace(four, 4, True)
    assert np.array_equal(view, keep)
    lq.removeIdenRow(four)
    assert np.array_equal(view, keep)
    ok_r, res_r = lq.fme_ragged([four[0]], [1])          # one class of the same shape: staged where the view lies
    assert np.array_equal(view, keep)
    assert ok_r[0] == lq.fme(four[:1], 4, 1)[0][0]
