"""Shared by tests/test_gpu_batch_geometry.py and its child process tests/batch_geometry_worker.py: a Python mirror of the
launch rules of the batched LP kernel (csrc/batch_kernels.hip.h: batch_geometry, batch_host, batch_dev_ragged, sm_solve,
sm_solve_lp), the LP families the cases are made of, the case table derived from the mirror, and a small exact simplex on
fractions.Fraction. No GPU and no library is needed to import it."""
import zlib
from collections import namedtuple
from fractions import Fraction

import numpy as np

F64, RAT = 0, 1
LDS_MAX = 160 * 1024
SMALL_LDS_STATIC = 272                  # batch_kernels.hip.h: what the kernels hold in LDS besides the LP's arrays
SIZEOF_CAND = {F64: 16, RAT: 12}        # lp_kernels.hip.h: struct Cand { S q; int idx; } -- double (8-aligned) / two int32
NO_LIMIT = 0xFFFFFFFF
GENERIC, WAVE0, OVERLAPPED, SPECIALISED = "generic", "wave0-fast", "overlapped", "specialised"
FORMS = (GENERIC, WAVE0, OVERLAPPED, SPECIALISED)


# ---- mirror of the host rules ---------------------------------------------------------------------------------------------
def solved_as(is_max, m, cols):
    """(R rows, V variables) of the slack form the kernel builds: the primal under maxm, the dual under minm."""
    return (m, cols - 1) if is_max else (cols - 1, m)


def caller_shape(is_max, R, V):
    """(m, cols) of the caller's arrays for an LP solved as R x V."""
    return (R, V + 1) if is_max else (V, R + 1)


def small_lds_bytes(kind, R, V):
    wmax = V + 1 + R + 1
    nmax = wmax - 1
    pw = (nmax + 31) // 32
    b = R * wmax * 8                      # tab
    b += wmax * 8 * 3                     # obj, e, x
    b += ((R + 1) & ~1) * 8               # k
    b += 16 * SIZEOF_CAND[kind]           # sh_c
    b += nmax * 4 * 3                     # bv2eq, rowcnt, colcnt
    b += R * 4                            # eq2bv
    b += nmax * pw * 4                    # ppt
    b += 16 * 4 + 8 * 4                   # sh_i, sh_w
    b += ((nmax + 3) & ~3) * 2            # nv, bv
    return (b + 15) & ~15


def lds_fits(kind, R, V):
    """small_lds_fits: the LP's arrays and the kernel's own LDS fit one CU's 160 KB together."""
    return small_lds_bytes(kind, R, V) + SMALL_LDS_STATIC <= LDS_MAX


def thread_rule(R, V):
    cells = R * (V + R + 2)
    return 256 if cells >= 2048 else (128 if cells >= 1024 else 64)


Geom = namedtuple("Geom", "lds refused cells threads per_cu five grid seats slice_shape slice_crowded")


def geometry(kind, R, V, nb, cus=256):
    """batch_geometry<S>(R, V, nb, num_cus), field by field."""
    lds = small_lds_bytes(kind, R, V)
    per_cu = max(LDS_MAX // lds, 1)
    grid = min(256 * min(per_cu, 16) * 64, nb)
    five = per_cu >= 5
    seats = cus * (min(per_cu, 5) if five else min(per_cu, 4))
    threads = thread_rule(R, V)
    return Geom(lds, int(not lds_fits(kind, R, V)), R * (V + R + 2), threads, per_cu, int(five), grid, seats,
                int(threads >= 128 and R <= 64 and R + V <= 127), int(nb > seats + seats // 4))


def sliced(kind, R, V, nb, cus=256, force=False, slice_env=512):
    """batch_dev: whether the launch runs in time slices (they apply to `overlapped` solves only)."""
    g = geometry(kind, R, V, nb, cus)
    return bool(slice_env != 0 and g.slice_shape and (g.slice_crowded or force) and g.grid == nb and not g.refused)


def pinned_route(m, cols, nb):
    """batch_host: pinned staging (out_sol copied for status 0 only) up to 1 MiB of input, pageable copies above."""
    return nb * m * cols * 8 + nb * cols * 8 <= (1 << 20)


def loop_form(kind, R, V, threads, aux):
    """sm_solve: the loop one solve runs in. aux: stage 1's auxiliary LP (one more column: rhs = V + R + 1)."""
    rhs = V + R + (1 if aux else 0)
    if R > 64 or rhs > 128:
        return GENERIC
    if not (rhs <= 127 and threads >= 128):
        return WAVE0
    ld, W = V + R + 2, rhs + 1            # (every launch carves the LDS for the LP's own shape: ld = V + 1 + R + 1)
    if kind == F64 and R == 32 and ld == 97 and threads == 256 and W in (96, 97):
        return SPECIALISED
    return OVERLAPPED


def loop_forms(kind, R, V, threads, stage1):
    """(form of stage 1's solve or None, form of the LP's own solve)."""
    return (loop_form(kind, R, V, threads, True) if stage1 else None, loop_form(kind, R, V, threads, False))


def stage1_runs(b, c):
    """sm_solve_lp (lpsol.h:1794-1803): no positive objective coefficient, or a negative right-hand side."""
    return bool(not (np.asarray(c) > 0).any() or (np.asarray(b) < 0).any())


def ragged_threads(kind, shapes):
    """batch_dev_ragged: threads (and LDS) come from the largest R and the largest V of the call."""
    return thread_rule(max(s[0] for s in shapes), max(s[1] for s in shapes))


def first_shape(pred, shapes):
    for s in shapes:
        if pred(*s):
            return s
    raise LookupError("no shape satisfies the predicate")


def largest_accepted(kind, family):
    """The largest k with family(k) = (R, V) accepted; family(k + 1) is the first refused shape."""
    ok = lambda k: lds_fits(kind, *family(k))
    k = 4
    while ok(2 * k):
        k *= 2
    hi = 2 * k
    while hi - k > 1:
        mid = (k + hi) // 2
        k, hi = (mid, hi) if ok(mid) else (k, mid)
    return k


LIMIT_FAMILIES = {"square": lambda k: (k, k), "tall": lambda k: (k, 24), "wide": lambda k: (24, k)}


# ---- LP families, all in the form that is SOLVED: maximise c.x, A x <= b, x >= 0 with A [R, V] ----------------------------------
# Under maxm the caller hands over exactly that; under minm the caller hands over its dual written as a covering problem
# (minimise b.y, -A^T y <= -c, y >= 0), of which SIX::minm builds the dual again: the kernel solves the same slack form, so
# the shape (R, V), the stage-1 trigger and the loop forms of a case do not depend on the mode.
def _ones_rows(rng, R, V, maxlen):
    A = np.zeros((R, V))
    tiles = max(1, min(R // 2, V // 8))
    starts = np.linspace(0, V, tiles + 1).astype(int)
    for k in range(tiles):
        A[k, starts[k]:starts[k + 1]] = 1                  # the first rows tile the columns: every variable is bounded
    for r in range(tiles, R):
        a = int(rng.integers(0, max(V - 1, 1)))
        A[r, a:min(V, a + int(rng.integers(1 if V < 3 else 2, maxlen + 1)))] = 1
    return A


def fam_ones(rng, kind, R, V, stage1):
    """Consecutive-ones rows (totally unimodular: every basis inverse is integral), integer b and c: exact in both scalar
    types; fp64 rows and columns are rescaled by powers of two as gen.interval_lp_f64 does. stage1: a third of the rows become
    lower bounds -x_j <= -1 (a negated unit row keeps the matrix totally unimodular)."""
    A = _ones_rows(rng, R, V, max(2, min(24, V // 2)))
    b = rng.integers(1, 40, size=R).astype(np.float64)
    c = rng.integers(1, 9, size=V).astype(np.float64)
    if stage1:
        tiles = max(1, min(R // 2, V // 8))
        rows = [r for r in range(tiles, R)][: max(3, R // 3 + 2)] or [R - 1]      # (one pivot of stage 1's solve each, or so)
        for t, r in enumerate(rows):
            A[r] = 0
            A[r, (7 * t + 1) % V] = -1
            b[r] = -1
    if kind == F64:
        rs = 2.0 ** rng.integers(-2, 3, size=R)
        cs = 2.0 ** rng.integers(-2, 3, size=V)
        A, b, c = A * rs[:, None] * cs[None, :], b * rs, c * cs
    return A, b, c


def fam_dense(rng, kind, R, V, stage1):
    """Dense positive data (origin feasible): U(0.1, 1) in fp64 (rounded arithmetic: the reference's 1e-17 final check may
    end it OPTIMAL_IS_INFEASIBLE), integers 1..9 as Rational. stage1: a third of the rows are negated into covering rows."""
    if kind == F64:
        A = 0.1 + 0.9 * rng.random((R, V)); b = V * (0.5 + 0.5 * rng.random(R)); c = 0.1 + 0.9 * rng.random(V)
    else:
        A = rng.integers(1, 10, size=(R, V)).astype(np.float64)
        b = rng.integers(3 * V, 5 * V + 1, size=R).astype(np.float64)
        c = rng.integers(1, 10, size=V).astype(np.float64)
    if stage1:                                             # a third of the rows become covering rows a.x >= b' that x = 1 satisfies
        for r in range(R - max(1, R // 3), R):
            A[r] = -A[r]
            b[r] = -0.2 * V if kind == F64 else -float(V)
    return A, b, c


def fam_dep(rng, kind, R, V, stage1):
    """Dependence-test-like (gen.small_lp_batch_f64 family 1): entries in -3..3 at density 1/4, objective all ones; the
    right-hand sides in -2..17 with stage 1 and a third of them in -3..-1, in 0..17 without."""
    A = np.where(rng.random((R, V)) < 0.25, rng.integers(-3, 4, size=(R, V)), 0).astype(np.float64)
    b = rng.integers(-2 if stage1 else 0, 18, size=R).astype(np.float64)
    if stage1:
        b[rng.permutation(R)[: max(1, R // 3)]] = -rng.integers(1, 4, size=max(1, R // 3))
    return A, b, np.ones(V)


def fam_unbounded(rng, kind, R, V, stage1):
    """fam_dep with a first column that no row limits from above and a positive cost on it."""
    A, b, c = fam_dep(rng, kind, R, V, stage1)
    A[:, 0] = -np.abs(A[:, 0])
    b = np.abs(b) if not stage1 else b
    return A, b, c


def fam_chain(rng, kind, R, V, stage1, feasible=True):
    """Difference constraints x_0 >= 1, x_k >= x_{k-1} + 1 under loose upper bounds (integer data: exact as Rational; in
    fp64 the auxiliary column and the all-ones row bring divisors that are not powers of two, and results carry rounding). stage 1's solve raises the variables one pivot at a time, min(R - 1, V) pivots -- the family that gives stage 1's
    solve a length. feasible=False: the last row caps the last variable of the chain below what the chain demands. Without
    stage 1 there is no such LP: fam_ones stands in."""
    if not stage1:
        return fam_ones(rng, RAT, R, V, False)
    A = np.zeros((R, V)); b = np.zeros(R); c = np.ones(V)
    K = min(R - 1, V)
    for k in range(K):
        A[k, k] = -1
        if k:
            A[k, k - 1] = 1
        b[k] = -1
    for r in range(K, R):
        A[r, int(rng.integers(0, V))] = 1
        b[r] = int(rng.integers(K + 1, 3 * K + 2))
    A[R - 1] = 0
    if feasible:
        A[R - 1, :] = 1; b[R - 1] = K * K + int(rng.integers(0, 5))
    else:
        A[R - 1, K - 1] = 1; b[R - 1] = K - 1
    return A, b, c


def fam_chain_infeasible(rng, kind, R, V, stage1):
    return fam_chain(rng, kind, R, V, stage1, feasible=False)


FAMILIES = {"chain": fam_chain, "chainx": fam_chain_infeasible, "ones": fam_ones, "dense": fam_dense, "dep": fam_dep, "unbounded": fam_unbounded}
# fp64 arithmetic is exact on these WITHOUT stage 1 (each is then fam_ones: A is totally unimodular, so every tableau entry is
# 0 or +-1 times powers of two and every operation is exact). With stage 1 the auxiliary column of -1 breaks total
# unimodularity: solutions with full mantissas were seen at 32 x 63, so fp64 LPs with stage 1 never take the exact check.
EXACT_FAMILIES = ("ones", "chain", "chainx")
MIX = ("ones", "dense", "dep", "unbounded", "chain", "dep", "chainx", "dense")      # one LP of each in turn
CHEAP = ("ones", "chainx", "chain")         # few pivots: Rational at large shapes (dense or dependence-like data costs the
                                            # CPU oracle ~10 s per LP there: ~8 000 pivots, most through the float rescue)


# ---- the case table -------------------------------------------------------------------------------------------------------
# kind, is_max, R, V (as solved), nb, stage1 (whether every LP of the case runs stage 1), recipe (families in turn), limit
# (max_iter), label (the branch the case is in the table for), entry ("host", "dev": the _dev form with out_pivots)
Case = namedtuple("Case", "kind is_max R V nb stage1 recipe limit label entry")


def case_id(cs):
    return "%s-%s-%s-%dx%d-nb%d%s" % ("f64" if cs.kind == F64 else "rat", "maxm" if cs.is_max else "minm", cs.label.replace(" ", "_"),
                                      cs.R, cs.V, cs.nb, "-s1" if cs.stage1 else "")


def case_seed(cs):
    # (neither the mode nor the limit is part of the seed: the maxm and the minm case of a shape solve the same slack forms)
    return zlib.crc32(("%d %s %d %d %d" % (cs.kind, cs.label, cs.R, cs.V, cs.stage1)).encode())


# Seeds found by a search with the CPU oracle (Port): the cases made of the exact families alone must END with status 0
# in at least half of their LPs (tests/test_gpu_batch_geometry.py test_cases_are_not_vacuous); at these shapes the reference's
# pair table ends many a bounded LP as UNBOUND or OPTIMAL_IS_INFEASIBLE. The seeds are part of the fixture.
SALTS = {(0, 'largest square', 96, 96, 0): 1, (1, 'largest square', 96, 96, 0): 1, (0, 'exact', 20, 40, 0): 2, (0, 'exact', 40, 87, 0): 1, (0, 'exact', 70, 40, 0): 1, (1, 'exact', 20, 40, 0): 4, (1, 'exact', 40, 87, 0): 5, (1, 'exact', 40, 100, 0): 5, (1, 'exact', 32, 63, 1): 1,
         (0, 'exact', 14, 12, 0): 1, (1, 'exact', 14, 12, 0): 6}


def make_lps(cs):
    """The LPs of a case as solved: a list of (family, A, b, c). Deterministic: the generator calls, seeds included, are the
    fixture. Batches above 64 LPs repeat their first 64 (the oracles solve each distinct LP once)."""
    rng = np.random.default_rng([case_seed(cs), SALTS.get((cs.kind, cs.label, cs.R, cs.V, cs.stage1), 0)])
    out = []
    for i in range(min(cs.nb, 64)):
        fam = cs.recipe[i % len(cs.recipe)]
        A, b, c = FAMILIES[fam](rng, cs.kind, cs.R, cs.V, cs.stage1)
        if not cs.stage1 and not (c > 0).any():
            c[0] = 1
        assert stage1_runs(b, c) == bool(cs.stage1), (cs, fam)
        out.append((fam, A, b, c))
    return [out[i % 64] for i in range(cs.nb)]


def c0_of(i):
    """The constant term of the objective of LP i of a batch: 0, 1, 2, 3 in turn (it does not change a pivot)."""
    return float(i % 4)


def caller_arrays(kind, is_max, lps):
    """(tgtf [nb, cols], leq [nb, m, cols]) as the caller hands them over; Rational: int32 (num, den) pairs."""
    tg, lq = [], []
    for i, (_, A, b, c) in enumerate(lps):
        if is_max:
            lq.append(np.concatenate([A, b[:, None]], axis=1)); tg.append(np.concatenate([c, [c0_of(i)]]))
        else:
            lq.append(np.concatenate([-A.T, -c[:, None]], axis=1)); tg.append(np.concatenate([b, [c0_of(i)]]))
    tg, lq = np.ascontiguousarray(np.stack(tg)) + 0.0, np.ascontiguousarray(np.stack(lq)) + 0.0     # (+ 0.0: no -0.0 cells)
    if kind == RAT:
        assert (tg == np.floor(tg)).all() and (lq == np.floor(lq)).all()
        return _to_rat(tg), _to_rat(lq)
    return tg, lq


def _to_rat(a):
    out = np.empty(a.shape + (2,), dtype=np.int32)
    out[..., 0] = a
    out[..., 1] = 1
    return out


def _shape_scan():
    for R in list(range(1, 70)) + [96, 100]:
        for V in list(range(1, 131)):
            yield R, V


def reachable_form_pairs():
    """Every (stage-1 form or None, own form) some accepted shape of some kind has."""
    seen = set()
    for kind in (F64, RAT):
        for R, V in _shape_scan():
            if lds_fits(kind, R, V):
                for s1 in (False, True):
                    seen.add(loop_forms(kind, R, V, thread_rule(R, V), s1))
    return seen


def _cases():
    c = []

    def add(kind, R, V, label, stage1=False, nb=8, recipe=None, limit=NO_LIMIT, modes=(1, 0), entry="host"):
        big = R * (R + V + 2) >= 2048
        recipe = recipe or (MIX if kind == F64 or not big else CHEAP)
        for is_max in modes:
            c.append(Case(kind, is_max, R, V, nb, int(stage1), tuple(recipe), limit, label, entry))

    both = (F64, RAT)
    # thread count: cells = R (V + R + 2) at 1023 / 1024 and 2047 / 2048 -- the shapes come from the rule itself
    for R, lo in ((16, 1024), (32, 2048)):
        V_hi = first_shape(lambda r, v: r * (v + r + 2) >= lo, ((R, v) for v in range(1, 200)))[1]
        for kind in both:
            add(kind, R, V_hi - 1, "cells below %d" % lo)
            add(kind, R, V_hi, "cells at %d" % lo)
            add(kind, R, V_hi, "cells at %d" % lo, stage1=True)
    # row count: the fast loops take at most 64 rows
    for kind in both:
        for s1 in (False, True):
            add(kind, 64, 40, "rows 64", stage1=s1, nb=6)
            add(kind, 65, 40, "rows 65", stage1=s1, nb=6)
    # R + V = 126 .. 129: rhs 127 / 128 / 129 in the auxiliary solve (stage 1) and in the own solve (without), separately
    for kind in both:
        for tot in (126, 127, 128, 129):
            for s1 in (False, True):
                add(kind, 40, tot - 40, "R+V %d" % tot, stage1=s1, nb=6)
    for tot in (127, 128):                       # the same edge on one wavefront (64 threads: 8 rows)
        for s1 in (False, True):
            add(F64, 7, tot - 7, "R+V %d on 64 threads" % tot, stage1=s1, nb=6)
    # the specialised loop (fp64, 32 rows, 63 variables, 256 threads) and its near misses
    for s1 in (False, True):
        add(F64, 32, 63, "specialised", stage1=s1, nb=16, modes=(1,))
        add(F64, 32, 63, "specialised dual", stage1=s1, nb=8, modes=(0,))           # 63 rows x 33 columns under minm
        for R, V, lab in ((32, 62, "one variable less"), (32, 64, "one variable more"), (31, 63, "one row less"),
                          (33, 63, "one row more")):
            add(F64, R, V, "specialised near miss " + lab, stage1=s1, nb=8)
        add(RAT, 32, 63, "specialised near miss rational", stage1=s1, nb=6)
    add(F64, 63, 32, "specialised near miss transposed", nb=8, modes=(1, 0))    # minm: 32 rows x 64 columns handed over, solved 63 x 32
    # the kernel instance: five LPs per CU by LDS, or four
    for kind in both:
        V5 = max(v for v in range(1, 400) if LDS_MAX // small_lds_bytes(kind, 32, v) >= 5)
        add(kind, 32, V5, "five per CU", nb=6)
        add(kind, 32, V5 + 1, "four per CU", nb=6)
    # fully generic shapes: tall and wide
    for kind in both:
        for R, V in ((70, 20), (96, 60), (40, 100), (30, 110)):
            for s1 in (False, True):
                add(kind, R, V, "generic %s" % ("tall" if R > V else "wide"), stage1=s1, nb=6 if kind == F64 else 4)
    # the smallest shapes
    for kind in both:
        add(kind, 1, 1, "one by one", nb=8, recipe=("ones", "dense", "dep", "unbounded"))
        add(kind, 1, 1, "one by one", stage1=True, nb=8, recipe=("ones", "dep"))
        add(kind, 1, 90, "one row", nb=6, recipe=("ones", "dense", "dep", "unbounded"))
        add(kind, 90, 1, "one variable", nb=6, recipe=("ones", "dense", "dep"))
    # the largest accepted shape of each family and the first refused one
    for kind in both:
        for fam, f in LIMIT_FAMILIES.items():
            k = largest_accepted(kind, f)
            add(kind, *f(k), "largest %s" % fam, nb=2, recipe=("ones",))
            if kind == F64:
                add(kind, *f(k), "largest %s mixed" % fam, nb=3, recipe=("dep", "dense", "unbounded"), stage1=True)
            add(kind, *f(k + 1), "refused %s" % fam, nb=1, recipe=("ones",))
            # shapes whose arrays alone fit 160 KB but not beside the kernel's own 272 bytes: the rule used to accept them and
            # the launch failed with XPG_ERR_HIP (found at Rational 126 x 24, 163 808 bytes); now refused like any other
            for k2 in range(k + 1, k + 40):
                if small_lds_bytes(kind, *f(k2)) <= LDS_MAX:
                    add(kind, *f(k2), "refused static LDS %s" % fam, nb=2, recipe=("ones",))
    # the byte edge of the refusal rule: arrays + the kernel's own LDS = 160 KB exactly (accepted), 16 bytes more (refused)
    edge = [(R, V) for R in range(20, 90) for V in range(100, 600)]
    add(F64, *first_shape(lambda r, v: small_lds_bytes(F64, r, v) + SMALL_LDS_STATIC == LDS_MAX, edge), "largest static edge", nb=2, recipe=("ones",))
    add(F64, *first_shape(lambda r, v: small_lds_bytes(F64, r, v) + SMALL_LDS_STATIC == LDS_MAX + 16, edge), "refused static edge", nb=2, recipe=("ones",))
    # more LPs than the chip seats at a slice-eligible shape: the launch runs in time slices without any hook
    add(F64, 20, 40, "crowded", stage1=True, nb=2000, modes=(1,))
    add(F64, 32, 63, "crowded", nb=2000, modes=(1,))
    # nb above the grid cap of a small shape (lp += nmain), and a single LP
    cap = geometry(F64, 12, 12, 1 << 30).grid
    add(F64, 12, 12, "grid stride", nb=cap + 37, modes=(1,))
    add(F64, 12, 12, "grid stride", nb=cap + 37, stage1=True, modes=(0,))
    for kind in both:
        add(kind, 12, 12, "single LP", nb=1, recipe=("chainx",), stage1=True)
        add(kind, 40, 100, "single LP generic", nb=1, recipe=("ones",))
    # iteration limits: SIX_TIME_OUT inside stage 1 (status 2) and in the own solve (status 4), in every loop form
    for kind, R, V, lim in ((F64, 14, 12, 10), (F64, 20, 40, 15), (F64, 32, 63, 25), (F64, 70, 20, 14), (RAT, 20, 40, 15),
                            (RAT, 14, 12, 10), (RAT, 70, 20, 14)):
        for s1 in (False, True):
            add(kind, R, V, "limit %d" % lim, stage1=s1, nb=12, limit=lim, recipe=("dense", "dep", "ones", "chain"))
    # the exact families alone, in every loop form (the cases that claim the exact check)
    for kind in both:
        for R, V in ((14, 12), (20, 40), (32, 63), (40, 87), (40, 100), (70, 40)):
            for s1 in (False, True):
                if not (s1 and R > 64):             # (a third of 70 rows as lower bounds leaves the oracle almost no LP to end with status 0)
                    add(kind, R, V, "exact", stage1=s1, nb=6, recipe=("ones", "chain") if s1 else ("ones",))
    # the _dev entry points with out_pivots
    for kind in both:
        for R, V in ((12, 12), (12, 10), (20, 40), (32, 63), (70, 20)):
            for s1 in (False, True):
                add(kind, R, V, "dev pivots", stage1=s1, nb=8 if kind == F64 else 6, entry="dev")
    return c


CASES = _cases()


def case_facts(cs, cus=256):
    g = geometry(cs.kind, cs.R, cs.V, cs.nb, cus)
    m, cols = caller_shape(cs.is_max, cs.R, cs.V)
    return dict(geom=g, forms=loop_forms(cs.kind, cs.R, cs.V, g.threads, cs.stage1), pinned=pinned_route(m, cols, cs.nb),
                stride=cs.nb > g.grid)


# the two batches of the host-route case: the same LPs, one LP more puts the call above 1 MiB
def route_cases():
    R, V = 16, 46
    m, cols = caller_shape(1, R, V)
    nb = max(n for n in range(1, 4000) if pinned_route(m, cols, n))
    mk = lambda n, lab: Case(F64, 1, R, V, n, 1, ("dep", "ones", "dense", "chainx", "chain"), NO_LIMIT, lab, "host")
    return mk(nb, "host route"), mk(nb + 1, "host route")        # (pinned, pageable: the same label, so the same LPs)


# ragged parity: LPs (kind, is_max, R, V, stage1) and the companion shapes that set the call's threads and LDS
RAGGED_LPS = [(F64, 1, 8, 10, 0), (F64, 1, 8, 10, 1), (F64, 1, 16, 30, 1), (F64, 1, 32, 63, 0), (F64, 1, 32, 63, 1),
              (F64, 0, 12, 9, 1), (RAT, 1, 8, 10, 1), (RAT, 1, 16, 30, 0), (RAT, 0, 12, 9, 1)]
RAGGED_COMPANIONS = {128: (20, 40), 256: (40, 80)}        # the mirror checks the thread counts these force


# slices at the eligibility edge (child process on the hooks build, XPG_BATCH_SLICE_FORCE=1)
SLICE_CASES = [
    Case(F64, 1, 40, 87, 24, 1, ("dense", "dep", "ones", "chain", "chainx"), NO_LIMIT, "slices R+V 127", "host"),      # aux rhs 128: wave0-fast, own overlapped
    Case(F64, 1, 40, 87, 24, 0, ("dense", "dep", "ones", "chain", "chainx"), NO_LIMIT, "slices R+V 127", "host"),
    Case(F64, 1, 40, 88, 24, 1, ("dense", "dep", "ones", "chain", "chainx"), NO_LIMIT, "slices R+V 128", "host"),
    Case(F64, 1, 64, 40, 24, 1, ("dense", "dep", "ones", "chain", "chainx"), NO_LIMIT, "slices rows 64", "host"),
    Case(F64, 1, 65, 40, 24, 1, ("dense", "dep", "ones", "chain", "chainx"), NO_LIMIT, "slices rows 65", "host"),
    Case(F64, 1, 20, 40, 24, 1, ("dense", "dep", "ones", "chain", "chainx"), NO_LIMIT, "slices 128 threads", "host"),
    Case(F64, 0, 20, 40, 24, 0, ("dense", "dep", "ones", "chain", "chainx"), NO_LIMIT, "slices 128 threads", "host"),
    Case(RAT, 1, 20, 40, 12, 1, ("dense", "dep", "ones", "chain", "chainx"), NO_LIMIT, "slices 128 threads", "host"),
    Case(F64, 1, 16, 30, 24, 1, ("dense", "dep", "ones", "chain", "chainx"), NO_LIMIT, "slices 64 threads", "host"),
    Case(F64, 1, 40, 87, 24, 1, ("dense", "dep", "ones", "chain", "chainx"), 23, "slices R+V 127 limit 23", "host"),
]


# ---- exact arithmetic -----------------------------------------------------------------------------------------------------
def exact_max(A, b, c):
    """maximise c.x, A x <= b, x >= 0 on Fractions: ("optimal", value) / ("unbounded", None) / ("infeasible", None).
    A plain dictionary simplex with Bland's rule (smallest index enters, smallest index among the tied ratios leaves) and an
    auxiliary variable for a negative right-hand side; nothing of the kernel's pair table, pricing order or stage 1."""
    R, V = len(A), len(c)
    n = V + R                                              # x_0..x_{V-1}, slacks x_V..x_{n-1}; aux x_n
    rows = [[Fraction(0)] * (n + 2) for _ in range(R)]     # row i: basic[i] + sum_j rows[i][j] x_j = rows[i][n + 1]
    for i in range(R):
        for j in range(V):
            rows[i][j] = Fraction(A[i][j])
        rows[i][V + i] = Fraction(1)
        rows[i][n + 1] = Fraction(b[i])
    basic = [V + i for i in range(R)]

    def pivot(r, col, objs):
        p = rows[r][col]
        rows[r] = [x / p for x in rows[r]]
        for i in range(R):
            if i != r and rows[i][col] != 0:
                f = rows[i][col]
                rows[i] = [x - f * y for x, y in zip(rows[i], rows[r])]
        for o in objs:
            if o[col] != 0:
                f = o[col]
                o[:] = [x - f * y for x, y in zip(o, rows[r])]
        basic[r] = col

    def run(obj, objs, allowed):
        """obj: reduced costs z - sum obj[j] x_j ... kept as row 'obj[j]' = -(reduced cost), obj[n + 1] = -value."""
        while True:
            enter = next((j for j in allowed if obj[j] < 0 and j not in basic), None)
            if enter is None:
                return True
            best = None
            for i in range(R):
                if rows[i][enter] > 0:
                    q = rows[i][n + 1] / rows[i][enter]
                    if best is None or q < best[0] or (q == best[0] and basic[i] < basic[best[1]]):
                        best = (q, i)
            if best is None:
                return False
            pivot(best[1], enter, objs)

    obj = [Fraction(-x) for x in c] + [Fraction(0)] * (R + 2)          # z row: z - c.x = 0
    if min(Fraction(x) for x in b) < 0:
        for i in range(R):
            rows[i][n] = Fraction(-1)
        aux = [Fraction(0)] * (n + 2)
        aux[n] = Fraction(1)                                              # maximise -x_n: w + x_n = 0
        r0 = min(range(R), key=lambda i: (rows[i][n + 1], i))
        pivot(r0, n, [obj, aux])
        run(aux, [obj, aux], range(n + 1))
        if aux[n + 1] != 0:
            return "infeasible", None
        if n in basic:                                                    # degenerate: drive it out
            r = basic.index(n)
            col = next(j for j in range(n) if rows[r][j] != 0)
            pivot(r, col, [obj, aux])
        for i in range(R):
            rows[i][n] = Fraction(0)
    if not run(obj, [obj], range(n)):
        return "unbounded", None
    return "optimal", obj[n + 1]


def frac(x):
    """A cell of either kind as a Fraction (fp64 cells are dyadic rationals: exact)."""
    if isinstance(x, np.ndarray) and x.shape == (2,):
        return Fraction(int(x[0]), int(x[1]))
    return Fraction(float(x))
