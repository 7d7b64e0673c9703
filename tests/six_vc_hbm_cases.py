"""Shared by tests/test_six_batch_vc_hbm_host.py and tests/test_gpu_six_batch_vc_hbm.py: a Python restatement of the route rule
of xpg_six_batch_vc_hbm_* (csrc/six_batch_vc_hbm.hip.h: six_vc_hbm_plan, six_vc_hbm_slot), the batches the GPU cases are made of
and their answers from the CPU restatement of the reference (oracle.checker.Port().six_solve inside free_var_cases.non_strict --
the real reference is undefined with a free variable --, pivot counts from port.pivot_count(); computed once per case and
shared). Importing it needs no GPU and no library.

six_eq_cases.one_problem does not serve at these sizes: every LP of (64, 2, 64, 2) ends with status 2. The two families here
sit on top of batch_hbm_cases.mixed_batch / succ_batch (integer data, so both kinds get the same LPs); the free variables are
the FIRST nfree columns, so one vc serves a batch.

  "pairs"  twins and kept equality pairs, no substitution. Free columns f_k in front; per k two base variables a != b and a
           constant c (0 in even LPs, -3..3 in odd ones); while the shape has rows for it, the equality f_k - x_a + x_b = c and
           the same row times 2 -- equality rows left over are further multiples (3 x, 4 x, ...) of f_0's, so no column ever has
           exactly one equality and every equality stays as a pair. Inequalities i with i % 3 == k % 3 get t (f_k - x_a + x_b)
           on the left and t c on the right, t in {1, 2}; the objective gets (f_k - x_a + x_b).
  "fold"   substitution on device memory and ragged rows: "pairs" plus one dense equality g (coefficients 1..3 on every
           non-free variable, constant = their sum plus 0..4). In even LPs g stands alone, so the first column private to g is
           substituted into every inequality that has it (and a third multiple of f_0's equality keeps eq_rows equal across
           the batch); in odd LPs 2 g is added, nothing is substituted and both copies stay as pairs. One batch so holds normal
           forms of different row counts. The substitution reads its leading value at the inequality's ROW index
           (lpsol.h:1232): g is zero in the free columns, so inequalities 0 .. nfree - 1 give the substituted column up
           beforehand (a zero leading value is a division by zero in the reference). And it ADDS the equality's scaled cells
           in front of the constant column (:1241-1250), so an inequality with a positive coefficient there turns into an
           all-positive row under a constant of about -40 and the LP is infeasible after a pivot or two: the even LPs carry
           that column with non-positive coefficients, which leaves LPs that end with status 0.
  "tall"   (130, 1, 40, 1), maxm only: more inequalities than columns. One dense equality over every column, f_0 included, so
           column 0 is substituted. Even LPs have no f_0 in the rows q >= cols and solve; odd LPs have one there, lpsol.h:1232
           leaves the equality's row, and they alone end -7."""
import numpy as np

import batch_geometry as bg
import batch_hbm_cases as hc
import six_eq_cases as sc
from free_var_cases import F64, RAT, non_strict
from tools import gen

LDS_MAX = bg.LDS_MAX
SIX_VC_LDS_MAX = 64 * 1024
MAX_EQ = 4096
SCRATCH_MAX = 256 << 20
LDS_STATIC = 256 + 16                    # six_batch_vc_hbm.hip.h SIX_VC_HBM_LDS_STATIC: the solver's reduction scratch + hdr[4]
THREADS, WAVES_PER_CU = 256, 16
ROUTE_LDS, ROUTE_HBM, ROUTE_OTHER = 0, 1, 2
NO_LIMIT = 0xFFFFFFFF
FIELDS = ("route", "nfree", "Rmax", "Vmax", "lds", "slot", "ld", "threads", "grid", "scratch")

# (leq_rows, eq_rows, nv, nfree)
FIRST = (60, 4, 62, 2)                   # the smallest past 64 KB in both directions: 81 808 / 77 472 bytes (fp64)
ODD = (61, 4, 62, 2)                     # the other parity of V + R + 2
SPLIT = (30, 3, 130, 2)                  # maxm fits 64 KB (60 256 bytes), minm does not (191 968): the same arrays take both kernels
TALL = (130, 1, 40, 1)                   # leq_rows > cols: lpsol.h:1232 leaves the row; maxm only
PAIRS_SHAPES = (FIRST, ODD, SPLIT)
FOLD_SHAPES = ((60, 6, 62, 2), (61, 6, 62, 2))       # FIRST and ODD with g and its companion row
SUCC_SHAPES = {True: (96, 4, 103, 2), False: (101, 4, 98, 2)}
COUNT, RAT_COUNT, SUCC_COUNT = 64, 8, 16
CAPS, RAT_CAP = (300, 48), 48


# ---- mirror of the host rule ----------------------------------------------------------------------------------------------
def even(c):
    return (c + 1) & ~1


def slot_cells(leq_rows, eq_rows, cols, nfree, Rmax, ld):
    """six_vc_hbm_slot: fv | L | E | rest | N | obj | y | v | tab, every section on a 16-byte line, the slot on a 256-byte one."""
    n0, n, rows_max = cols - 1, cols - 1 + nfree, leq_rows + 2 * eq_rows
    o = even((n0 + 1) // 2) + even(leq_rows * cols) + even(eq_rows * cols) + even((eq_rows + 1) // 2)
    o += even(rows_max * (n + 1)) + 2 * even(n + 1) + 2 + Rmax * ld
    return (o + 31) & ~31


def lds_slot_cells(leq_rows, eq_rows, cols, nfree):
    """six_vc_slot (six_batch_vc.hip.h): fv | N | obj | y | v."""
    n0, n, rows_max = cols - 1, cols - 1 + nfree, leq_rows + 2 * eq_rows
    return ((n0 + 1) // 2 + rows_max * (n + 1) + 2 * (n + 1) + 1 + 31) & ~31


def lds_geometry(kind, nfree, nb, leq_rows, eq_rows, cols, is_max):
    """six_vc_geometry: (lds, threads, grid, slot cells) of k_six_batch_vc's launch; nfree < 0: the _dev form."""
    cap = nfree if nfree >= 0 else cols - 1
    least = sc.plan_bytes(leq_rows, eq_rows, cols - 1, max(nfree, 0), is_max, kind)
    lds = min(sc.plan_bytes(leq_rows, eq_rows, cols - 1, cap, is_max, kind), SIX_VC_LDS_MAX)
    del least
    rows, n = leq_rows + 2 * eq_rows, cols - 1 + max(nfree, 0)
    R, V = (rows, n) if is_max else (n, rows)
    cells = lds_slot_cells(leq_rows, eq_rows, cols, cap)
    grid = min(256 * min(max(LDS_MAX // lds, 1), 16) * 64, nb)
    by_scratch = SCRATCH_MAX // (cells * 8)
    if grid > by_scratch:
        grid = max(by_scratch, 1)
    return lds, bg.thread_rule(R, V), grid, cells


def plan(kind, pattern, nfree, leq_rows, eq_rows, cols, is_max, nb, cus=256):
    """six_vc_hbm_plan<S> as the dict xpoly_amd.six.six_batch_vc_hbm_plan returns. nfree < 0: the _dev forms (every variable
    taken as free); a general vc: pattern False, nfree 0."""
    cap = nfree if nfree >= 0 else cols - 1
    rows_max, n = leq_rows + 2 * eq_rows, cols - 1 + cap
    Rmax, Vmax = (rows_max, n) if is_max else (n, rows_max)
    full = bg.small_lds_bytes(kind, Rmax, Vmax)
    out = dict(nfree=nfree if nfree >= 0 else -1, Rmax=Rmax, Vmax=Vmax)
    if pattern and full <= SIX_VC_LDS_MAX and eq_rows <= MAX_EQ:
        lds, threads, grid, cells = lds_geometry(kind, nfree, nb, leq_rows, eq_rows, cols, is_max)
        assert lds == full
        out.update(route=ROUTE_LDS, lds=full, slot=cells * 8, ld=Vmax + Rmax + 2, threads=threads, grid=grid, scratch=grid * cells * 8)
        return out
    ld = (Vmax + Rmax + 2 + 1) & ~1
    lds = hc.side_bytes(kind, Rmax, Vmax)
    slot = slot_cells(leq_rows, eq_rows, cols, cap, Rmax, ld) * 8
    out.update(lds=lds, slot=slot, ld=ld, threads=THREADS)
    if not pattern or eq_rows > MAX_EQ or lds + LDS_STATIC > LDS_MAX or slot > SCRATCH_MAX:
        out.update(route=ROUTE_OTHER, grid=0, scratch=0)
        return out
    per_cu = max(1, min(WAVES_PER_CU * 64 // THREADS, LDS_MAX // (lds + LDS_STATIC)))
    grid = max(1, min(cus * per_cu, SCRATCH_MAX // slot, nb))
    out.update(route=ROUTE_HBM, grid=grid, scratch=grid * slot)
    return out


def plan_of_shape(kind, shape, is_max, nb, cus=256, dev=False):
    m, me, nv, nfree = shape
    return plan(kind, True, -1 if dev else nfree, m, me, nv + 1, is_max, nb, cus)


# ---- the families ---------------------------------------------------------------------------------------------------------
def _base(shape, is_max, count, succ):
    """The inequality-only LPs under a shape: (leq [count, m, nvb + 1], tgtf [count, nvb + 1]) as float64 holding integers
    (mixed_batch) or the block LPs that end SIX_SUCC (succ_batch, fp64 only)."""
    m, _, nv, nfree = shape
    nvb = nv - nfree
    if succ:
        leq, tg = hc.succ_batch(is_max, count)
    else:
        R, V = bg.solved_as(is_max, m, nvb + 1)
        leq, tg = hc.mixed_batch(F64, is_max, R, V, count, 0)
    assert leq.shape == (count, m, nvb + 1), (leq.shape, shape)
    return np.array(leq, dtype=np.float64), np.array(tg, dtype=np.float64)


def _pairs_arrays(shape, is_max, count, succ=False, eq_rows=None):
    m, me, nv, nfree = shape
    me = me if eq_rows is None else eq_rows
    nvb = nv - nfree
    bl, bt = _base(shape, is_max, count, succ)
    rng = np.random.default_rng([20261018, m, me, nv, nfree, int(is_max), int(succ)])
    leq = np.zeros((count, m, nv + 1)); tg = np.zeros((count, nv + 1)); eq = np.zeros((count, me, nv + 1))
    leq[:, :, nfree:] = bl; tg[:, nfree:] = bt
    for i in range(count):
        f_rows = []
        for k in range(nfree):
            a, b = (int(x) for x in rng.choice(nvb, 2, replace=False))
            c = 0 if i % 2 == 0 else int(rng.integers(-3, 4))
            row = np.zeros(nv + 1); row[k] = 1; row[nfree + a] = -1; row[nfree + b] = 1; row[nv] = c
            f_rows.append(row)
            for q in range(k % 3, m, 3):
                leq[i, q] += int(rng.integers(1, 3)) * row
            tg[i, :nv] += row[:nv]
        r = 0
        for k in range(nfree):
            if r + 2 <= me:
                eq[i, r] = f_rows[k]; eq[i, r + 1] = 2 * f_rows[k]; r += 2
        mult = 3
        while r < me:
            eq[i, r] = mult * f_rows[0]; r += 1; mult += 1
    return tg, eq, leq


def _fold_arrays(shape, is_max, count):
    m, me, nv, nfree = shape
    tg, eq0, leq = _pairs_arrays(shape, is_max, count, eq_rows=me - 2)
    rng = np.random.default_rng([20261019, m, me, nv, nfree, int(is_max)])
    eq = np.zeros((count, me, nv + 1))
    eq[:, :me - 2] = eq0
    for i in range(count):
        g = np.zeros(nv + 1)
        g[nfree:nv] = rng.integers(1, 4, size=nv - nfree)
        g[nv] = g[:nv].sum() + int(rng.integers(0, 5))
        eq[i, me - 2] = g
        if i % 2 == 0:
            eq[i, me - 1] = 3 * eq0[i, 0]
            # the column the reference will substitute: the first in which g alone has a nonzero
            j = next(c for c in range(nv) if np.count_nonzero(eq[i, :, c]) == 1)
            assert g[j] != 0
            leq[i, :, j] = -np.abs(leq[i, :, j])
            leq[i, :nfree, j] = 0
        else:
            eq[i, me - 1] = 2 * g
    return tg, eq, leq


def _tall_arrays(shape, count):
    m, me, nv, nfree = shape
    assert (me, nfree) == (1, 1) and m > nv + 1
    bl, bt = _base(shape, True, count, False)
    rng = np.random.default_rng([20261020, m, nv])
    leq = np.zeros((count, m, nv + 1)); tg = np.zeros((count, nv + 1)); eq = np.zeros((count, 1, nv + 1))
    leq[:, :, 1:] = bl; tg[:, 1:] = bt
    for i in range(count):
        g = np.zeros(nv + 1)
        g[:nv] = rng.integers(1, 4, size=nv)
        g[nv] = g[:nv].sum() + int(rng.integers(0, 5))
        eq[i, 0] = g
        leq[i, :, 0] = rng.integers(0, 3, size=m)
        if i % 2 == 0:
            leq[i, nv + 1:, 0] = 0
        else:
            leq[i, nv + 1 + int(rng.integers(0, m - nv - 1)), 0] = 1
        tg[i, 0] = 1
    return tg, eq, leq


_arrays = {}


def arrays(family, shape, kind, is_max, count):
    """(tgtf [count, cols(,2)], vc, eq [count, eq_rows, cols(,2)], leq [count, leq_rows, cols(,2)]) of `kind`, read-only."""
    key = (family, shape, bool(is_max))
    if key not in _arrays:
        full = SUCC_COUNT if family == "succ" else COUNT
        if family == "pairs":
            a = _pairs_arrays(shape, is_max, full)
        elif family == "succ":
            a = _pairs_arrays(shape, is_max, full, succ=True)
        elif family == "fold":
            a = _fold_arrays(shape, is_max, full)
        else:
            assert family == "tall" and is_max
            a = _tall_arrays(shape, full)
        _arrays[key] = a
    tg, eq, leq = (x[:count] for x in _arrays[key])
    nv, nfree = shape[2], shape[3]
    if kind == F64:
        out = (np.ascontiguousarray(tg), gen.vc_nonneg(nv, True, range(nfree)), np.ascontiguousarray(eq), np.ascontiguousarray(leq))
    else:
        for x in (tg, eq, leq):
            assert (x == np.floor(x)).all()
        out = (gen.to_rat(tg.astype(np.int32)), gen.to_rat(gen.vc_nonneg(nv, False, range(nfree))), gen.to_rat(eq.astype(np.int32)),
               gen.to_rat(leq.astype(np.int32)))
    for x in out:
        x.setflags(write=False)
    return out


_answers = {}


def oracle_answers(family, shape, kind, is_max, count, max_iter=NO_LIMIT):
    """[(status, v, sol, pivots)] of the restatement for the first `count` LPs of a case, computed once and shared."""
    key = (family, shape, kind, bool(is_max), int(max_iter))
    have = _answers.setdefault(key, [])
    if len(have) < count:
        port = hc._port()
        tg, vc, eq, leq = arrays(family, shape, kind, is_max, count)
        with non_strict(port):
            for i in range(len(have), count):
                p0 = port.pivot_count()
                st, v, sol = port.six_solve(kind, is_max, tg[i], vc, eq[i], leq[i], max_iter)
                have.append((int(st), v, sol, int(port.pivot_count() - p0)))
    return have[:count]


same_answer = hc.same_answer

# every fp64 case of the GPU suite: (family, shape, is_max); each runs under both CAPS on COUNT LPs
F64_CASES = ([("pairs", s, d) for s in PAIRS_SHAPES for d in (True, False)] + [("fold", s, d) for s in FOLD_SHAPES for d in (True, False)])
# Rational: RAT_COUNT LPs under RAT_CAP
RAT_CASES = [("pairs", FIRST, True), ("pairs", FIRST, False)] + [("fold", s, d) for s in FOLD_SHAPES for d in (True, False)]
