"""Shared by tests/test_r32_loop_host.py (no GPU), tests/test_gpu_r32_loop_geometry.py and its child process
tests/r32_loop_worker.py: the launch geometries of the two HBM-resident Rational simplex loops (lp_fused_r32.hip.h, one launch
per pivot; lp_pipe_r32.hip.h, two launches) and the LPs that reach them.

* plan(): a Python mirror of r32_loop_plan (lp_host.hip.h, shown to tests as xpg_test_r32_loop_plan).
* CASES: the smallest shapes that reach every branch of that plan -- N pick workgroups 1 .. 16, a second (third) row per
  pick lane, every stager count NP, the max(m, N + NP) grid -- with LPs built so that pivots DO leave on second-round rows,
  on the lower row of two identical rows of one lane (i, i + lanes * N) and of two workgroups (i, i + lanes); the same
  shapes with random_problem families 1 and 2 (phase one, ties, degenerate steps), and non-canonical variants (cells scaled
  by k/k, n/0 cells) that send the loop to the generic forms and to the `weird` hand-off.
* replay(): K pivots of SIX::pivot (lpsol.h:1471-1510) on fractions.Fraction for a set of columns -- arithmetic that is
  none of this project's -- valid where no float32 rescue happened (Port.appro_count unchanged; the host test asserts it).
W = nv + m + 1 for a plain TwoStageMethod problem that is feasible at the origin."""
import ctypes as C
import zlib
from fractions import Fraction

import numpy as np

from tools import gen

RAT = 1
NONE, FUSED, PIPE = 0, 1, 2                       # the `forced` argument: XPG_R32_LOOP unset / fused / pipe
PICK_MAX_WGS = 16
FUSED_FROM, FUSED_UPTO = 350000, 5000000          # cells: where the size rule takes the one-launch loop
PLAN_FIELDS = ("fused", "fN", "fNP", "fgx", "fgy", "frows", "pN", "pNP", "pgx", "pgy", "prows")


def plan(m, W, forced=NONE):
    cells = m * W
    fused = 0 if forced == PIPE else int(forced == FUSED or FUSED_FROM <= cells <= FUSED_UPTO)
    NP = -(-W // 256)
    fN = min(-(-m // 64), PICK_MAX_WGS)
    pN = min(-(-m // 256), PICK_MAX_WGS)
    return dict(fused=fused, fN=fN, fNP=NP, fgx=max(m, fN + NP), fgy=1 + NP, frows=-(-m // (64 * fN)),
                pN=pN, pNP=NP, pgx=max(m, pN), pgy=1 + NP, prows=-(-m // (256 * pN)))


def lib_plan(m, W, forced=NONE):
    from xpoly_amd._capi import lib
    o = (C.c_int32 * 11)()
    rc = lib().xpg_test_r32_loop_plan(C.c_int(m), C.c_int(W), C.c_int(forced), o, C.c_int(11))
    assert rc == 0, rc
    return dict(zip(PLAN_FIELDS, list(o)))


def stride(m, lanes):
    """Rows between two visits of one pick lane: lanes * N (lanes = 64: the fused loop's one-wave pick workgroups, 256: the
    two-launch loop's)."""
    return lanes * min(-(-m // lanes), PICK_MAX_WGS)


# ---- builders -------------------------------------------------------------------------------------------------------------
def craft(m, nv, lanes, seed=0, late=0):
    """An origin-feasible LP in int_lp_rat's ranges (A in 1..9, b = nv * {3, 4, 5}, c in 1..9) with, for the pick geometry of
    `lanes` rows per workgroup: up to six rows of the second round (i >= lanes * N) holding the smallest constant 2 * nv,
    up to three pairs i, i + lanes * N of identical rows (a tie inside one lane) and up to three pairs i, i + lanes (a tie
    between two pick workgroups), all with that constant; the row meant for column t has the column's largest entry.
    late > 0: the first `late` objective coefficients are 0, so the entering columns begin there (stager block edges).
    Returns (leq, tgtf, marks) -- marks: dict(alone=[row m - 1 where it is the last pick workgroup's only row], second=[rows], lane_pairs=[(i, i + S)], wg_pairs=[(i, i + lanes)])."""
    rng = np.random.default_rng([4404, seed, m, nv, lanes])
    A = rng.integers(1, 10, size=(m, nv))
    b = nv * rng.integers(3, 6, size=m)
    c = rng.integers(1, 10, size=nv)
    c[:late] = 0
    S = stride(m, lanes)
    used = set()
    second, lane_pairs, wg_pairs = [], [], []
    alone = [m - 1] if m > 1 and (m - 1) % lanes == 0 and m - 1 < S else []      # the one row of the last pick workgroup
    used.update(alone)
    if m > S:
        for i in sorted({int(x) for x in np.linspace(0, m - S - 1, 3)}):
            lane_pairs.append((i, i + S)); used.update((i, i + S))
        for i in sorted({int(x) for x in np.linspace(S, m - 1, 7)}):
            if i not in used and len(second) < 6:
                second.append(i); used.add(i)
    for i in (lanes - 1, 7, (min(S, m) // lanes // 2) * lanes + 11):
        if i + lanes < min(S, m) and i not in used and i + lanes not in used and len(wg_pairs) < 3:
            wg_pairs.append((i, i + lanes)); used.update((i, i + lanes))
    # the rows meant to leave, dealt to the columns in turn: second round, lane pair, workgroup pair, ...
    order, pools = list(alone), [list(second), [p[0] for p in lane_pairs], [p[0] for p in wg_pairs]]
    while any(pools):
        for pool in pools:
            if pool:
                order.append(pool.pop(0))
    for t, i in enumerate(order):
        A[i] = np.minimum(A[i], 8)
        if late + t < nv:
            A[i, late + t] = 9
        b[i] = 2 * nv
    for lo, hi in lane_pairs + wg_pairs:
        A[hi] = A[lo]; b[hi] = b[lo]
    leq = np.concatenate([A, b[:, None]], axis=1).astype(np.int32)
    tgtf = np.concatenate([c, [0]]).astype(np.int32)
    return gen.to_rat(leq), gen.to_rat(tgtf), dict(alone=alone, second=second, lane_pairs=lane_pairs, wg_pairs=wg_pairs)


def with_kk(leq, seed):
    """Some cells scaled by k/k: the same values, not in lowest terms (rational.cpp never reduces on construction), as
    tests/test_gpu_parity.py::test_rational_device_loop_with_fractions_not_in_lowest_terms does."""
    rng = np.random.default_rng([4405, seed])
    leq = leq.copy()
    m, cols = leq.shape[0], leq.shape[1]
    for _ in range(m):
        i, j, k = int(rng.integers(0, m)), int(rng.integers(0, cols)), int(rng.integers(2, 5))
        leq[i, j] = (leq[i, j, 0] * k, leq[i, j, 1] * k)
    return leq


def with_n0(m, nv, seed):
    """tests/crosscheck_unordered.py's LPs: signed sparse integers, positive constants, and a few n/0 cells -- values that
    Rational's cross-multiplying comparisons do not order -- also in the constant column."""
    rng = np.random.default_rng([4406, seed, m, nv])
    A = rng.integers(-3, 7, size=(m, nv)).astype(np.int32); A[rng.random((m, nv)) < 0.4] = 0
    b = (rng.integers(1, 4, size=m) * 6).astype(np.int32); c = rng.integers(-2, 5, size=nv).astype(np.int32)
    leq = gen.to_rat(np.concatenate([A, b[:, None]], axis=1)); tg = gen.to_rat(np.concatenate([c, [0]]).astype(np.int32))
    for _ in range(max(2, m // 40)):
        i, j = int(rng.integers(0, m)), int(rng.integers(0, nv + 1))
        leq[i, j] = (int(rng.choice([-2, -1, 1, 3])), 0)
    return leq, tg


# ---- the table ------------------------------------------------------------------------------------------------------------
# kind: "craft" (origin feasible; exact replay and minimum-ratio check), "wide" (craft with late entering columns),
#       "rand1" / "rand2" (random_problem families 1 / 2: phase one), "kk" / "n0" (non-canonical).
# loops: the forced loops the case runs on ("fused", "pipe"); every case also runs with no loop forced.
# Ks: the pivot budgets (always 1, an odd and an even count: either side of the ping-pong tableau is read back).
def _case(kind, m, nv, loops, Ks, lanes=64, seed=0, late=0, exact=False):
    return dict(name="%s-%dx%d%s" % (kind, m, nv, "-p" if lanes == 256 and kind == "craft" else ""), kind=kind, m=m, nv=nv, loops=loops,
                Ks=Ks, lanes=lanes, seed=seed, late=late, exact=exact)


BOTH = ("fused", "pipe")
TALL_KS = (1, 2, 5, 8)
WIDE_KS = (1, 2, 7, 12)
# (the seeds are part of the table: the first for which the checker's run has no float32 rescue -- the exact set -- is defined
# by the reference -- no status -7 -- and, for the n/0 variants, starts at the origin and does raise the `weird` hand-off)
FUSED_TALL = [(64, 6, 0), (65, 6, 0), (960, 7, 2), (961, 7, 0), (1024, 8, 0), (1025, 8, 0), (1088, 8, 0), (1100, 8, 0), (2049, 8, 0)]
FUSED_WIDE = [(33, 221, 4), (33, 222, 1), (33, 223, 0), (40, 471, 8), (40, 472, 3)]
CASES = (
    [_case("craft", m, nv, BOTH, TALL_KS, seed=s, exact=True) for m, nv, s in FUSED_TALL]
    # W = 255 / 256 / 257 / 512 / 513: one, two and three stagers, the constant column alone in the last block; the entering
    # columns begin at the block edge (late)
    + [_case("wide", m, nv, BOTH, WIDE_KS, seed=s, late=min(255, nv - 8), exact=True) for m, nv, s in FUSED_WIDE]
    + [_case("wide", 2, 600, BOTH, (1, 2, 3), late=255, exact=True)]             # N + NP = 4 > m = 2: the grid's other branch
    # the two-launch loop's own geometry: 256 rows per pick workgroup, a second row per lane above 4096 rows
    + [_case("craft", m, nv, BOTH, TALL_KS, lanes=256, exact=True) for m, nv in ((256, 8), (257, 8), (1025, 8))]
    + [_case("craft", 4100, 3, ("pipe",), (1, 2, 3, 4), lanes=256, exact=True)]
    + [_case("rand1", 1100, 12, BOTH, (1, 4, 9)), _case("rand2", 1100, 12, BOTH, (1, 4, 9)),
       _case("rand2", 65, 8, BOTH, (1, 3, 4, 1000)), _case("rand1", 961, 8, BOTH, (1, 4, 9))]
    + [_case("kk", 130, 40, BOTH, TALL_KS), _case("n0", 130, 40, BOTH, TALL_KS, seed=4),
       _case("kk", 300, 40, BOTH, TALL_KS), _case("n0", 300, 40, BOTH, TALL_KS, seed=18),
       _case("kk", 1100, 8, BOTH, TALL_KS), _case("n0", 1100, 8, BOTH, TALL_KS, seed=3)]
)
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# shapes on both sides of the two thresholds of the size rule (host test only)
SIZE_RULE = [(349, 1002, 0), (499, 701, 0), (350, 1000, 1), (500, 700, 1), (2000, 2500, 1), (1250, 4000, 1), (2000, 2501, 0), (1250, 4001, 0)]
SAMPLED = 16                                      # columns the exact replay follows besides the constant and the entering ones


def build(case):
    """(leq, tgtf, marks) of a case; marks is None unless the LP is crafted."""
    k, m, nv = case["kind"], case["m"], case["nv"]
    if k in ("craft", "wide"):
        return craft(m, nv, case["lanes"], case["seed"], case["late"])
    if k == "kk":
        leq, tg, marks = craft(m, nv, 64, case["seed"])
        return with_kk(leq, case["seed"]), tg, marks
    if k == "n0":
        leq, tg = with_n0(m, nv, case["seed"])
        return leq, tg, None
    fam = 1 if k == "rand1" else 2
    prob = gen.random_problem(np.random.default_rng([4407, fam, m, nv, case["seed"]]), RAT, fam, m, nv, plain=True)
    return prob["leq"], prob["tgtf"], None


def runs_in(case, env_loop):
    """env_loop: "fused" / "pipe" (forced) or None (the size rule decides)."""
    return env_loop is None or env_loop in case["loops"]


# ---- the checker with its pivot trace ----------------------------------------------------------------------------------------
def crc(a):
    return "%08x" % (zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF)


def two_stage_trace(port, leq, tgtf, K):
    """Port.two_stage plus the (entering, leaving) pairs (orc_two_stage_trace)."""
    leq = np.ascontiguousarray(leq, dtype=np.int32); tgtf = np.ascontiguousarray(tgtf, dtype=np.int32)
    m, cols = leq.shape[0], leq.shape[1]
    vc = np.zeros((cols - 1, cols, 2), dtype=np.int32); vc[..., 1] = 1
    vc[np.arange(cols - 1), np.arange(cols - 1), 0] = -1
    capc = cols + m + 1
    tab = np.zeros((m, capc, 2), dtype=np.int32); otg = np.zeros((capc, 2), dtype=np.int32)
    nv = np.zeros(capc, dtype=np.uint8); bv = np.zeros(capc, dtype=np.uint8)
    bv2eq = np.zeros(capc, dtype=np.int32); eq2bv = np.zeros(m, dtype=np.int32)
    orows, ocols, orhs, tlen = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    maxv = np.zeros((1, 2), dtype=np.int32); sol = np.zeros((capc, 2), dtype=np.int32)
    cap = 2 * 4096
    tr = np.zeros(cap, dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    fn = port.lib.orc_two_stage_trace
    fn.restype = C.c_int
    st = fn(C.c_int(RAT), vp(leq), C.c_int(m), C.c_int(cols), vp(vc), vp(tgtf), C.c_uint(K), vp(tab), C.byref(orows), C.byref(ocols),
            vp(otg), vp(nv), vp(bv), vp(bv2eq), vp(eq2bv), C.byref(orhs), vp(maxv), vp(sol), vp(tr), C.c_int(cap), C.byref(tlen))
    r, c, rhs = orows.value, ocols.value, orhs.value
    assert tlen.value <= cap
    return dict(status=st, tab=tab.reshape(-1)[: r * c * 2].reshape(r, c, 2).copy(), tgtf=otg[:c].copy(), nvset=nv[:rhs].copy(),
                bvset=bv[:rhs].copy(), bv2eq=bv2eq[:rhs].copy(), eq2bv=eq2bv[:r].copy(), rhs=rhs, maxv=maxv[0].copy(), sol=sol[:c].copy(),
                trace=tr[: tlen.value].reshape(-1, 2).copy())


END_STATES = (0, 1, 3)                            # SIX_SUCC, UNBOUND, OPTIMAL_IS_INFEASIBLE: the solve ended inside K


def record(res, case, K, cols=None):
    """What the GPU worker prints for one (case, K) and what the tests make of the checker's answer: status and CRC-32 of
    every array compared bit for bit (status 2 -- phase one did not finish -- leaves no state to compare)."""
    rec = dict(name=case["name"], K=K, status=int(res["status"]), trace=np.asarray(res["trace"]).reshape(-1).tolist())
    if res["status"] != 2:
        rec.update(tab=crc(res["tab"]), tgtf=crc(res["tgtf"]), nvset=crc(np.asarray(res["nvset"], dtype=np.uint8)),
                   bvset=crc(np.asarray(res["bvset"], dtype=np.uint8)), bv2eq=crc(np.asarray(res["bv2eq"], dtype=np.int32)),
                   eq2bv=crc(np.asarray(res["eq2bv"], dtype=np.int32)))
        if res["status"] == 0:
            rec.update(maxv=crc(res["maxv"]), sol=crc(res["sol"]))
        if cols is not None:
            rec["cols"] = [int(j) for j in cols]
            rec["tabcols"] = np.asarray(res["tab"])[:, cols].reshape(-1).tolist()
            rec["objcols"] = np.asarray(res["tgtf"])[cols].reshape(-1).tolist()
    return rec


def leaving_rows(m, nv, trace):
    """Rows the pivots of an origin-feasible solve left on: the basis bookkeeping of SIX::pivot (lpsol.h:1504-1510) replayed
    from the slack basis (row i holds slack nv + i)."""
    eq2bv = [nv + i for i in range(m)]
    bv2eq = {nv + i: i for i in range(m)}
    rows = []
    for enter, leave in trace:
        r = bv2eq.pop(int(leave))
        eq2bv[r] = int(enter); bv2eq[int(enter)] = r
        rows.append(r)
    return rows


def replay_cols(m, nv, trace):
    """The column set of the exact replay: the constant column, every entering column, SAMPLED others spread over the
    width (structural and slack columns)."""
    W = nv + m + 1
    cols = {W - 1} | {int(e) for e, _ in trace} | {int(x) for x in np.linspace(0, W - 2, SAMPLED)}
    return sorted(cols)


def replay(leq, tgtf, trace, cols, check_ratio=True):
    """K pivots of SIX::pivot (lpsol.h:1471-1510) in fractions.Fraction on the columns `cols` of the slack form [A | I | b]
    of an origin-feasible LP: a pivot updates column j from column j and the entering column alone, so the entering columns,
    the constant column and any sample can be followed without the rest. Returns (columns {j: [Fraction] * m}, objective
    {j: Fraction}, rows left). check_ratio: at every step the row left attains the minimum of b_i / a_i over the rows with
    a_i > 0 and is the lowest such row (lpsol.h:604-611), and the constant column stays >= 0."""
    leq = np.asarray(leq); tgtf = np.asarray(tgtf)
    m, nv = leq.shape[0], leq.shape[1] - 1
    W = nv + m + 1
    rhs = W - 1
    assert rhs in cols and all(int(e) in cols for e, _ in trace)

    def col0(j):
        if j < nv:
            return [Fraction(int(leq[i, j, 0]), int(leq[i, j, 1])) for i in range(m)]
        if j < rhs:
            return [Fraction(int(i == j - nv)) for i in range(m)]
        return [Fraction(int(leq[i, nv, 0]), int(leq[i, nv, 1])) for i in range(m)]

    col = {j: col0(j) for j in cols}
    obj = {j: (Fraction(int(tgtf[j, 0]), int(tgtf[j, 1])) if j < nv else Fraction(0)) for j in cols}
    rows = leaving_rows(m, nv, trace)
    for (enter, _), r in zip(trace, rows):
        enter = int(enter)
        a = col[enter]
        if check_ratio:
            b = col[rhs]
            assert all(x >= 0 for x in b), "constant column went negative"
            assert a[r] > 0, (enter, r)
            best = min(b[i] / a[i] for i in range(m) if a[i] > 0)
            lowest = min(i for i in range(m) if a[i] > 0 and b[i] / a[i] == best)
            assert r == lowest, ("row left", r, "lowest row of the minimum ratio", lowest)
        piv, cnv = a[r], obj[enter]
        k = [-x for x in a]                                         # coeff_of_nv, lpsol.h:1485 (before the row is scaled)
        for j in cols:
            cj = col[j]
            if cj[r] == 0:                                          # e = 0: every cell a + k * 0 = a, the objective likewise
                continue
            e = cj[r] / piv                                         # lpsol.h:1471
            col[j] = [e if i == r else cj[i] + k[i] * e for i in range(m)]    # lpsol.h:1481-1490
            obj[j] = obj[j] + cnv * (e if j >= rhs else -e)         # lpsol.h:1496-1501
    return col, obj, rows


def origin_feasible(port, leq, tgtf):
    """SIX::TwoStageMethod's own test (lpsol.h:1760-1770, :1907-1930): a positive objective coefficient and no negative
    constant -- else phase one runs first."""
    nv = leq.shape[1] - 1
    any_pos = any(port.rat_cmp(2, tuple(int(x) for x in tgtf[j]), (0, 1)) for j in range(nv))
    return any_pos and not any(port.rat_cmp(0, tuple(int(x) for x in leq[i, nv]), (0, 1)) for i in range(leq.shape[0]))


def weird_steps(port, leq, tgtf, K):
    """Pivots 1 .. K of an origin-feasible n/0 LP at which the first ratio pass meets what the pick workgroups hand to the
    generic pick: a candidate quotient with den <= 0, or a row left that is not the plain first-pass arg-min under
    Rational's comparisons (the checker's answers and its scalar operations alone)."""
    m, nv = leq.shape[0], leq.shape[1] - 1
    full = two_stage_trace(port, leq, tgtf, K)
    rows = leaving_rows(m, nv, full["trace"])
    out = []
    for t, ((enter, _), r) in enumerate(zip(full["trace"], rows)):
        st = two_stage_trace(port, leq, tgtf, t) if t else None
        tab = st["tab"] if st else None
        rhs = nv + m
        best, besti, bad = None, -1, False
        for i in range(m):
            if tab is None:
                a = tuple(int(x) for x in leq[i, enter]) if enter < nv else (int(i == enter - nv), 1)
                b = tuple(int(x) for x in leq[i, nv])
            else:
                a = tuple(int(x) for x in tab[i, enter]); b = tuple(int(x) for x in tab[i, rhs])
            if port.rat_cmp(1, a, (0, 1)):                          # IS_LE(a, 0), lpsol.h:575
                continue
            q = port.rat_op(1, b, a)
            bad |= q[1] <= 0
            if best is None or port.rat_cmp(2, best, q):
                best, besti = q, i
        if bad or besti != r:
            out.append(t + 1)
    return out


def facts(port, case):
    """What the GPU cases rest on, from the checker's answers alone (K = the case's largest budget): status, pivots made,
    whether phase one ran, float32 rescues; for the LPs that start at the origin the pivots (counted from 1) that left on the
    last workgroup's only row, on a second-round row, on the lower row of an identical pair of one lane / of two workgroups,
    on the UPPER row of a pair (never); the 256-column blocks of the entering and leaving variables (wide); the pivots whose
    ratio test is handed to the generic pick (n0)."""
    leq, tg, marks = build(case)
    K = max(case["Ks"])
    a0 = port.appro_count()
    res = two_stage_trace(port, leq, tg, K)
    f = dict(status=int(res["status"]), pivots=len(res["trace"]), phase_one=not origin_feasible(port, leq, tg), appro=int(port.appro_count() - a0))
    if f["phase_one"]:
        return f
    rows = leaving_rows(case["m"], case["nv"], res["trace"])
    step = lambda rs: [t + 1 for t, r in enumerate(rows) if r in rs]
    if marks:
        S = stride(case["m"], case["lanes"])
        f.update(alone=step(marks["alone"]), second=[t + 1 for t, r in enumerate(rows) if r >= S],
                 lane_lo=step([p[0] for p in marks["lane_pairs"]]), wg_lo=step([p[0] for p in marks["wg_pairs"]]),
                 upper=step([p[1] for p in marks["lane_pairs"] + marks["wg_pairs"]]))
    if case["kind"] == "wide":
        f.update(enter_blocks=sorted({int(e) // 256 for e, _ in res["trace"]}), leave_blocks=sorted({int(l) // 256 for _, l in res["trace"]}))
    if case["kind"] == "n0":
        f["weird"] = weird_steps(port, leq, tg, K)
    return f


# facts(port, case) of every case: recorded here so that a change of a builder, of a generator or of the checker that moves a
# pivot off the rows a case is about is seen (tests/test_r32_loop_host.py compares and checks what the table must reach)
EXPECT = {
    'craft-64x6': dict(status=4, pivots=8, phase_one=False, appro=0, alone=[], second=[], lane_lo=[], wg_lo=[], upper=[]),
    'craft-65x6': dict(status=4, pivots=8, phase_one=False, appro=0, alone=[1, 2], second=[], lane_lo=[], wg_lo=[], upper=[]),
    'craft-960x7': dict(status=4, pivots=8, phase_one=False, appro=0, alone=[], second=[], lane_lo=[], wg_lo=[1, 2, 7], upper=[]),
    'craft-961x7': dict(status=0, pivots=6, phase_one=False, appro=0, alone=[1, 3, 5], second=[], lane_lo=[], wg_lo=[2, 4, 6], upper=[]),
    'craft-1024x8': dict(status=4, pivots=8, phase_one=False, appro=0, alone=[], second=[], lane_lo=[], wg_lo=[1, 2, 3, 4, 5], upper=[]),
    'craft-1025x8': dict(status=4, pivots=8, phase_one=False, appro=0, alone=[], second=[], lane_lo=[1], wg_lo=[4, 8], upper=[]),
    'craft-1088x8': dict(status=4, pivots=8, phase_one=False, appro=0, alone=[], second=[1, 8], lane_lo=[2, 4, 7], wg_lo=[3, 5, 6], upper=[]),
    'craft-1100x8': dict(status=4, pivots=8, phase_one=False, appro=0, alone=[], second=[1, 4, 5, 7], lane_lo=[3, 6, 8], wg_lo=[2], upper=[]),
    'craft-2049x8': dict(status=4, pivots=8, phase_one=False, appro=0, alone=[], second=[1, 3, 6, 8], lane_lo=[2, 4, 5, 7], wg_lo=[], upper=[]),
    'wide-33x221': dict(status=4, pivots=12, phase_one=False, appro=0, alone=[], second=[], lane_lo=[], wg_lo=[], upper=[], enter_blocks=[0], leave_blocks=[0]),
    'wide-33x222': dict(status=0, pivots=6, phase_one=False, appro=0, alone=[], second=[], lane_lo=[], wg_lo=[], upper=[], enter_blocks=[0], leave_blocks=[0]),
    'wide-33x223': dict(status=4, pivots=12, phase_one=False, appro=0, alone=[], second=[], lane_lo=[], wg_lo=[], upper=[], enter_blocks=[0], leave_blocks=[0]),
    'wide-40x471': dict(status=4, pivots=12, phase_one=False, appro=0, alone=[], second=[], lane_lo=[], wg_lo=[], upper=[], enter_blocks=[0, 1], leave_blocks=[0, 1]),
    'wide-40x472': dict(status=4, pivots=12, phase_one=False, appro=0, alone=[], second=[], lane_lo=[], wg_lo=[], upper=[], enter_blocks=[0, 1], leave_blocks=[0, 1]),
    'wide-2x600': dict(status=4, pivots=3, phase_one=False, appro=0, alone=[], second=[], lane_lo=[], wg_lo=[], upper=[], enter_blocks=[0, 1], leave_blocks=[1, 2]),
    'craft-256x8-p': dict(status=4, pivots=8, phase_one=False, appro=0, alone=[], second=[], lane_lo=[], wg_lo=[], upper=[]),
    'craft-257x8-p': dict(status=4, pivots=8, phase_one=False, appro=0, alone=[1], second=[], lane_lo=[], wg_lo=[], upper=[]),
    'craft-1025x8-p': dict(status=4, pivots=8, phase_one=False, appro=0, alone=[1, 7], second=[], lane_lo=[], wg_lo=[2, 3, 4, 5, 6, 8], upper=[]),
    'craft-4100x3-p': dict(status=4, pivots=4, phase_one=False, appro=0, alone=[], second=[1], lane_lo=[2], wg_lo=[3, 4], upper=[]),
    'rand1-1100x12': dict(status=2, pivots=10, phase_one=True, appro=0),
    'rand2-1100x12': dict(status=2, pivots=3, phase_one=True, appro=0),
    'rand2-65x8': dict(status=2, pivots=4, phase_one=True, appro=0),
    'rand1-961x8': dict(status=2, pivots=10, phase_one=True, appro=0),
    'kk-130x40': dict(status=4, pivots=8, phase_one=False, appro=16, alone=[], second=[], lane_lo=[], wg_lo=[1, 2, 7, 8], upper=[]),
    'n0-130x40': dict(status=4, pivots=8, phase_one=False, appro=0, weird=[2, 4, 5, 6, 7, 8]),
    'kk-300x40': dict(status=4, pivots=8, phase_one=False, appro=0, alone=[], second=[], lane_lo=[], wg_lo=[1, 2, 4], upper=[]),
    'n0-300x40': dict(status=4, pivots=8, phase_one=False, appro=0, weird=[3]),
    'kk-1100x8': dict(status=4, pivots=8, phase_one=False, appro=0, alone=[], second=[1, 4, 5, 7], lane_lo=[3, 6, 8], wg_lo=[2], upper=[]),
    'n0-1100x8': dict(status=4, pivots=8, phase_one=False, appro=0, weird=[1, 3, 5, 6, 7, 8]),
}
