"""What tests/test_lineq_transform_host.py and tests/test_gpu_lineq_transform.py share: a restatement of the plan of a
transformed-nest call (lineq_host.hip.h transform_plan: the levels' plan with rhs_idx slots a system, a level's slot no smaller
than the nest, and the place of the inverse's scratch), the nests and transformations of the cases, and the composed checker --
oracle/checker.py's rat_det and rat_inv, its rat_op cell by cell in the order of the reference's operator* (src/com/matt.h:60-79),
and lineq_levels_cases.stepped_levels over the list rhs_idx-1 .. 1 -- with an independent check in fractions.Fraction. These
cases keep the Rational exact on purpose; the nests and transformations that make it approximate live in
tests/lineq_rescue_cases.py, tests/test_lineq_rescue_host.py and tests/test_gpu_lineq_rescue.py."""
from fractions import Fraction

import numpy as np

import lineq_levels_cases as lc
import lineq_project_cases as pc
from lineq_project_cases import XPG_ERR_SHAPE, XPG_ERR_UNSUPPORTED, rows_equal, CHAIN_MAX   # noqa: F401 (re-exported)

PLAN_KEYS = ("launches", "grid", "groups", "sys_lds", "cap_lds", "seat_bytes", "level_bytes", "cap", "cap_out", "inv_at")
ROUTE_KEYS = PLAN_KEYS[:7]
MUL, ADD, EQ, LT = 0, 2, 4, 0                         # oracle rat_op / rat_cmp codes


def inv_bytes(n):
    """LDS bytes of the inverse's scratch: [T | E] n x 2n, T's copy n x n, n row factors (8-byte cells), n live flags."""
    return ((3 * n * n + n) * 8 + n + 15) & ~15


def plan(nb, rows, cols, rhs, cap_rows=0, cap_out_rows=0):
    """The ten figures of xpg_test_lineq_transform_plan, or the error code."""
    if nb <= 0 or rows <= 0 or cols <= 1 or rhs < 1 or rhs >= cols:
        return XPG_ERR_SHAPE
    if rhs - 1 > CHAIN_MAX:
        return XPG_ERR_UNSUPPORTED
    if 0 < cap_out_rows < rows:
        return XPG_ERR_SHAPE
    if rows > 32767:
        return XPG_ERR_UNSUPPORTED
    cap = max(rows * rows // 4 + rows + 1 if cap_rows <= 0 else cap_rows, rows)
    cap_out = min(cap, 4 * rows + 16) if cap_out_rows <= 0 else min(cap_out_rows, cap)
    if cap > 32767:
        return XPG_ERR_UNSUPPORTED
    cap_lds, lds = pc.fme_lds(cap, cap, cols)
    inv_at = 0
    if inv_bytes(rhs) > (cap_lds + cap) * cols * 8:         # not in the walk's two areas: behind the walk's scratch
        inv_at = (lds + 15) & ~15
        lds = inv_at + inv_bytes(rhs)
    if lds > 160 * 1024:
        return XPG_ERR_UNSUPPORTED
    sys_lds = (lds + 15) & ~15
    grid = min(nb, 4096)                                     # fme takes the whole wave: one system per workgroup
    return dict(zip(PLAN_KEYS, (1, grid, 1, sys_lds, cap_lds, grid * 2 * cap * cols * 8, nb * rhs * cap_out * cols * 8, cap, cap_out,
                                inv_at)))


def plan_view(nb, rows, cols, rhs, cap_rows=0, cap_out_rows=0):
    """xpg_test_lineq_transform_plan (host only): the same dict, or the error code."""
    import ctypes as C
    from xpoly_amd._capi import lib
    out = np.zeros(10, dtype=np.int64)
    rc = lib().xpg_test_lineq_transform_plan(C.c_int(nb), C.c_int(rows), C.c_int(cols), C.c_int(rhs), C.c_int(cap_rows),
                                             C.c_int(cap_out_rows), out.ctypes.data_as(C.c_void_p), C.c_int(10))
    return rc if rc != 0 else dict(zip(PLAN_KEYS, (int(x) for x in out)))


# ---- the cases' data: every entry within |.| <= 3 ---------------------------------------------------------------------------------
def to_rat(m):
    a = np.asarray(m, dtype=np.int32)
    out = np.empty(a.shape + (2,), dtype=np.int32)
    out[..., 0] = a
    out[..., 1] = 1
    return out


def nest(n, consts=1):
    """A triangular nest of depth n as A * i <= C, [rows, n + consts, 2]: 0 <= i0 <= 3 (+ N), 0 <= ik <= i(k-1) + 2. Depth 1 has
    a second pair of bounds so that it has 4 rows too; depth 2, 3, 4 have 4, 6, 8."""
    rows = []
    for k in range(n):
        lo = [0] * (n + consts); lo[k] = -1
        up = [0] * (n + consts); up[k] = 1
        if k:
            up[k - 1] = -1
        up[n] = 3 if k == 0 else 2
        if consts == 2 and k != 1:
            up[n + 1] = 1                                    # a symbolic extent N
        rows += [lo, up]
    if n == 1:
        lo = [0] * (n + consts); lo[0] = -1; lo[n] = 1
        up = [0] * (n + consts); up[0] = 2; up[n] = 3
        rows += [lo, up]
    return to_rat(rows)


def empty_nest(n, at):
    """The nest of depth n >= 2 with i(at) >= i(at-1) + 1 added against i(at) <= i(at-1) - 1: no point, and fme finds it when
    variable `at` goes."""
    a = nest(n)[..., 0].tolist()
    lo = [0] * (n + 1); lo[at] = -1; lo[at - 1] = 1; lo[n] = -1
    up = [0] * (n + 1); up[at] = 1; up[at - 1] = -1; up[n] = -1
    return to_rat(a[:2 * at] + [lo, up] + a[2 * at + 2:])


def _eye(n):
    return np.eye(n, dtype=np.int64)


def tmats(n):
    """{name: T [n, n, 2]} -- the kinds of the cases at depth n."""
    out = {"identity": to_rat(_eye(n))}
    rev = _eye(n); rev[n - 1, n - 1] = -1
    out["reversal"] = to_rat(rev)
    sing = _eye(n); sing[n - 1] = sing[0] if n > 1 else 0
    out["singular"] = to_rat(sing)
    two = _eye(n); two[0, 0] = 2
    out["diag2"] = to_rat(two)
    non = to_rat(_eye(n)); non[0, 0] = (2, 2)
    out["noncanonical"] = non
    if n >= 2:
        ic = _eye(n); ic[[0, 1]] = ic[[1, 0]]
        lower = _eye(n); lower[1, 0] = 1
        upper = _eye(n); upper[0, 1] = 1
        out.update(interchange=to_rat(ic), lower=to_rat(lower), upper=to_rat(upper))
        dense = lower @ upper @ ic @ rev
        if n >= 3:
            lo2 = _eye(n); lo2[n - 1, 0] = -1
            up2 = _eye(n); up2[1, n - 1] = 1
            dense = lo2 @ dense @ up2
        assert np.abs(dense).max() <= 3, dense
        out["dense"] = to_rat(dense)
    return out


# ---- the composed checker -----------------------------------------------------------------------------------------------------------
def _cell(c):
    return int(c[0]), int(c[1])


def product(port, a, m, n):
    """(a[:, :n] * m | a[:, n:]): operator* (matt.h:60-79) -- tmp = 0, tmp = tmp + a(i,k) * m(k,j), k ascending -- with the
    checker's own '+' and '*'; the other columns bit for bit."""
    out = np.array(a, dtype=np.int32, copy=True)
    for i in range(a.shape[0]):
        for j in range(n):
            tmp = (0, 1)
            for k in range(n):
                tmp = port.rat_op(ADD, tmp, port.rat_op(MUL, _cell(a[i, k]), _cell(m[k, j])))
            out[i, j] = tmp
    return out


def kind_of(port, t):
    """(kind, det, M or None) as k_transform_levels_batch decides in mode 0: det first (ldtran.cpp:148), then inv (:160)."""
    det = port.rat_det(t)
    if port.rat_cmp(EQ, det, (0, 1)):
        return 1, det, None
    mag = (-det[0], det[1]) if port.rat_cmp(LT, det, (0, 1)) else det
    if not port.rat_cmp(EQ, mag, (1, 1)):
        return 2, det, None
    ok, m = port.rat_inv(t)
    return (0, det, m) if ok else (1, det, None)


def transformed(port, a, t, mode=0, cap_rows=None, cap_out_rows=None):
    """(ok, steps, kind, det, mult, levels, needs, sizes) of one system: a [rows, cols, 2], t [n, n, 2]. levels has n entries,
    level 0 the transformed nest; a system of kind 1 or 2 or with ok <= 0 has every level empty. needs / sizes as
    lineq_levels_cases.stepped_levels gives them for the steps."""
    a, t = np.asarray(a, dtype=np.int32), np.asarray(t, dtype=np.int32)
    n = t.shape[0]
    empty = np.zeros((0, a.shape[1], 2), dtype=np.int32)
    kind, det, m = (0, None, t) if mode == 1 else kind_of(port, t)
    if kind:
        return 1, 0, kind, det, np.zeros((n, n, 2), dtype=np.int32), [empty] * n, [], []
    a1 = product(port, a, m, n)
    ok, steps, levels, needs, sizes = lc.stepped_levels(port, a1, n, list(range(n - 1, 0, -1)), False, cap_rows, cap_out_rows)
    return ok, steps, 0, det, np.asarray(m), [a1 if ok == 1 else empty] + levels, needs, sizes


def _frac(m):
    return [[Fraction(int(c[0]), int(c[1])) for c in row] for row in m]


def exact_check(a, t, mult, level0, mode):
    """Independent of the checker, in exact arithmetic: level0[:, :n] * T == a[:, :n], the constant columns are unchanged, and
    M * T == I (mode 0; in mode 1 `t` is M itself: level0[:, :n] == a[:, :n] * M)."""
    n = len(t)
    fa, ft, fm, f0 = _frac(a), _frac(t), _frac(mult), _frac(level0)
    eye = [[Fraction(int(i == j)) for j in range(n)] for i in range(n)]
    mul = lambda x, y: [[sum(x[i][k] * y[k][j] for k in range(n)) for j in range(n)] for i in range(len(x))]
    if mode == 0:
        assert mul(fm, ft) == eye, (mult, t)
        assert mul([r[:n] for r in f0], ft) == [r[:n] for r in fa]
    else:
        assert fm == ft and [r[:n] for r in f0] == mul([r[:n] for r in fa], ft)
    assert np.array_equal(np.asarray(level0)[:, n:], np.asarray(a)[:, n:])


def check(got, want, tag=()):
    """(ok, steps, kind, det, mult, levels) of a call against [transformed(...)] system by system, bit for bit."""
    ok, steps, kind, det, mult, levels = got
    assert len(ok) == len(want)
    for b, w in enumerate(want):
        assert (ok[b], steps[b], kind[b]) == (w[0], w[1], w[2]), tag + (b, ok[b], steps[b], kind[b], w[:3])
        if w[3] is not None:
            assert tuple(det[b]) == tuple(w[3]), tag + (b, det[b], w[3])
        assert np.array_equal(mult[b], w[4]), tag + (b, "mult")
        assert len(levels[b]) == len(w[5])
        for k, wl in enumerate(w[5]):
            assert rows_equal(levels[b][k], wl), tag + (b, k)
        if w[0] <= 0 or w[2]:
            assert all(lv.shape[0] == 0 for lv in levels[b]), tag + (b,)
