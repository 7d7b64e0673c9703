"""CPU suite: which variable constraints the device tree walk of MIP takes, and which shapes fit it. Host-only views of the
library (xpg_test_vc_pattern, xpg_test_mip_fits): no device is opened."""
import ctypes as C

import numpy as np
import pytest

from tools import gen

F64, RAT = 0, 1
XPG_ERR_SHAPE = -3


def _lib():
    from xpoly_amd import build, _capi
    build.build()
    return _capi.lib()


def _as(vc, kind):
    return np.ascontiguousarray(vc, dtype=np.float64) if kind == F64 else gen.to_rat(vc)


def _pattern(vc, kind, vc_rows=None):
    nv = vc.shape[0]
    a = _as(vc, kind)
    out = np.full(nv, 7, dtype=np.uint8)
    rc = _lib().xpg_test_vc_pattern(C.c_int(kind), a.ctypes.data_as(C.c_void_p), C.c_int(nv if vc_rows is None else vc_rows),
                                    C.c_int(nv + 1), out.ctypes.data_as(C.c_void_p))
    return rc, out


@pytest.mark.parametrize("kind", [F64, RAT])
def test_sign_patterns_are_recognised_with_their_free_variables(kind):
    for nv in (1, 4, 9):
        rc, free = _pattern(gen.vc_nonneg(nv, False), kind)                      # -I: nothing free
        assert rc == 1 and not free.any()
        for fs in ((), (1,), tuple(range(nv))):
            fs = tuple(j for j in fs if j < nv)
            rc, free = _pattern(gen.vc_nonneg(nv, False, fs), kind)
            assert rc == 1, (nv, fs)
            assert tuple(np.flatnonzero(free)) == fs, (nv, fs, free)


@pytest.mark.parametrize("kind", [F64, RAT])
def test_every_other_vc_is_general(kind):
    nv = 5
    base = gen.vc_nonneg(nv, False, (2,))
    for change in (lambda v: v.__setitem__((0, 0), -2),                          # a diagonal other than -1 / 0
                   lambda v: v.__setitem__((3, 3), 1),
                   lambda v: v.__setitem__((1, nv), -1),                         # a nonzero constant
                   lambda v: v.__setitem__((2, nv), 3),                          # ... in a free variable's row
                   lambda v: v.__setitem__((0, 2), 1),                           # an off-diagonal cell in a zero-diagonal column
                   lambda v: v.__setitem__((4, 1), -1)):
        vc = base.copy()
        change(vc)
        rc, _ = _pattern(vc, kind)
        assert rc == 0, vc
    rc, _ = _pattern(base, kind)
    assert rc == 1


@pytest.mark.parametrize("kind", [F64, RAT])
def test_wrong_vc_rows_is_a_shape_error(kind):
    vc = gen.vc_nonneg(4, False)
    assert _pattern(vc, kind, vc_rows=3)[0] == XPG_ERR_SHAPE
    assert _pattern(vc, kind, vc_rows=5)[0] == XPG_ERR_SHAPE


def _small_lds_bytes(R, V):
    """small_lds_bytes of batch_kernels.hip.h restated: the LDS arrays of one LP with R rows and V variables."""
    Wmax = V + 1 + R + 1
    nmax = Wmax - 1
    pw = (nmax + 31) // 32
    b = R * Wmax * 8 + Wmax * 8 * 3 + ((R + 1) & ~1) * 8 + 16 * 16
    b += nmax * 4 * 3 + R * 4 + nmax * pw * 4 + 16 * 4 + 8 * 4 + ((nmax + 3) & ~3) * 2
    return (b + 15) & ~15


def _fits_restated(leq_rows, eq_rows, cols, is_bin, extra):
    n = cols - 1
    rmax = leq_rows + (0 if is_bin else n)
    if eq_rows > 0:
        rmax += 2 * (eq_rows + (n if is_bin else 0))
    if rmax <= 0 or eq_rows + n + 2 > 256:
        return 0
    return int(_small_lds_bytes(rmax, n + extra) <= 65536 and _small_lds_bytes(n + extra, rmax) <= 65536)


def _fits(kind, leq_rows, eq_rows, cols, is_bin, extra):
    return _lib().xpg_test_mip_fits(C.c_int(kind), C.c_int(leq_rows), C.c_int(eq_rows), C.c_int(cols), C.c_int(int(is_bin)), C.c_int(extra))


def test_mip_fits_without_free_variables_is_the_rule_the_walk_had():
    leq, _ = gen.knapsack_batch_rat(2, 24)
    shapes = [(leq.shape[1], 0, leq.shape[2], True),                             # the bench's 0-1 knapsacks: 26 x 25
              (6, 0, 5, False), (12, 3, 7, False), (5, 2, 6, True), (0, 3, 5, False), (40, 0, 41, False), (64, 0, 65, False),
              (200, 0, 30, False), (30, 120, 20, True)]
    seen = set()
    for leq_rows, eq_rows, cols, is_bin in shapes:
        for kind in (F64, RAT):
            got = _fits(kind, leq_rows, eq_rows, cols, is_bin, 0)
            assert got == _fits_restated(leq_rows, eq_rows, cols, is_bin, 0), (leq_rows, eq_rows, cols, is_bin)
            seen.add(got)
    assert seen == {0, 1}
    assert _fits(RAT, leq.shape[1], 0, leq.shape[2], True, 0) == 1


def test_mip_fits_counts_the_twins_of_the_free_variables():
    """fp64, 50 inequalities x 21 columns, integer branching: the largest node LP has 70 rows. With 20 variables it needs
    about 56 KB of LDS; with the twins of 16 free variables about 66 KB, over the 64 KB a workgroup may have."""
    assert _small_lds_bytes(70, 20) <= 65536 < _small_lds_bytes(70, 36)
    assert 55 * 1024 < _small_lds_bytes(70, 20) < 58 * 1024 and 65 * 1024 < _small_lds_bytes(70, 36) < 68 * 1024
    assert _fits(F64, 50, 0, 21, False, 0) == 1
    assert _fits(F64, 50, 0, 21, False, 16) == 0
    for extra in range(0, 21):
        assert _fits(F64, 50, 0, 21, False, extra) == _fits_restated(50, 0, 21, False, extra), extra
    assert _fits(F64, 50, 0, 21, False, -1) == XPG_ERR_SHAPE
