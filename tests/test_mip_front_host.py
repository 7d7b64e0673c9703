"""CPU suite: the one route rule of the MIP entry points (mip_front_route, mip_host.hip.h) -- device tree walk or host
controller -- through the host-only view xpg_test_mip_front_route (no device is opened), against the four rules as
xpg_mip_maxm / minm_*, xpg_mip_batch_*, xpg_mip_batch_eq_* and xpg_mip_batch_vc_* each stated their own before there was
one."""
import ctypes as C
import itertools

import pytest

import batch_geometry as bg
from batch_geometry import F64, RAT

XPG_ERR_SHAPE = -3
MIP_EQ_MAX = 256                      # mip_kernels.hip.h
LDS_WALK = 64 * 1024                  # what k_mip_tree takes for the node LP's arrays
FIT_LAUNCH, FIT_BOTH = 0, 1           # mip_host.hip.h MipFit
HOST, DEVICE = 0, 1


def _view(fit, kind, pattern, extra, leq_rows, eq_rows, cols, is_bin, is_max, allowed):
    from xpoly_amd._capi import lib
    return lib().xpg_test_mip_front_route(*(C.c_int(int(x)) for x in (fit, kind, pattern, extra, leq_rows, eq_rows, cols, is_bin, is_max, allowed)))


def _rmax(leq_rows, eq_rows, n, is_bin):
    """mip_rmax: the rows of the largest node LP of the deepest path."""
    r = leq_rows + (0 if is_bin else n)
    if eq_rows > 0:
        r += 2 * (eq_rows + (n if is_bin else 0))
    return r


def _device_fits(kind, leq_rows, cols, is_bin, eq_rows, extra):
    """mip_device_fits: the largest node LP fits the walk maximising AND minimising, its equality list fits the node."""
    n = cols - 1
    rmax = _rmax(leq_rows, eq_rows, n, is_bin)
    if rmax <= 0 or eq_rows + n + 2 > MIP_EQ_MAX or extra < 0 or extra > n:
        return False
    return bg.small_lds_bytes(kind, rmax, n + extra) <= LDS_WALK and bg.small_lds_bytes(kind, n + extra, rmax) <= LDS_WALK


def _launch_takes(kind, leq_rows, cols, is_bin, is_max, eq_rows, extra):
    """What mip_batch_device itself refuses (XPG_ERR_UNSUPPORTED): the LDS of the direction asked for, mip_geom's."""
    n = cols - 1 + extra
    rmax = _rmax(leq_rows, eq_rows, cols - 1, is_bin)
    R, V = (rmax, n) if is_max else (n, rmax)
    return bg.small_lds_bytes(kind, R, V) <= LDS_WALK


# The four fronts: (fit mode the entry point asks the one rule with, whether its argument check takes the call, its own rule).
def _mip_batch(kind, pattern, extra, m, me, cols, is_bin, is_max, allowed):
    """x >= 0, inequalities only: the switch, then straight to the launch."""
    if not (m > 0 and me == 0 and pattern and extra == 0):
        return None
    return allowed and _launch_takes(kind, m, cols, is_bin, is_max, 0, 0)


def _mip_batch_eq(kind, pattern, extra, m, me, cols, is_bin, is_max, allowed):
    """x >= 0, equalities at the root: the switch and mip_device_fits."""
    if not (me > 0 and pattern and extra == 0):
        return None
    return allowed and _device_fits(kind, m, cols, is_bin, me, 0)


def _mip_batch_vc(kind, pattern, extra, m, me, cols, is_bin, is_max, allowed):
    """The caller's vc: the switch, a sign pattern, mip_device_fits with its free variables. mip_solve's rule is the same."""
    if m == 0 and me == 0:
        return None
    return allowed and pattern and _device_fits(kind, m, cols, is_bin, me, extra)


FRONTS = (("mip_batch", FIT_LAUNCH, _mip_batch), ("mip_batch_eq", FIT_BOTH, _mip_batch_eq), ("mip_batch_vc", FIT_BOTH, _mip_batch_vc),
          ("mip_solve", FIT_BOTH, _mip_batch_vc))


def test_the_view_gives_each_front_the_rule_it_had():
    seen = {}
    for kind, is_bin, is_max, m, me, cols, pattern, allowed in itertools.product(
            (F64, RAT), (False, True), (False, True), (0, 1, 12, 52, 112, 400), (0, 2, 250), (2, 9, 25, 256, 300), (True, False), (True, False)):
        for extra in sorted({0, 1, cols - 1}):
            for name, fit, rule in FRONTS:
                want = rule(kind, pattern, extra, m, me, cols, is_bin, is_max, allowed)
                if want is None:                                   # the entry point's argument check refuses the call
                    continue
                got = _view(fit, kind, pattern, extra, m, me, cols, is_bin, is_max, allowed)
                assert got == (DEVICE if want else HOST), (name, kind, pattern, extra, m, me, cols, is_bin, is_max, allowed, got)
                if allowed and pattern:                            # the sides the SHAPE decides
                    seen.setdefault((name, got), 0)
                    seen[(name, got)] += 1
    for name, _, _ in FRONTS:
        assert seen.get((name, DEVICE), 0) > 0 and seen.get((name, HOST), 0) > 0, (name, seen)


@pytest.mark.parametrize("kind", [F64, RAT])
def test_the_one_difference_between_the_fit_modes(kind):
    """112 inequalities, 8 integer variables: the largest node LP has 120 rows. Maximising, the tableau alone is 120 x 130 x 8
    = 124 800 bytes; minimising (8 x 120) it all fits. mip_device_fits asks both directions, the launch the one asked for."""
    m, cols = 112, 9
    assert bg.small_lds_bytes(kind, 8, 120) <= LDS_WALK < 120 * 130 * 8 <= bg.small_lds_bytes(kind, 120, 8)
    from xpoly_amd._capi import lib
    assert lib().xpg_test_mip_fits(C.c_int(kind), C.c_int(m), C.c_int(0), C.c_int(cols), C.c_int(0), C.c_int(0)) == 0
    assert _view(FIT_LAUNCH, kind, 1, 0, m, 0, cols, False, False, 1) == DEVICE
    assert _view(FIT_LAUNCH, kind, 1, 0, m, 0, cols, False, True, 1) == HOST
    for is_max in (False, True):
        assert _view(FIT_BOTH, kind, 1, 0, m, 0, cols, False, is_max, 1) == HOST
        assert _view(FIT_LAUNCH, kind, 1, 0, m, 0, cols, False, is_max, 0) == HOST      # the switch wins


def test_the_switch_and_the_pattern_come_first_and_bad_arguments_are_refused():
    ok = dict(fit=FIT_BOTH, kind=RAT, pattern=1, extra=0, leq_rows=12, eq_rows=0, cols=9, is_bin=0, is_max=1, allowed=1)
    call = lambda **k: _view(**dict(ok, **k))
    assert call() == DEVICE and call(fit=FIT_LAUNCH) == DEVICE
    for fit in (FIT_LAUNCH, FIT_BOTH):
        assert call(fit=fit, allowed=0) == HOST and call(fit=fit, pattern=0) == HOST
    assert call(extra=8) == DEVICE and call(extra=9) == HOST           # more free variables than variables: no walk
    for bad in (dict(fit=2), dict(fit=-1), dict(kind=2), dict(cols=1), dict(leq_rows=-1), dict(eq_rows=-1), dict(extra=-1),
                dict(leq_rows=0, eq_rows=0)):
        assert call(**bad) == XPG_ERR_SHAPE, bad
