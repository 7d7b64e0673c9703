"""CPU suite: which batches of LPs with equalities and free variables xpg_six_batch_vc_* reshapes and solves on the device,
and the sizes it decides by. Host-only view of the library (xpg_test_six_batch_vc_plan): no device is opened."""
import numpy as np
import pytest

import free_var_cases as fc
import six_eq_cases as sc
from tools import gen

F64, RAT = 0, 1
XPG_ERR_SHAPE = -3
LDS_MAX = 64 * 1024


_plan = sc.plan_view


@pytest.mark.parametrize("kind", [F64, RAT])
def test_sign_patterns_take_the_device_with_their_free_count_and_sizes(kind):
    for leq_rows, eq_rows, nv, nfree in sc.SHAPES + sc.EXTRA_SHAPES:
        vc = gen.vc_nonneg(nv, False, range(nfree))
        for is_max in (True, False):
            rc, out = _plan(vc, kind, leq_rows, eq_rows, is_max)
            assert rc == 0
            assert out == [1, nfree, leq_rows + 2 * eq_rows, nv + nfree, sc.plan_bytes(leq_rows, eq_rows, nv, nfree, is_max, kind)], \
                (leq_rows, eq_rows, nv, nfree, is_max, out)
    # 66 equalities (sc.WIDE_EQ): the largest normal form leaves the device maximising, fits it minimising (the dual)
    assert [_plan(gen.vc_nonneg(4, False, (0,)), kind, 3, 66, is_max)[1][0] for is_max in (True, False)] == [0, 1]
    # the free variables need not come first
    rc, out = _plan(gen.vc_nonneg(6, False, (1, 4)), kind, 3, 2, True)
    assert rc == 0 and out[:4] == [1, 2, 7, 8]


@pytest.mark.parametrize("kind", [F64, RAT])
def test_a_general_vc_takes_the_fallback(kind):
    for nv in (4, 5, 12):
        for vc in fc.general_vcs(nv):
            for is_max in (True, False):
                rc, out = _plan(vc, kind, 5, 2, is_max)
                assert rc == 0 and out[0] == 0, (nv, is_max, out)
                assert out[1] == 0 and out[2] == 9 and out[3] == nv       # no column of these vc is empty
    vc = gen.vc_nonneg(5, False, (2,)); vc[0, 2] = 1                      # a zero diagonal whose column is not empty: not free
    rc, out = _plan(vc, kind, 5, 2, True)
    assert rc == 0 and out[0] == 0 and out[1] == 0
    vc = gen.vc_nonneg(5, False, (2,)); vc[0, 0] = 3                      # general, and variable 2 is free all the same
    rc, out = _plan(vc, kind, 5, 2, True)
    assert rc == 0 and out[0] == 0 and out[1] == 1 and out[3] == 6


@pytest.mark.parametrize("kind", [F64, RAT])
def test_wrong_vc_rows_is_a_shape_error(kind):
    vc = gen.vc_nonneg(4, False)
    assert _plan(vc, kind, 4, 1, True, vc_rows=3)[0] == XPG_ERR_SHAPE
    assert _plan(vc, kind, 4, 1, True, vc_rows=5)[0] == XPG_ERR_SHAPE
    assert _plan(vc, kind, 0, 0, True)[0] == XPG_ERR_SHAPE               # neither inequalities nor equalities
    assert _plan(vc, kind, 4, 1, True)[0] == 0


largest_square = sc.largest_square


@pytest.mark.parametrize("is_max", [True, False])
@pytest.mark.parametrize("kind", [F64, RAT])
def test_the_64_kb_edge(kind, is_max):
    """Square shapes with one equality: the largest the view accepts and the next, which it refuses -- both sides of the edge
    agree with small_lds_bytes recomputed here. The same edge with two free variables lies lower."""
    for nfree in (0, 2):
        nv = largest_square(is_max, 1, nfree, kind)
        assert 40 <= nv <= 64, nv
        for n, want in ((nv, 1), (nv + 1, 0)):
            rc, out = _plan(gen.vc_nonneg(n, False, range(nfree)), kind, n, 1, is_max)
            b = sc.plan_bytes(n, 1, n, nfree, is_max, kind)
            assert rc == 0 and out == [want, nfree, n + 2, n + nfree, b], (n, out, b)
            assert (b <= LDS_MAX) == bool(want)
    assert largest_square(is_max, 1, 2, kind) < largest_square(is_max, 1, 0, kind)
