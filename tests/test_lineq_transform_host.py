"""CPU suite: the transformed-nest entry points (xpg_lineq_transform_levels_batch_*: T^-1, A * T^-1 and every level of the fme
loop in one launch of k_transform_levels_batch) as far as they can be checked without a device -- the symbols, the plan of a
call through the host-only view xpg_test_lineq_transform_plan against the restatement in tests/lineq_transform_cases.py (depth 1,
the floor of a level's slot and the place of the inverse's scratch included), the refusals of shape and mode, which are answered
before the handle is looked at, and the cases' own data on the CPU checker: no entry makes the reference's Rational approximate.
The answers are tests/test_gpu_lineq_transform.py's."""
import ctypes as C

import numpy as np

import lineq_levels_cases as lc
import lineq_transform_cases as tc
from lineq_transform_cases import XPG_ERR_SHAPE, XPG_ERR_UNSUPPORTED

NAMES = ("xpg_lineq_transform_levels_batch_packed_rat32", "xpg_lineq_transform_levels_batch_rat32_dev", "xpg_lineq_transform_last_route",
         "xpg_test_lineq_transform_plan")
SHAPES = [(4, 2, 1), (4, 3, 1), (4, 3, 2), (4, 4, 2), (6, 4, 3), (6, 5, 3), (8, 5, 4), (8, 6, 4)]      # the cases' (rows, cols, rhs)


def _lib():
    from xpoly_amd import build, _capi
    build.build()
    return _capi.lib()


def test_the_library_exports_the_transform_entry_points():
    import os
    lib = _lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "xpoly_amd.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name + "(" in hdr, name
    from xpoly_amd import _capi
    assert set(NAMES) <= set(_capi.SYMBOLS)
    from xpoly_amd.lineq import Lineq, transform_levels_dev
    assert callable(Lineq.transform_levels_packed) and callable(Lineq.transform_last_route) and callable(transform_levels_dev)


def test_plan_view_equals_the_restated_rule():
    _lib()
    places = set()
    shapes = SHAPES + [(1, 2, 1), (1, 6, 5), (2, 9, 8), (12, 7, 6), (40, 13, 12), (60, 20, 6), (3, 70, 65), (3, 70, 66)]
    for rows, cols, rhs in shapes:
        for cap in (0, rows, 37, 256, 1000):
            for cap_out in (0, rows - 1, rows, 64, 5000):
                for nb in (1, 65, 4096, 4396, 16384):
                    got, want = tc.plan_view(nb, rows, cols, rhs, cap, cap_out), tc.plan(nb, rows, cols, rhs, cap, cap_out)
                    assert got == want, (rows, cols, rhs, cap, cap_out, nb, got, want)
                    if not isinstance(got, dict):
                        continue
                    assert got["cap"] >= rows and rows <= got["cap_out"] <= got["cap"]
                    assert got["level_bytes"] == nb * rhs * got["cap_out"] * cols * 8            # rhs slots a system
                    places.add(got["inv_at"] == 0)
                    if rhs >= 2:                   # the walk is the levels': capacities, result area, seats; the LDS where aliased
                        p = lc.plan_view(nb, rows, cols, rhs - 1, cap, max(cap_out, 0))
                        assert all(got[k] == p[k] for k in ("grid", "groups", "cap_lds", "seat_bytes", "cap", "cap_out")), (got, p)
                        assert (got["sys_lds"] == p["sys_lds"]) == (got["inv_at"] == 0)
                    if got["inv_at"]:              # behind the walk's block, its bytes added
                        assert got["sys_lds"] == got["inv_at"] + tc.inv_bytes(rhs)
                        assert tc.inv_bytes(rhs) > (got["cap_lds"] + got["cap"]) * cols * 8
    assert places == {True, False}
    # the LDS statement: the cases' nests hold the inverse's scratch in the walk's two idle areas -- no byte is added
    for rows, cols, rhs in SHAPES:
        assert tc.plan_view(8, rows, cols, rhs)["inv_at"] == 0
    # a nest too small for it pays for it: 1 row, depth 5
    d = tc.plan_view(8, 1, 6, 5)
    assert d["inv_at"] > 0 and d["sys_lds"] == d["inv_at"] + tc.inv_bytes(5) == d["inv_at"] + 656
    # depth 1: no step, one slot a system
    d = tc.plan_view(8, 4, 2, 1)
    assert isinstance(d, dict) and d["level_bytes"] == 8 * 1 * d["cap_out"] * 2 * 8
    # a level's slot holds the nest
    assert tc.plan_view(8, 6, 4, 3, 0, 5) == XPG_ERR_SHAPE and tc.plan_view(8, 6, 4, 3, 0, 6)["cap_out"] == 6
    assert tc.plan_view(8, 40, 13, 5)["cap_out"] == 4 * 40 + 16 and tc.plan_view(8, 6, 4, 3)["cap_out"] == 6 * 6 // 4 + 6 + 1
    # refusals of the shape alone
    assert tc.plan_view(0, 4, 3, 2) == XPG_ERR_SHAPE and tc.plan_view(4, 0, 3, 2) == XPG_ERR_SHAPE and tc.plan_view(4, 4, 1, 1) == XPG_ERR_SHAPE
    assert tc.plan_view(4, 4, 3, 0) == XPG_ERR_SHAPE and tc.plan_view(4, 4, 3, 3) == XPG_ERR_SHAPE
    assert tc.plan_view(4, 3, 70, 66) == XPG_ERR_UNSUPPORTED and isinstance(tc.plan_view(4, 3, 70, 65), dict)
    assert tc.plan_view(4, 4, 3, 2, 32768) == XPG_ERR_UNSUPPORTED and tc.plan_view(4, 40, 13, 5, 1600) == XPG_ERR_UNSUPPORTED


def test_shape_and_mode_refusals_need_no_handle():
    """rhs_idx outside [1, cols) and a mode outside {0, 1} are answered before the handle is looked at; everything else the
    missing handle's XPG_ERR_SHAPE. No device is opened, nothing is launched."""
    lib = _lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    nests = tc.nest(3); t = np.stack([tc.tmats(3)["identity"]] * 2)
    off = np.zeros(2 * 3 + 1, dtype=np.int64)
    ok, steps, kind = (np.zeros(2, dtype=np.int32) for _ in range(3))
    det = np.zeros((2, 2), dtype=np.int32); mult = np.zeros((2, 3, 3, 2), dtype=np.int32)

    def packed(nb, cols, rhs, mode, tm=t):
        return lib.xpg_lineq_transform_levels_batch_packed_rat32(
            None, C.c_int(nb), vp(nests), C.c_int(1), vp(tm) if tm is not None else None, C.c_int(6), C.c_int(cols), C.c_int(rhs), C.c_int(mode),
            C.c_int(0), C.c_int(0), None, C.c_longlong(0), None, vp(off), vp(ok), vp(steps), vp(kind), vp(det), vp(mult))

    def dev(nb, cols, rhs, mode, tm=t):
        return lib.xpg_lineq_transform_levels_batch_rat32_dev(
            None, C.c_int(nb), None, C.c_int(1), None, C.c_int(6), C.c_int(cols), C.c_int(rhs), C.c_int(mode), C.c_int(8), C.c_int(8),
            None, None, None, None, None, None, None)

    for call in (packed, dev):
        for args in ((2, 4, 0, 0), (2, 4, 4, 0), (2, 4, 5, 0), (2, 1, 1, 0), (2, 4, 3, 2), (2, 4, 3, -1), (-1, 4, 3, 0), (2, 4, 3, 0), (2, 4, 3, 1)):
            assert call(*args) == XPG_ERR_SHAPE, args
    assert packed(2, 4, 3, 0, None) == XPG_ERR_SHAPE                                  # no transformations with nb > 0
    route = np.full(7, -1, dtype=np.int64)
    assert lib.xpg_lineq_transform_last_route(vp(route), C.c_int(7)) == 0 and route.tolist() == [0] * 7
    route[:] = -1
    assert lib.xpg_lineq_transform_last_route(vp(route), C.c_int(3)) == 0 and route.tolist() == [0, 0, 0, -1, -1, -1, -1]
    assert lib.xpg_lineq_transform_last_route(None, C.c_int(7)) == XPG_ERR_SHAPE
    assert lib.xpg_test_lineq_transform_plan(C.c_int(4), C.c_int(4), C.c_int(3), C.c_int(2), C.c_int(0), C.c_int(0), None, C.c_int(10)) == XPG_ERR_SHAPE


def test_the_cases_never_make_the_rational_approximate(port):
    """Every nest and transformation of the cases through the composed checker (the real reference too where its build is
    present): entries stay within |.| <= 3, appro_count() does not move, and what comes out passes the exact check. The cases
    that DO make it approximate live in tests/lineq_rescue_cases.py, held by tests/test_lineq_rescue_host.py and
    tests/test_gpu_lineq_rescue.py."""
    from oracle.checker import Ref
    for lib in [port] + ([Ref()] if Ref.available() else []):
        for n in (1, 2, 3, 4):
            for consts in (1, 2):
                a = tc.nest(n, consts)
                assert a.shape[0] in (4, 6, 8) and np.abs(a[..., 0]).max() <= 3
                for name, t in tc.tmats(n).items():
                    assert np.abs(t[..., 0]).max() <= 3
                    before = lib.appro_count()
                    w = tc.transformed(lib, a, t)
                    assert lib.appro_count() == before, (n, consts, name)
                    assert w[2] == {"singular": 1, "diag2": 2}.get(name, 2 if (name, n) == ("noncanonical", 1) else 0), (n, name, w[2])
                    if w[2] == 0:
                        assert w[0] == 1 and w[1] == n - 1 and w[5][0].shape[0] == a.shape[0]
                        tc.exact_check(a, t, w[4], w[5][0], 0)
    # the verdicts the GPU cases rely on, found here on the CPU
    dense3, dense4 = tc.tmats(3)["dense"], tc.tmats(4)["dense"]
    assert tc.transformed(port, tc.empty_nest(3, 1), tc.tmats(3)["identity"])[:2] == (0, 1)
    assert tc.transformed(port, tc.empty_nest(3, 1), dense3)[:2] == (0, 0)           # the transformation moves the step
    assert tc.transformed(port, tc.nest(3), dense3, cap_rows=8)[:2] == (-9, 1)        # step 1 builds 9 rows
    assert tc.transformed(port, tc.nest(4, 2), dense4, cap_out_rows=10)[:2] == (-11, 2)   # level 3 has 11 rows
