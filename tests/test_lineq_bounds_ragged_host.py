"""CPU suite: the ragged calcBound entry point (xpg_lineq_bounds_batch_ragged_rat32: every chain of systems of mixed shapes in
one launch of k_calc_bound_ragged) as far as it can be checked without a device -- the symbols, the plan of a call through the
host-only view xpg_test_lineq_bounds_ragged_plan against the restatement in tests/lineq_bounds_ragged_cases.py and, where all
shapes agree, against xpg_test_lineq_bounds_plan figure for figure, every error code, the call without systems, and the C++
collector, which must compile and link. The answers are tests/test_gpu_lineq_bounds_ragged.py's."""
import ctypes as C
import os
import subprocess

import numpy as np

import lineq_bounds_cases as bc
import lineq_bounds_ragged_cases as rc_
from lineq_bounds_ragged_cases import XPG_ERR_SHAPE, XPG_ERR_UNSUPPORTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("xpg_lineq_bounds_batch_ragged_rat32", "xpg_lineq_bounds_ragged_last_route", "xpg_test_lineq_bounds_ragged_plan")


def _lib():
    from xpoly_amd import build, _capi
    build.build()
    return _capi.lib()


def build_collector():
    from xpoly_amd import build
    build.build()
    exe = os.path.join(ROOT, "tests", "cxx", "calc_bound_each")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "calc_bound_each.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "xpoly_amd"), "-lxpoly_amd", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "xpoly_amd")])
    return exe


def _shapes():
    rows = [r for r, _, n in rc_.CLASSES for _ in range(n)]
    cols = [nv + 1 for _, nv, n in rc_.CLASSES for _ in range(n)]
    return rows, cols


def test_the_library_exports_the_entry_points():
    lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "xpoly_amd.h")).read()
    from xpoly_amd._capi import SYMBOLS
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name + "(" in hdr and name in SYMBOLS, name
    from xpoly_amd.lineq import Lineq
    assert callable(Lineq.bounds_ragged) and callable(Lineq.bounds_ragged_last_route)


def test_plan_view_equals_the_restated_rule_for_mixed_batches():
    _lib()
    rows, cols = _shapes()
    assert len(rows) == 108
    for cap in (0, 5, 37, 256, 512, 1000):
        for cap_out in (0, 3, 8, 40, 5000):
            for reps in (1, 40):                                                     # 108 systems, and 4320: above the grid
                r, c = rows * reps, cols * reps
                got, want = rc_.plan_view(r, c, None, cap, cap_out), rc_.plan(r, c, None, cap, cap_out)
                assert got == want and isinstance(got, dict), (cap, cap_out, reps, got, want)
                assert (got["cols"], got["rows"]) == (6, 9) and got["cap"] >= 9 and 1 <= got["cap_out"] <= got["cap"]
                assert got["cap_lds"] * 6 >= got["cap"] and got["grid"] == min(len(r), 4096) and got["groups"] == 1
                assert got["seat_bytes"] == got["grid"] * 3 * got["cap"] * 6 * 8
                assert got["out_bytes"] == sum((cc - 1) * cc for cc in c) * got["cap_out"] * 8
                assert got["steps"] == sum((cc - 2) * (cc + 1) // 2 for cc in c)
    # the figures the GPU tests rely on
    assert rc_.plan_view(rows, cols, None, 512)["cap_lds"] == 86 and rc_.plan_view(rows, cols, None, 256)["cap_lds"] == 43
    d = rc_.plan_view(rows, cols)
    assert d["cap"] == 4 * 9 + 16 == d["cap_out"]                                    # the defaults follow the system with the most rows
    assert rc_.plan_view(rows, cols, None, 5)["cap"] == 9 and rc_.plan_view(rows, cols, None, 40, 41)["cap_out"] == 40
    # an explicit rhs_idx: the constant column inside the matrix; None is the last column of each
    rhs = [c - 2 if c > 2 else 1 for c in cols]
    assert rc_.plan_view(rows, cols, rhs, 512, 40) == rc_.plan(rows, cols, rhs, 512, 40)
    assert rc_.plan_view(rows, cols, [c - 1 for c in cols], 512, 40) == rc_.plan_view(rows, cols, None, 512, 40)


def test_a_batch_of_one_shape_gets_the_uniform_plan():
    _lib()
    shared = ("launches", "grid", "groups", "sys_lds", "cap_lds", "seat_bytes", "cap", "cap_out")
    for rows, cols, rhs in ((1, 2, 1), (4, 3, 2), (6, 5, 4), (9, 5, 4), (12, 7, 6), (16, 9, 5), (40, 13, 12), (60, 20, 19)):
        for cap in (0, rows, 37, 256, 512, 1000):
            for cap_out in (0, 8, 5000):
                for nb in (1, 48, 4097):
                    u = bc.plan_view(nb, rows, cols, rhs, cap, cap_out)
                    g = rc_.plan_view([rows] * nb, [cols] * nb, [rhs] * nb, cap, cap_out)
                    if not isinstance(u, dict):
                        assert g == u, (rows, cols, rhs, cap, cap_out, nb, g, u)
                        continue
                    assert all(g[k] == u[k] for k in shared), (rows, cols, rhs, cap, cap_out, nb, g, u)
                    assert g["steps"] == nb * u["steps"] and g["out_bytes"] == nb * rhs * g["cap_out"] * cols * 8
                    assert (g["cols"], g["rows"]) == (cols, rows)


def test_every_error_code():
    lib = _lib()
    pv = rc_.plan_view
    assert pv([], [], nb=0) == XPG_ERR_SHAPE and pv([4], [3], nb=-1) == XPG_ERR_SHAPE          # nb <= 0
    assert pv([4, 0], [3, 3]) == XPG_ERR_SHAPE and pv([4, -1], [3, 3]) == XPG_ERR_SHAPE        # rows <= 0
    assert pv([4, 4], [3, 1]) == XPG_ERR_SHAPE                                                 # cols <= 1
    assert pv([4, 4], [3, 3], [2, 0]) == XPG_ERR_SHAPE and pv([4, 4], [3, 3], [3, 2]) == XPG_ERR_SHAPE   # rhs outside [1, cols)
    assert isinstance(pv([4, 4], [3, 3], [1, 2]), dict) and isinstance(pv([4, 4], [3, 3]), dict)         # NULL rhs_idx: the last column
    assert pv([4, 4], [3, 3])["steps"] == 4 and pv([4, 4], [3, 3], [1, 2])["steps"] == 2
    assert pv([4, 4], [3, 3], None, 32768) == XPG_ERR_UNSUPPORTED                              # cap > 32767
    assert pv([4, 40000], [3, 3]) == XPG_ERR_UNSUPPORTED                                       # (rows alone put cap there)
    assert pv([4, 40], [3, 13], None, 1600) == XPG_ERR_UNSUPPORTED                             # the envelope's layout over 160 KB
    assert isinstance(pv([4, 40], [3, 13], None, 1200), dict)
    assert pv([40, 4], [3, 13], None, 1600) == XPG_ERR_UNSUPPORTED                             # (the envelope: widest cols, not the tall system's)
    assert isinstance(pv([40, 4], [3, 3], None, 1600), dict)
    # a shape error anywhere wins over a capacity refusal
    assert pv([4, 0], [3, 3], None, 32768) == XPG_ERR_SHAPE
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    assert lib.xpg_test_lineq_bounds_ragged_plan(C.c_int(1), vp(i32([4])), vp(i32([3])), None, C.c_int(0), C.c_int(0), None, C.c_int(12)) == XPG_ERR_SHAPE
    assert lib.xpg_test_lineq_bounds_ragged_plan(C.c_int(1), None, vp(i32([3])), None, C.c_int(0), C.c_int(0), vp(np.zeros(12, dtype=np.int64)),
                                                 C.c_int(12)) == XPG_ERR_SHAPE
    # the call itself without a handle, and with shapes it refuses: no device is opened, nothing is launched
    mats = np.zeros((2 * 4 * 5, 2), dtype=np.int32); mats[..., 1] = 1
    rows, cols, offs = i32([4, 4]), i32([5, 5]), np.array([0, 20], dtype=np.int64)
    ooff = np.zeros(9, dtype=np.int64); orows = np.zeros(8, dtype=np.int32)
    ok = np.zeros(2, dtype=np.int32); ch = np.zeros(2, dtype=np.int32); st = np.zeros(2, dtype=np.int32)

    def call(nb=2, rhs=None, cap=0, ooff_=ooff, rows_=rows):
        return lib.xpg_lineq_bounds_batch_ragged_rat32(None, C.c_int(nb), vp(mats), vp(rows_), vp(cols), vp(offs), vp(rhs), C.c_int(cap), C.c_int(0),
                                                       None, C.c_longlong(0), None, vp(ooff_), vp(orows), vp(ok), vp(ch), vp(st))

    assert call() == XPG_ERR_SHAPE                                                             # no handle
    assert call(rhs=i32([4, 0])) == XPG_ERR_SHAPE and call(rhs=i32([5, 4])) == XPG_ERR_SHAPE
    assert call(rows_=i32([4, 0])) == XPG_ERR_SHAPE and call(nb=-1) == XPG_ERR_SHAPE
    assert call(cap=32768) == XPG_ERR_UNSUPPORTED and call(cap=4000) == XPG_ERR_UNSUPPORTED    # decided before the handle is looked at
    assert call(ooff_=None) == XPG_ERR_SHAPE
    route = np.full(8, -1, dtype=np.int64)
    assert lib.xpg_lineq_bounds_ragged_last_route(vp(route), C.c_int(8)) == 0 and route.tolist() == [0] * 8
    assert lib.xpg_lineq_bounds_ragged_last_route(None, C.c_int(8)) == XPG_ERR_SHAPE
    # no systems: 0, the one offset written, nothing else looked at
    ooff[:] = 7
    assert lib.xpg_lineq_bounds_batch_ragged_rat32(None, C.c_int(0), None, None, None, None, None, C.c_int(0), C.c_int(0), None, C.c_longlong(0), None,
                                                   vp(ooff), None, None, None, None) == 0
    assert ooff[0] == 0 and ooff[1] == 7
    assert lib.xpg_lineq_bounds_ragged_last_route(vp(route), C.c_int(8)) == 0 and route.tolist() == [0] * 8


def test_the_collector_compiles_and_links():
    assert os.path.exists(build_collector())
