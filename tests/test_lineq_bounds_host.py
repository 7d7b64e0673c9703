"""CPU suite: the fused calcBound entry points (xpg_lineq_bounds_batch_*: every elimination chain of every system in one launch
of k_calc_bound_batch) as far as they can be checked without a device -- the symbols, the plan of a call through the host-only
view xpg_test_lineq_bounds_plan against the restatement in tests/lineq_bounds_cases.py, the three slots of a seat, the steps
figure, the shape errors that need no handle, and the C++ collector, which must compile and link. The answers are
tests/test_gpu_lineq_bounds.py's."""
import ctypes as C
import os
import subprocess

import numpy as np

import lineq_bounds_cases as bc
import lineq_project_cases as pc
from lineq_bounds_cases import XPG_ERR_SHAPE, XPG_ERR_UNSUPPORTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("xpg_lineq_bounds_batch_packed_rat32", "xpg_lineq_bounds_batch_rat32_dev", "xpg_lineq_bounds_last_route",
         "xpg_test_lineq_bounds_plan")


def _lib():
    from xpoly_amd import build, _capi
    build.build()
    return _capi.lib()


def build_collector():
    from xpoly_amd import build
    build.build()
    exe = os.path.join(ROOT, "tests", "cxx", "calc_bound_all")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "calc_bound_all.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "xpoly_amd"), "-lxpoly_amd", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "xpoly_amd")])
    return exe


def test_the_library_exports_the_bounds_entry_points():
    lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "xpoly_amd.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name + "(" in hdr, name
    from xpoly_amd.lineq import Lineq, bounds_dev
    assert callable(Lineq.bounds_packed) and callable(Lineq.bounds_last_route) and callable(bounds_dev)


def test_plan_view_equals_the_restated_rule():
    _lib()
    layouts = set()
    for rows, cols, rhs in ((1, 2, 1), (3, 2, 1), (4, 3, 2), (6, 5, 4), (9, 5, 4), (12, 7, 6), (16, 9, 5), (40, 13, 12), (60, 20, 19)):
        for cap in (0, rows, 37, 256, 512, 1000):
            for cap_out in (0, 8, 5000):
                for nb in (1, 48, 4096, 4097, 4396, 16384):
                    got, want = bc.plan_view(nb, rows, cols, rhs, cap, cap_out), bc.plan(nb, rows, cols, rhs, cap, cap_out)
                    assert got == want, (rows, cols, rhs, cap, cap_out, nb, got, want)
                    if isinstance(got, dict):
                        assert got["cap"] >= rows and 1 <= got["cap_out"] <= got["cap"] and got["cap_lds"] * cols >= got["cap"]
                        assert got["sys_lds"] * got["groups"] <= 160 * 1024 and got["grid"] * got["groups"] <= 4096
                        layouts.add(got["cap_lds"] == got["cap"])
    assert layouts == {True, False}             # the whole result in LDS, and the area that only holds the row factors
    # the defaults: the packed calcBound's 4 rows + 16, and the result slots as large as the intermediates'
    d = bc.plan_view(8, 12, 7, 6)
    assert d["cap"] == 4 * 12 + 16 and d["cap_out"] == d["cap"]
    assert bc.plan_view(8, 12, 7, 6, 5, 0)["cap"] == 12                              # never under the input's rows
    assert bc.plan_view(8, 12, 7, 6, 40, 41)["cap_out"] == 40                        # never above cap


def test_the_12_kb_boundary_of_the_lds_layout():
    """fme_lds keeps the whole result in LDS while result, input and scratch fit 12 KB: the last cap that does and the first
    that does not, at two widths, through the view."""
    _lib()
    for cols, rhs in ((5, 4), (9, 5)):
        fits = [cap for cap in range(8, 400) if pc.fme_lds(cap, cap, cols)[0] == cap]
        last = max(fits)
        assert fits == list(range(8, last + 1)) and pc.fme_lds(last, last, cols)[1] <= 12 * 1024
        a, b = bc.plan_view(48, 6, cols, rhs, last), bc.plan_view(48, 6, cols, rhs, last + 1)
        assert a == bc.plan(48, 6, cols, rhs, last) and b == bc.plan(48, 6, cols, rhs, last + 1)
        assert a["cap_lds"] == last and a["sys_lds"] <= 12 * 1024
        assert b["cap_lds"] == (last + 1 + cols - 1) // cols < last + 1


def test_refusals_of_the_shape_alone():
    lib = _lib()
    assert bc.plan_view(0, 4, 3, 2) == XPG_ERR_SHAPE and bc.plan_view(4, 0, 3, 2) == XPG_ERR_SHAPE and bc.plan_view(4, 4, 1, 1) == XPG_ERR_SHAPE
    assert bc.plan_view(4, 4, 3, 0) == XPG_ERR_SHAPE and bc.plan_view(4, 4, 3, 3) == XPG_ERR_SHAPE   # rhs_idx outside [1, cols)
    assert isinstance(bc.plan_view(4, 4, 3, 1), dict) and isinstance(bc.plan_view(4, 4, 3, 2), dict)
    assert bc.plan_view(4, 4, 3, 2, 32768) == XPG_ERR_UNSUPPORTED                    # cap > 32767
    assert bc.plan_view(4, 40, 13, 12, 1600) == XPG_ERR_UNSUPPORTED                  # the layout of cap rows over 160 KB
    assert isinstance(bc.plan_view(4, 40, 13, 12, 1200), dict)
    assert lib.xpg_test_lineq_bounds_plan(C.c_int(4), C.c_int(4), C.c_int(3), C.c_int(2), C.c_int(0), C.c_int(0), None, C.c_int(9)) == XPG_ERR_SHAPE
    # the calls themselves without a handle, and with a shape they refuse: no device is opened, nothing is launched
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    mats = np.zeros((2, 4, 5, 2), dtype=np.int32); mats[..., 1] = 1
    off = np.zeros(9, dtype=np.int64); ok = np.zeros(2, dtype=np.int32); ch = np.zeros(2, dtype=np.int32); st = np.zeros(2, dtype=np.int32)
    for rhs in (4, 0, 5):
        assert lib.xpg_lineq_bounds_batch_packed_rat32(None, C.c_int(2), vp(mats), C.c_int(4), C.c_int(5), C.c_int(rhs), C.c_int(0), C.c_int(0),
                                                       None, C.c_longlong(0), None, vp(off), vp(ok), vp(ch), vp(st)) == XPG_ERR_SHAPE
        assert lib.xpg_lineq_bounds_batch_rat32_dev(None, C.c_int(2), None, C.c_int(4), C.c_int(5), C.c_int(rhs), C.c_int(8), C.c_int(8),
                                                    None, None, None, None, None) == XPG_ERR_SHAPE
    route = np.full(7, -1, dtype=np.int64)
    assert lib.xpg_lineq_bounds_last_route(vp(route), C.c_int(7)) == 0 and route.tolist() == [0] * 7
    assert lib.xpg_lineq_bounds_last_route(None, C.c_int(7)) == XPG_ERR_SHAPE


def test_a_seat_has_three_slots_and_they_follow_the_grid():
    _lib()
    for rows, cols, rhs, cap in ((6, 5, 4, 256), (9, 5, 4, 512), (16, 9, 8, 0), (40, 13, 12, 400)):
        small = bc.plan_view(48, rows, cols, rhs, cap)
        assert small["seat_bytes"] == 48 * small["groups"] * 3 * small["cap"] * cols * 8
        # half as much again as the projection call's two slots per seat at the same capacity
        assert 2 * small["seat_bytes"] == 3 * pc.plan_view(48, rows, cols, small["cap"])["seat_bytes"]
        full = [bc.plan_view(nb, rows, cols, rhs, cap) for nb in (4096, 4097, 16384, 1 << 20)]
        seats = full[0]["grid"] * full[0]["groups"]
        assert seats == 4096 * full[0]["groups"]
        for p in full:
            assert p["grid"] * p["groups"] == seats and p["seat_bytes"] == seats * 3 * p["cap"] * cols * 8, p
        # against the chained-launch form's three [nb][cap][cols] areas and its [nb][rhs][cap][cols] results
        assert full[2]["seat_bytes"] < 3 * 16384 * full[2]["cap"] * cols * 8


def test_steps_per_system():
    """rhs - 1 prefix steps and rhs (rhs - 1) / 2 tail steps, (rhs - 1)(rhs + 2) / 2 in all, counted here chain by chain: chain
    j shares its first rhs - 1 - j steps with the walk of the prefixes and runs j of its own."""
    _lib()
    for rhs in range(1, 20):
        want = (rhs - 1) + sum(j for j in range(rhs))
        assert want == (rhs - 1) * (rhs + 2) // 2
        assert all(len(bc.chain_list(rhs, j)) == rhs - 1 for j in range(rhs))
        got = bc.plan_view(48, 4, rhs + 1, rhs)
        assert got["steps"] == want, (rhs, got)
        if rhs > 2:
            assert want < rhs * (rhs - 1)                                            # fewer than the chains run one by one
    assert bc.plan_view(48, 4, 2, 1)["steps"] == 0                                   # one variable: no step at all


def test_the_collector_compiles_and_links():
    assert os.path.exists(build_collector())
