"""CPU suite: the projection entry points (a list of variables eliminated in one launch, xpg_lineq_project_batch_*) as far as
they can be checked without a device -- the symbols, the plan of a call through the host-only view xpg_test_lineq_project_plan
against the restatement in tests/lineq_project_cases.py, that the intermediates' slots follow the grid and not the batch, every
shape error of the elimination list (no handle needed), and the C++ collector, which must compile and link. The answers are
tests/test_gpu_lineq_project.py's."""
import ctypes as C
import os
import subprocess

import numpy as np

import lineq_project_cases as pc
from lineq_project_cases import XPG_ERR_SHAPE, XPG_ERR_UNSUPPORTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the projection's five entry points: two calls, the route view and the two host-only views (plan, list check)
NAMES = ("xpg_lineq_project_batch_packed_rat32", "xpg_lineq_project_batch_rat32_dev", "xpg_lineq_project_last_route",
         "xpg_test_lineq_project_plan", "xpg_test_lineq_project_check")


def _lib():
    from xpoly_amd import build, _capi
    build.build()
    return _capi.lib()


def build_collector():
    from xpoly_amd import build
    build.build()
    exe = os.path.join(ROOT, "tests", "cxx", "project_all")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "project_all.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "xpoly_amd"), "-lxpoly_amd", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "xpoly_amd")])
    return exe


def test_the_library_exports_the_projection_entry_points():
    lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "xpoly_amd.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name + "(" in hdr, name
    from xpoly_amd.lineq import Lineq, project_dev
    assert callable(Lineq.project_packed) and callable(project_dev)


def test_plan_view_equals_the_restated_rule():
    _lib()
    layouts = set()
    for rows, cols in ((1, 2), (4, 3), (6, 5), (9, 5), (12, 7), (16, 9), (40, 13), (60, 20)):
        for cap in (0, rows, 37, 256, 1000):
            for cap_out in (0, 8, 5000):
                for nb in (1, 48, 4096, 4097, 16384):
                    got, want = pc.plan_view(nb, rows, cols, cap, cap_out), pc.plan(nb, rows, cols, cap, cap_out)
                    assert got == want, (rows, cols, cap, cap_out, nb, got, want)
                    if isinstance(got, dict):
                        assert got["cap"] >= rows and 1 <= got["cap_out"] <= got["cap"] and got["cap_lds"] * cols >= got["cap"]
                        assert got["sys_lds"] * got["groups"] <= 160 * 1024
                        layouts.add(got["cap_lds"] == got["cap"])
    assert layouts == {True, False}             # the whole result in LDS, and the area that only holds the row factors
    # the defaults: fme's worst case for `rows`, and the final slots as large as the intermediates'
    d = pc.plan_view(8, 12, 7)
    assert d["cap"] == 12 * 12 // 4 + 12 + 1 and d["cap_out"] == d["cap"]
    assert pc.plan_view(8, 12, 7, 5, 0)["cap"] == 12                                 # never under the input's rows
    # refusals of the shape alone
    assert pc.plan_view(0, 4, 3) == XPG_ERR_SHAPE and pc.plan_view(4, 0, 3) == XPG_ERR_SHAPE and pc.plan_view(4, 4, 1) == XPG_ERR_SHAPE
    assert pc.plan_view(4, 4, 3, 32768) == XPG_ERR_UNSUPPORTED                       # cap > 32767
    assert pc.plan_view(4, 40, 13, 1600) == XPG_ERR_UNSUPPORTED                      # the layout of cap rows over 160 KB
    assert isinstance(pc.plan_view(4, 40, 13, 1200), dict)


def test_seat_slots_follow_the_grid_not_the_batch():
    _lib()
    for rows, cols, cap in ((6, 5, 256), (16, 9, 0), (40, 13, 400)):
        small = pc.plan_view(48, rows, cols, cap)
        assert small["seat_bytes"] == 48 * small["groups"] * 2 * small["cap"] * cols * 8
        full = [pc.plan_view(nb, rows, cols, cap) for nb in (4096, 4097, 16384, 1 << 20)]
        seats = full[0]["grid"] * full[0]["groups"]
        assert seats == 4096 * full[0]["groups"]
        for p in full:
            assert p["grid"] * p["groups"] == seats and p["seat_bytes"] == seats * 2 * p["cap"] * cols * 8, p
        # against the chained-launch form's three [nb][cap][cols] areas
        assert full[2]["seat_bytes"] < 3 * 16384 * full[2]["cap"] * cols * 8


def test_every_shape_error_is_returned_without_a_handle():
    """The rules of the elimination list -- n_elim <= 0, an index outside [0, rhs_idx), rhs_idx outside [1, cols), more than 64
    entries -- through the host-only view xpg_test_lineq_project_check (the function both calls ask first), and through the
    calls themselves without a handle: they answer the list before they look at the handle, so a list too long comes back as
    XPG_ERR_UNSUPPORTED and not as the XPG_ERR_SHAPE of the missing handle. No device is opened, nothing is launched."""
    lib = _lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    mats = np.zeros((2, 4, 5, 2), dtype=np.int32); mats[..., 1] = 1
    off = np.zeros(3, dtype=np.int64); ok = np.zeros(2, dtype=np.int32); steps = np.zeros(2, dtype=np.int32)

    def check(cols, rhs, elim):
        el = np.asarray(elim, dtype=np.int32)
        return lib.xpg_test_lineq_project_check(C.c_int(cols), C.c_int(rhs), vp(el) if el.size else None, C.c_int(el.size))

    def packed(rhs, elim):
        el = np.asarray(elim, dtype=np.int32)
        return lib.xpg_lineq_project_batch_packed_rat32(None, C.c_int(2), vp(mats), C.c_int(4), C.c_int(5), C.c_int(rhs), vp(el), C.c_int(el.size),
                                                        C.c_int(0), C.c_int(0), C.c_int(0), None, C.c_longlong(0), None, vp(off), vp(ok), vp(steps))

    def dev(rhs, elim):
        el = np.asarray(elim, dtype=np.int32)
        return lib.xpg_lineq_project_batch_rat32_dev(None, C.c_int(2), None, C.c_int(4), C.c_int(5), C.c_int(rhs), vp(el), C.c_int(el.size), C.c_int(0),
                                                     C.c_int(8), C.c_int(8), None, None, None, None)

    assert check(5, 4, [3, 2]) == 0 and check(5, 4, [3, 3, 0]) == 0                  # a repeated index is allowed
    assert check(5, 4, []) == XPG_ERR_SHAPE                                          # n_elim <= 0
    assert lib.xpg_test_lineq_project_check(C.c_int(5), C.c_int(4), None, C.c_int(2)) == XPG_ERR_SHAPE
    assert lib.xpg_test_lineq_project_check(C.c_int(5), C.c_int(4), vp(np.zeros(1, dtype=np.int32)), C.c_int(-1)) == XPG_ERR_SHAPE
    assert check(5, 4, [4]) == XPG_ERR_SHAPE and check(5, 4, [3, -1]) == XPG_ERR_SHAPE   # an index outside [0, rhs_idx)
    assert check(5, 0, [0]) == XPG_ERR_SHAPE and check(5, 5, [3]) == XPG_ERR_SHAPE   # rhs_idx outside [1, cols)
    assert check(1, 0, [0]) == XPG_ERR_SHAPE
    assert check(5, 4, [3] * pc.CHAIN_MAX) == 0 and check(5, 4, [3] * (pc.CHAIN_MAX + 1)) == XPG_ERR_UNSUPPORTED
    assert check(5, 4, [3] * pc.CHAIN_MAX + [4]) == XPG_ERR_SHAPE                    # a bad index wins over the length
    for call in (packed, dev):                                                       # no handle: the list is still answered first
        assert call(4, [3] * (pc.CHAIN_MAX + 1)) == XPG_ERR_UNSUPPORTED
        assert call(4, [4]) == XPG_ERR_SHAPE and call(5, [3]) == XPG_ERR_SHAPE and call(4, [3, 2]) == XPG_ERR_SHAPE
    route = np.full(6, -1, dtype=np.int64)
    assert lib.xpg_lineq_project_last_route(vp(route), C.c_int(6)) == 0 and route.tolist() == [0] * 6
    assert lib.xpg_lineq_project_last_route(None, C.c_int(6)) == XPG_ERR_SHAPE
    assert lib.xpg_test_lineq_project_plan(C.c_int(4), C.c_int(4), C.c_int(3), C.c_int(0), C.c_int(0), None, C.c_int(8)) == XPG_ERR_SHAPE


def test_the_collector_compiles_and_links():
    assert os.path.exists(build_collector())
