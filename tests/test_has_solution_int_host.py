"""CPU suite: the route rule of xpg_has_solution_int_batch_* -- which batches run the LDS-resident tree walk twice, which the
device-memory kernel answers in one launch, which keep has_solution_batch's host composition -- through the host-only view
xpg_test_has_solution_int_plan (no device is opened) against the restatement in tests/has_solution_int_cases.py; the shape errors
of the entry points; and the C++ collector, which must compile and link. The answers are tests/test_gpu_has_solution_int.py's."""
import ctypes as C
import os
import subprocess

import numpy as np

import batch_geometry as bg
import batch_hbm_cases as hc
import free_var_cases as fc
import has_solution_int_cases as hi
from free_var_cases import RAT
from tools import gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XPG_ERR_SHAPE = -3


def _view(vc_arr, leq_rows, eq_rows, cols, nb, cus=256):
    from xpoly_amd.six import has_solution_int_plan
    return has_solution_int_plan(vc_arr, leq_rows, eq_rows, cols, nb, cus)


def _view_shape(shape, nb, cus=256):
    m, me, nv, nfree = shape
    return _view(hi.vc_of(nv, nfree), m, me, nv + 1, nb, cus)


def _mip_plan(shape, is_max, nb, cus=256):
    from xpoly_amd.six import mip_hbm_plan
    m, me, nv, nfree = shape
    return mip_hbm_plan(RAT, hi.vc_of(nv, nfree), m, me, nv + 1, False, is_max, nb, cus)


def test_view_equals_the_restated_rule():
    routes = set()
    shapes = hi.LDS_SHAPES + (hi.NEGATIVE_SHAPE, hi.WIDE_SHAPE, hi.WIDE_EQ_SHAPE, (20, 2, 20, 1), (100, 0, 100, 0), (1000, 0, 200, 0), (400, 0, 200, 0))
    for shape in shapes:
        m, me, nv, nfree = shape
        for nb in (1, 64, 5000):
            for cus in (64, 256):
                got, want = _view_shape(shape, nb, cus), hi.plan(hi.vc_of(nv, nfree), m, me, nv + 1, nb, cus)
                assert got == want, (shape, nb, cus, got, want)
                routes.add(got["route"])
    assert routes == {hi.ROUTE_LDS, hi.ROUTE_HBM, hi.ROUTE_HOST}


def test_small_shapes_run_the_lds_walk_twice():
    for shape in hi.LDS_SHAPES + (hi.NEGATIVE_SHAPE,):
        m, me, nv, nfree = shape
        g = _view_shape(shape, 64)
        up, down = _mip_plan(shape, True, 64), _mip_plan(shape, False, 64)
        assert g["route"] == hi.ROUTE_LDS and g["free"] == nfree and g["slot"] == 0 and g["obj_word"] == 0, (shape, g)
        # geometry per pass: each direction's own, as mip_geom gives it
        assert (g["lds_max"], g["threads_max"], g["grid_max"]) == (up["lds"], up["threads"], up["grid"]) and g["grid_max"] == 64
        assert (g["lds_min"], g["threads_min"], g["grid_min"]) == (down["lds"], down["threads"], down["grid"]) and g["grid_min"] == 64
        assert g["lds_max"] == bg.small_lds_bytes(RAT, g["rmax"], nv + nfree) <= 64 * 1024
        assert g["lds_min"] == bg.small_lds_bytes(RAT, nv + nfree, g["rmax"]) <= 64 * 1024
        # helper workgroups by mip_batch_device's rule: none behind root equalities, one per CU where the chip is under-filled
        assert g["help_max"] == g["help_min"] == (0 if me else 256)
        assert g["ws_words"] == up["ws_words"] and g["scratch"] == (64 + g["help_max"]) * g["ws_words"] * 8
    g = _view(hi.vc_of(4, 0), 4, 0, 5, 64)
    assert g["route"] == hi.ROUTE_LDS and g["help_max"] == g["help_min"] == 256 and g["scratch"] == (64 + 256) * g["ws_words"] * 8
    assert _view(hi.vc_of(4, 0), 4, 0, 5, 5000)["help_max"] == 0                   # more trees than walkers: no helpers


def test_the_wide_shape_takes_the_device_memory_kernel_sized_for_the_larger_direction():
    for shape in (hi.WIDE_SHAPE, hi.WIDE_EQ_SHAPE):
        m, me, nv, nfree = shape
        up, down = _mip_plan(shape, True, 16), _mip_plan(shape, False, 16)
        assert up["route"] == hi.ROUTE_HBM and down["route"] == hi.ROUTE_HBM
        g = _view_shape(shape, 16)
        assert g["route"] == hi.ROUTE_HBM and g["free"] == nfree and g["rmax"] == up["R"] == down["V"], g
        assert g["lds_max"] == g["lds_min"] == max(up["lds"], down["lds"])
        assert g["lds_max"] == max(hc.side_bytes(RAT, up["R"], up["V"]), hc.side_bytes(RAT, down["R"], down["V"]))
        assert up["lds"] != down["lds"] and g["lds_max"] + hi.LDS_STATIC <= hi.LDS_MAX
        assert g["slot"] == max(up["slot"], down["slot"]) and up["slot"] != down["slot"] and g["slot"] % 256 == 0
        assert (g["ld_max"], g["ld_min"]) == (up["ld"], down["ld"])
        assert g["slot"] >= up["R"] * g["ld_max"] * 8 and g["slot"] >= down["R"] * g["ld_min"] * 8
        # the workspace: mip_ws_words unchanged, the objective behind it
        assert g["obj_word"] == up["ws_words"] == down["ws_words"] and g["ws_words"] == g["obj_word"] + ((nv + 1 + 1) & ~1)
        assert g["threads_max"] == g["threads_min"] == 256 and g["grid_max"] == g["grid_min"] == 16 and g["help_max"] == g["help_min"] == 0
        assert g["scratch"] == 16 * (g["slot"] + g["ws_words"] * 8)


def test_the_grid_is_cut_by_nb_by_the_chip_and_by_scratch():
    assert _view_shape(hi.WIDE_SHAPE, 7)["grid_max"] == 7
    assert _view_shape(hi.WIDE_SHAPE, 5000, 256)["grid_max"] == 4 * 256            # 16 wavefronts of 256 threads: 4 workgroups per CU
    assert _view_shape(hi.WIDE_SHAPE, 5000, 64)["grid_max"] == 256
    g = _view_shape((400, 0, 200, 0), 5000)                                         # 600 x 802 cells: slots of 3.8 MB
    each = g["slot"] + g["ws_words"] * 8
    assert g["route"] == hi.ROUTE_HBM and g["grid_max"] == hi.SCRATCH_MAX // each < 256
    assert g["scratch"] == g["grid_max"] * each <= hi.SCRATCH_MAX < (g["grid_max"] + 1) * each
    # the LDS walk: each pass's grid by mip_geom, cut by nb
    g = _view_shape((5, 2, 5, 1), 100000)
    assert g["route"] == hi.ROUTE_LDS and g["grid_max"] < 100000 and g["grid_min"] < 100000 and g["threads_max"] == g["threads_min"] == 64
    assert _view_shape((5, 2, 5, 1), 3)["grid_max"] == _view_shape((5, 2, 5, 1), 3)["grid_min"] == 3


def test_what_the_rule_sends_to_the_host():
    for vc0 in fc.general_vcs(20):                              # a general vc, whatever the size
        for m in (50, 5):
            g = _view(gen.to_rat(vc0), m, 0, 21, 64)
            assert g["route"] == hi.ROUTE_HOST and g["grid_max"] == g["grid_min"] == 0 and g["scratch"] == 0 and g["free"] == 0, g
            assert g == hi.plan(gen.to_rat(vc0), m, 0, 21, 64)
    for vc0 in fc.general_vcs(4):
        assert _view(gen.to_rat(vc0), 4, 1, 5, 64)["route"] == hi.ROUTE_HOST
    # the pivot-pair table outgrows LDS at about R + V = 960
    g = _view_shape((1000, 0, 200, 0), 16)
    assert g["route"] == hi.ROUTE_HOST and g["grid_max"] == 0 and g["lds_max"] + hi.LDS_STATIC > hi.LDS_MAX
    # the node's equality list: eq_rows + n + 2 <= 256
    assert _view_shape((40, 256 - 60 - 2, 60, 0), 16)["route"] == hi.ROUTE_HBM and _view_shape((40, 256 - 60 - 1, 60, 0), 16)["route"] == hi.ROUTE_HOST


def test_malformed_calls_touch_nothing():
    from xpoly_amd._capi import lib
    from xpoly_amd.six import HAS_SOLUTION_INT_FIELDS, HAS_SOLUTION_INT_ROUTE_FIELDS
    arr = hi.vc_of(4, 1)
    p = arr.ctypes.data_as(C.c_void_p)
    nf = len(HAS_SOLUTION_INT_FIELDS)
    assert nf == 17 and len(HAS_SOLUTION_INT_ROUTE_FIELDS) == 6
    out = (C.c_longlong * nf)(*([-99] * nf))
    view = lambda vcp, vc_rows, m, me, cols, nb, cus, n=nf: lib().xpg_test_has_solution_int_plan(
        vcp, C.c_int(vc_rows), C.c_int(m), C.c_int(me), C.c_int(cols), C.c_int(nb), C.c_int(cus), out, C.c_int(n))
    assert view(p, 4, 4, 1, 5, 64, 256, n=2) == 0 and list(out)[:2] == [0, 1] and list(out)[2:] == [-99] * (nf - 2)
    assert view(p, 3, 4, 1, 5, 64, 256) == XPG_ERR_SHAPE                            # vc_rows != cols - 1
    assert view(None, 4, 4, 1, 5, 64, 256) == XPG_ERR_SHAPE                         # no _dev form: the view needs vc
    assert view(p, 4, 0, 1, 5, 64, 256) == XPG_ERR_SHAPE                            # the view describes a launch: without inequalities there is none
    assert view(p, 4, 4, 1, 5, 0, 256) == XPG_ERR_SHAPE and view(p, 4, 4, 1, 5, 64, 0) == XPG_ERR_SHAPE
    assert list(out)[2:] == [-99] * (nf - 2)
    route = (C.c_longlong * 6)()
    assert lib().xpg_has_solution_int_batch_last_route(route, C.c_int(6)) == 0
    assert lib().xpg_has_solution_int_batch_last_route(None, C.c_int(6)) == XPG_ERR_SHAPE
    # no handle: XPG_ERR_SHAPE before anything else (the other shape rules need a handle: tests/test_gpu_has_solution_int.py)
    has = np.full(2, 55, dtype=np.int32); st = np.full((2, 2), 55, dtype=np.int32)
    hp, sp = has.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p)
    leq = gen.to_rat(np.ones((2, 4, 5), dtype=np.int32))
    lp = leq.ctypes.data_as(C.c_void_p)
    assert lib().xpg_has_solution_int_batch_rat32(None, C.c_int(2), lp, C.c_int(4), None, C.c_int(0), p, C.c_int(4), C.c_int(5), C.c_int(4),
                                                  C.c_int(1), hp, sp) == XPG_ERR_SHAPE
    rows = np.array([4, 4], dtype=np.int32); erows = np.zeros(2, dtype=np.int32); off = np.array([0, 20], dtype=np.int64)
    rp, ep, op = (a.ctypes.data_as(C.c_void_p) for a in (rows, erows, off))
    assert lib().xpg_has_solution_int_batch_ragged_rat32(None, C.c_int(2), lp, rp, op, None, ep, None, p, C.c_int(4), C.c_int(5), C.c_int(4),
                                                         C.c_int(1), hp, sp) == XPG_ERR_SHAPE
    assert (has == 55).all() and (st == 55).all()
    hdr = open(os.path.join(ROOT, "include", "xpoly_amd.h")).read()
    assert "There is no _dev form: the walk sizes its workspace by the number of free variables" in hdr


def test_the_fixtures_are_what_their_names_say():
    """Cells only, no checker: the classes of WIDE_HS and the equalities of WIDE_HS_EQ."""
    _, eq0, leq = hi.wide_hs()
    a = leq[..., 0]
    assert eq0 is None and a.shape == (16, 50, 21) and (leq[..., 1] == 1).all()
    assert a[1, 49].tolist() == [1] + [0] * 19 + [-5] and a[2, 1].tolist() == [0] * 20 + [1] and (a[2, 36:, 1] == 0).all()
    assert a[3, 48, 2] == 2 and a[3, 48, 20] == 1 and a[3, 49, 2] == -2 and a[3, 49, 20] == -1 and np.count_nonzero(a[3, 48:]) == 4
    _, eq, leq2 = hi.wide_hs_eq()
    e, b = eq[..., 0], leq2[..., 0]
    assert e.shape == (16, 2, 21) and e[0, 0, 18:].tolist() == [1, 1, 2] and e[0, 1, 18:].tolist() == [1, -1, 0] and e[8, 1, 18:].tolist() == [1, -1, 1]
    assert np.count_nonzero(e[:, :, :18]) == 0
    # the inequalities that mention x18 or x19 have row indices inside the equalities' rows (lpsol.h:1232)
    for j in (18, 19):
        assert all(set(np.flatnonzero(b[s, :, j])) <= {0, 1} for s in range(16))
    assert np.array_equal(b[0, 2:18], a[0, 2:18]) and np.array_equal(b[0, 0, :18], a[0, 18, :18])


def test_the_collector_compiles_and_links():
    """tests/cxx/has_solution_int_all.cpp: xpoly_amd::has_solution_all(is_int_sol = true) on a stub matrix type. Run without its
    input it says how it is called; tests/test_gpu_has_solution_int.py runs it on two shape classes."""
    exe = build_collector()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr


def build_collector():
    from xpoly_amd import build
    build.build()
    exe = os.path.join(ROOT, "tests", "cxx", "has_solution_int_all")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "has_solution_int_all.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "xpoly_amd"), "-lxpoly_amd", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "xpoly_amd")])
    return exe
