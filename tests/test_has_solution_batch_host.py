"""CPU suite: the route rule of xpg_has_solution_batch_* -- which batches the LDS-resident kernel answers, which the device-memory
kernel, which go per system -- through the host-only view xpg_test_has_solution_batch_plan (no device is opened) against the
restatement in tests/has_solution_cases.py; the shape errors of the entry points; and the C++ collector, which must compile and
link. The answers of the batch are tests/test_gpu_has_solution_batch.py's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import free_var_cases as fc
import has_solution_cases as hs
import six_eq_cases as sc
import six_vc_hbm_cases as vc
from tools import gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XPG_ERR_SHAPE, XPG_ERR_NO_DEVICE = -3, -5
HBM_SHAPES = (vc.FIRST, vc.ODD, vc.SPLIT, vc.TALL) + vc.FOLD_SHAPES
SHAPES = tuple(s for s, _ in hs.LDS_CASES) + HBM_SHAPES + ((64, 2, 64, 2), (100, 0, 100, 0), (600, 2, 500, 1), (2, 4097, 3, 0), (400, 2, 400, 0))


def _vc(nv, nfree):
    return gen.to_rat(gen.vc_nonneg(nv, False, range(nfree)))


def _view(vc_arr, leq_rows, eq_rows, cols, nb, cus=256):
    from xpoly_amd.six import HAS_SOLUTION_BATCH_FIELDS, has_solution_batch_plan
    assert HAS_SOLUTION_BATCH_FIELDS == hs.FIELDS
    return has_solution_batch_plan(vc_arr, leq_rows, eq_rows, cols, nb, cus)


def _view_shape(shape, nb, cus=256, dev=False):
    m, me, nv, nfree = shape
    return _view(None if dev else _vc(nv, nfree), m, me, nv + 1, nb, cus)


def test_view_equals_the_restated_rule():
    routes = set()
    for shape in SHAPES:
        for nb in (1, 64, 5000):
            for cus in (64, 256):
                for dev in (False, True):
                    got, want = _view_shape(shape, nb, cus, dev), hs.plan_of_shape(shape, nb, cus, dev)
                    assert got == want, (shape, nb, cus, dev, got, want)
                    routes.add(got["route"])
                    if got["route"] != hs.ROUTE_OTHER:
                        assert 1 <= got["grid"] <= nb and got["scratch"] == got["grid"] * got["slot"] <= vc.SCRATCH_MAX
                        assert got["slot"] % 256 == 0
    assert routes == {hs.ROUTE_LDS, hs.ROUTE_HBM, hs.ROUTE_OTHER}


def test_the_shapes_of_the_gpu_cases_take_the_routes_their_tests_assume():
    for shape, count in hs.LDS_CASES:
        g = _view_shape(shape, count)
        assert g["route"] == hs.ROUTE_LDS and g["grid"] == count and g["lds"] <= vc.SIX_VC_LDS_MAX, (shape, g)
        # sized for the larger direction
        m, me, nv, nfree = shape
        assert g["lds"] == max(sc.plan_bytes(m, me, nv, nfree, d, fc.RAT) for d in (True, False))
    assert _view_shape((20, 2, 20, 1), 32)["threads"] == 128 and _view_shape((30, 2, 30, 2), 16)["threads"] == 256
    assert _view_shape((5, 2, 5, 1), 128)["threads"] == 64
    for shape in (vc.FIRST, vc.ODD) + vc.FOLD_SHAPES:
        g = _view_shape(shape, hs.HBM_COUNT)
        assert g["route"] == hs.ROUTE_HBM and g["grid"] == hs.HBM_COUNT and g["threads"] == 256, (shape, g)
        assert g["lds"] + vc.LDS_STATIC <= vc.LDS_MAX


def test_split_takes_the_device_memory_kernel_as_a_whole():
    """(30, 3, 130, 2): maxm fits 64 KB, minm does not. One kernel answers both questions of a system, so the batch is the
    device-memory kernel's, with the tableau rows of the larger direction (minm's 132) and the larger side arrays."""
    m, me, nv, nfree = vc.SPLIT
    up, down = (vc.plan(fc.RAT, True, nfree, m, me, nv + 1, d, 64) for d in (True, False))
    assert up["route"] == vc.ROUTE_LDS and down["route"] == vc.ROUTE_HBM
    g = _view_shape(vc.SPLIT, 64)
    assert g["route"] == hs.ROUTE_HBM and g["Rmax"] == nv + nfree == 132 > m + 2 * me
    assert g["lds"] == max(hs.hc.side_bytes(fc.RAT, m + 2 * me, nv + nfree), hs.hc.side_bytes(fc.RAT, nv + nfree, m + 2 * me))
    assert g["slot"] > g["Rmax"] * g["ld"] * 8 and g["ld"] == down["ld"]


def test_what_the_rule_sends_to_the_host():
    # a general vc: per system whatever the size
    for vc0 in fc.general_vcs(62):
        for m, me in ((60, 4), (5, 2)):
            g = _view(vc0, m, me, 63, 64)
            assert g["route"] == hs.ROUTE_OTHER and g["grid"] == 0 and g["scratch"] == 0 and g["nfree"] == 0
            assert g == hs.plan(False, 0, m, me, 63, 64)
    for vc0 in fc.general_vcs(4):
        assert _view(vc0, 4, 1, 5, 64)["route"] == hs.ROUTE_OTHER
    # the pivot-pair table outgrows LDS at about R + V = 960; more equalities than the ballots' bit masks hold
    for shape in ((600, 2, 500, 1), (2, 4097, 3, 0)):
        assert _view_shape(shape, 16)["route"] == hs.ROUTE_OTHER
    # the _dev form sizes for every variable free: a shape that fits with its real vc may be refused there
    assert _view_shape((400, 2, 400, 0), 16)["route"] == hs.ROUTE_HBM and _view_shape((400, 2, 400, 0), 16, dev=True)["route"] == hs.ROUTE_OTHER


def test_malformed_calls():
    from xpoly_amd._capi import lib
    arr = _vc(4, 1)
    p = arr.ctypes.data_as(C.c_void_p)
    out = (C.c_longlong * 9)(*([-99] * 9))
    view = lambda vcp, vc_rows, m, me, cols, nb, cus, n=9: lib().xpg_test_has_solution_batch_plan(
        vcp, C.c_int(vc_rows), C.c_int(m), C.c_int(me), C.c_int(cols), C.c_int(nb), C.c_int(cus), out, C.c_int(n))
    assert view(p, 4, 4, 1, 5, 64, 256, n=2) == 0 and list(out)[:2] == [0, 1] and list(out)[2:] == [-99] * 7
    assert view(p, 3, 4, 1, 5, 64, 256) == XPG_ERR_SHAPE                            # vc_rows != cols - 1
    assert view(p, 4, 0, 1, 5, 64, 256) == XPG_ERR_SHAPE                            # the view describes a launch: without inequalities there is none
    assert view(p, 4, 4, 1, 5, 0, 256) == XPG_ERR_SHAPE and view(p, 4, 4, 1, 5, 64, 0) == XPG_ERR_SHAPE
    assert view(None, 0, 4, 1, 5, 64, 256) == 0 and out[1] == -1                    # the _dev form's view
    route = (C.c_longlong * 5)()
    assert lib().xpg_has_solution_batch_last_route(route, C.c_int(5)) == 0
    assert lib().xpg_has_solution_batch_last_route(None, C.c_int(5)) == XPG_ERR_SHAPE
    # has_solution()'s shape rule, checked before anything touches a device: no handle, rhs_idx != cols - 1, vc_rows != rhs_idx
    has = np.zeros(1, dtype=np.int32)
    hp = has.ctypes.data_as(C.c_void_p)
    for name in ("xpg_has_solution_batch_rat32", "xpg_has_solution_batch_rat32_dev"):
        fn = getattr(lib(), name)
        call = lambda ctx, vc_rows, cols, rhs: fn(ctx, C.c_int(1), p, C.c_int(4), None, C.c_int(0), p, C.c_int(vc_rows), C.c_int(cols),
                                                  C.c_int(rhs), C.c_int(0), C.c_int(1), C.c_uint(10), hp, None)
        assert call(None, 4, 5, 4) == XPG_ERR_SHAPE
    assert hs.NOT_RUN == 0x7FFFFFFF
    hdr = open(os.path.join(ROOT, "include", "xpoly_amd.h")).read()
    assert "enum { XPG_HS_NOT_RUN = 0x7FFFFFFF };" in hdr


def test_the_verdict_rule_of_the_restatement():
    """hs.verdict is linsys.cpp:864-876: a negative status ends the system, 0 decides, 1 decides unless a unique solution is
    demanded; (1, 2) is where is_unique_sol changes the verdict."""
    assert hs.verdict(0, None, True) == (1, hs.NOT_RUN) and hs.verdict(-7, None, False) == (-7, hs.NOT_RUN)
    assert hs.verdict(1, 2, False) == (1, hs.NOT_RUN) and hs.verdict(1, 2, True) == (0, 2)
    assert hs.verdict(2, 0, True) == (1, 0) and hs.verdict(2, 1, True) == (0, 1) and hs.verdict(2, 1, False) == (1, 1)
    assert hs.verdict(4, 0, True) == (1, 0) and hs.verdict(2, 4, False) == (0, 4) and hs.verdict(2, -7, False) == (-7, -7)


def test_the_feasibility_objective_reads_the_cells_as_given():
    leq = gen.to_rat(np.array([[0, 2, 0, 5], [0, 0, 0, 1]], dtype=np.int32))
    eq = gen.to_rat(np.array([[0, 0, -1, 3]], dtype=np.int32))
    assert hs.feasibility_objective(leq, None)[:, 0].tolist() == [0, 1, 0, 0]
    assert hs.feasibility_objective(leq, eq)[:, 0].tolist() == [0, 1, 1, 0]


def test_the_collector_compiles_and_links():
    """tests/cxx/has_solution_all.cpp: xpoly_amd::has_solution_all on a stub matrix type. Run without its input it says how it
    is called; tests/test_gpu_has_solution_batch.py runs it on two shape groups."""
    exe = build_collector()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr


def build_collector():
    from xpoly_amd import build
    build.build()
    exe = os.path.join(ROOT, "tests", "cxx", "has_solution_all")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "has_solution_all.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "xpoly_amd"), "-lxpoly_amd", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "xpoly_amd")])
    return exe
