"""CPU suite: the plan of xpg_has_solution_batch_ragged_rat32 -- which systems of a call of mixed shapes the LDS-resident kernel
answers, which the device-memory kernel, which go per system, and what the two launches are sized for -- through the host-only
view xpg_test_has_solution_batch_ragged_plan (no device is opened) against a restatement built on has_solution_cases.plan, the
restated rule of the uniform call: a system takes the route a uniform call of its shape takes, and every launch size is the
largest of the uniform view's values over the launch's systems. Also the shape errors of the entry point, and the C++ collector,
which must compile and link. The answers of the call are tests/test_gpu_has_solution_ragged.py's."""
import ctypes as C
import os
import subprocess

import numpy as np

import free_var_cases as fc
import has_solution_cases as hs
import six_eq_cases as sc
import six_vc_hbm_cases as vc
from tools import gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XPG_ERR_SHAPE = -3
ROUTE_NO_SOLVE = 3
HBM_SHAPES = (vc.FIRST, vc.ODD) + vc.FOLD_SHAPES


def _vc(nv, nfree):
    return gen.to_rat(gen.vc_nonneg(nv, False, range(nfree)))


def restated(pattern, nfree, rows, cols, cus=256):
    """(route per system, the launches' sizes) from the uniform rule alone. rows: [(leq_rows, eq_rows)]. The grid: every rule
    in the uniform plan's grid is a minimum of terms that fall as a size grows, so the launch's is the smallest a system's own
    plan gives for the launch's count."""
    from xpoly_amd.six import HAS_SOLUTION_RAGGED_FIELDS
    route, on = [], {hs.ROUTE_LDS: [], hs.ROUTE_HBM: []}
    for m, me in rows:
        r = ROUTE_NO_SOLVE if m == 0 else hs.plan(pattern, nfree, m, me, cols, 1, cus)["route"]
        route.append(r)
        if r in on:
            on[r].append((m, me))
    sizes = dict.fromkeys(HAS_SOLUTION_RAGGED_FIELDS, 0)
    for r, name, fields in ((hs.ROUTE_LDS, "lds", ("lds", "threads", "slot")), (hs.ROUTE_HBM, "hbm", ("lds", "slot", "Rmax", "ld", "threads"))):
        if on[r]:
            plans = [hs.plan(pattern, nfree, m, me, cols, len(on[r]), cus) for m, me in on[r]]
            sizes[name + "_count"] = len(on[r])
            for f in fields:
                sizes["%s_%s" % (name, f)] = max(g[f] for g in plans)
            sizes[name + "_grid"] = min(g["grid"] for g in plans)
    return route, sizes


def _check(vc_arr, pattern, nfree, rows, cols, cus=256):
    from xpoly_amd.six import has_solution_batch_plan, has_solution_ragged_plan
    route, sizes = has_solution_ragged_plan(vc_arr, [m for m, _ in rows], [me for _, me in rows], cus)
    want_route, want = restated(pattern, nfree, rows, cols, cus)
    assert route.tolist() == want_route and sizes == want, (rows, cols, cus, route.tolist(), want_route, sizes, want)
    for (m, me), r in zip(rows, route.tolist()):                 # the contract, through the uniform VIEW as well
        if m > 0:
            assert r == has_solution_batch_plan(vc_arr, m, me, cols, 1, cus)["route"], (m, me, r)
    return route.tolist(), sizes


def _mix(shape):
    """Row counts around a shape, under its columns and free variables: itself twice, taller without equalities, one row,
    nothing but equalities, no rows at all."""
    m, me = shape[0], shape[1]
    return [(m, me), (m + 3, 0), (1, min(me, 1)), (0, me), (m, me), (0, 0), (max(m // 2, 1), me + 1)]


def test_view_equals_the_restated_rule():
    seen = set()
    for shape in tuple(s for s, _ in hs.LDS_CASES) + HBM_SHAPES:
        nv, nfree = shape[2], shape[3]
        rows = _mix(shape) + ([(5, 1), (2, 4097), (900, 2)] if shape in HBM_SHAPES else [])
        for cus in (64, 256):
            route, sizes = _check(_vc(nv, nfree), True, nfree, rows, nv + 1, cus)
            seen.update(route)
            for name in ("lds", "hbm"):
                if sizes[name + "_count"]:
                    assert 1 <= sizes[name + "_grid"] <= sizes[name + "_count"] and sizes[name + "_slot"] % 256 == 0
                    assert sizes[name + "_grid"] * sizes[name + "_slot"] <= vc.SCRATCH_MAX
    assert seen == {hs.ROUTE_LDS, hs.ROUTE_HBM, hs.ROUTE_OTHER, ROUTE_NO_SOLVE}
    # the four device-memory shapes in one call: one launch, sized by the largest of each
    rows = [(s[0], s[1]) for s in HBM_SHAPES]
    route, sizes = _check(_vc(62, 2), True, 2, rows * 2, 63)
    assert route == [hs.ROUTE_HBM] * 8 and sizes["hbm_count"] == 8 and sizes["lds_count"] == 0 and sizes["hbm_threads"] == vc.THREADS
    # a general vc: every system with an inequality goes per system, whatever its size
    for vc0 in fc.general_vcs(62):
        route, sizes = _check(gen.to_rat(vc0), False, 0, [(60, 4), (5, 2), (0, 1)], 63)
        assert route == [hs.ROUTE_OTHER, hs.ROUTE_OTHER, ROUTE_NO_SOLVE] and not any(sizes.values())
    # a launch's thread count is the largest of its systems' own
    route, sizes = _check(_vc(20, 1), True, 1, [(4, 1), (20, 2), (20, 12)], 21)
    assert [hs.plan(True, 1, m, me, 21, 1)["threads"] for m, me in ((4, 1), (20, 2), (20, 12))] == [64, 128, 256]
    assert route == [hs.ROUTE_LDS] * 3 and sizes["lds_threads"] == 256


def test_a_launch_is_sized_by_its_systems_not_by_their_envelope():
    """nv = 20, one free variable: (50, 0) and (10, 20) each need 33 712 bytes of LDS; the envelope shape (50, 20) needs
    88 800 and is not the LDS-resident kernel's at all."""
    route, sizes = _check(_vc(20, 1), True, 1, [(50, 0), (10, 20)], 21)
    assert route == [hs.ROUTE_LDS, hs.ROUTE_LDS] and sizes["lds_lds"] == 33712 and sizes["lds_count"] == 2 and sizes["hbm_count"] == 0
    assert hs.plan(True, 1, 50, 0, 21, 1)["lds"] == 33712 and hs.plan(True, 1, 10, 20, 21, 1)["lds"] == 33712
    envelope = hs.plan(True, 1, 50, 20, 21, 1)
    assert envelope["route"] != hs.ROUTE_LDS and max(sc.plan_bytes(50, 20, 20, 1, d, fc.RAT) for d in (True, False)) == 88800
    from xpoly_amd.six import has_solution_batch_plan
    assert has_solution_batch_plan(_vc(20, 1), 50, 20, 21, 1)["route"] != hs.ROUTE_LDS


def test_one_call_holds_both_routes():
    m, me, nv, nfree = vc.FIRST
    route, sizes = _check(_vc(nv, nfree), True, nfree, [(5, 1), (m, me), (5, 1), (m, me)], nv + 1)
    assert route == [hs.ROUTE_LDS, hs.ROUTE_HBM, hs.ROUTE_LDS, hs.ROUTE_HBM]
    assert sizes["lds_count"] == 2 and sizes["hbm_count"] == 2 and sizes["lds_grid"] == 2 and sizes["hbm_grid"] == 2
    assert sizes["hbm_lds"] + vc.LDS_STATIC <= vc.LDS_MAX and sizes["lds_lds"] <= vc.SIX_VC_LDS_MAX


def test_malformed_calls():
    """XPG_ERR_SHAPE before anything touches a device: the calls are made without a handle, so a call that got past the shape
    rule could not answer XPG_ERR_SHAPE for another reason than the one named -- each is paired with the same call made well
    but for the handle, which is refused for the handle alone."""
    from xpoly_amd._capi import lib, vp
    arr = _vc(4, 1)
    leq = gen.to_rat(np.ones((7, 5), dtype=np.int32))
    rows = np.array([4, 3], dtype=np.int32); none = np.zeros(2, dtype=np.int32); off = np.array([0, 20], dtype=np.int64)
    has = np.full(2, 55, dtype=np.int32)

    def call(ctx=None, nb=2, l=leq, lr=rows, lo=off, e=None, er=none, eo=None, vc_rows=4, cols=5, rhs=4):
        return lib().xpg_has_solution_batch_ragged_rat32(ctx, C.c_int(nb), vp(l), vp(lr), vp(lo), vp(e), vp(er), vp(eo), vp(arr), C.c_int(vc_rows),
                                                         C.c_int(cols), C.c_int(rhs), C.c_int(0), C.c_int(1), C.c_uint(10), vp(has), None)
    assert call() == XPG_ERR_SHAPE                                                  # no handle
    assert call(lr=None) == XPG_ERR_SHAPE and call(er=None) == XPG_ERR_SHAPE and call(lo=None) == XPG_ERR_SHAPE
    assert call(lr=np.array([4, -1], dtype=np.int32)) == XPG_ERR_SHAPE and call(er=np.array([0, -2], dtype=np.int32)) == XPG_ERR_SHAPE
    assert call(lo=np.array([0, -20], dtype=np.int64)) == XPG_ERR_SHAPE
    assert call(er=np.array([0, 1], dtype=np.int32)) == XPG_ERR_SHAPE               # an equality row without eq / eq_offsets
    assert call(rhs=3) == XPG_ERR_SHAPE and call(vc_rows=3) == XPG_ERR_SHAPE and call(l=None) == XPG_ERR_SHAPE
    assert (has == 55).all()
    route = (C.c_longlong * 7)(*([-99] * 7))
    assert lib().xpg_has_solution_batch_ragged_last_route(route, C.c_int(7)) == 0 and list(route) == [0] * 7
    assert lib().xpg_has_solution_batch_ragged_last_route(None, C.c_int(7)) == XPG_ERR_SHAPE
    # the view: no vc, vc_rows != cols - 1, no systems, NULL shape arrays, a negative row count, no compute units
    out = (C.c_longlong * 12)(*([-99] * 12)); rt = np.full(2, -9, dtype=np.int32)
    view = lambda vcp=vp(arr), vc_rows=4, cols=5, nb=2, lr=rows, er=none, cus=256, n=12: lib().xpg_test_has_solution_batch_ragged_plan(
        vcp, C.c_int(vc_rows), C.c_int(cols), C.c_int(nb), vp(lr), vp(er), C.c_int(cus), vp(rt), out, C.c_int(n))
    assert view(n=1) == 0 and list(out) == [2] + [-99] * 11 and rt.tolist() == [0, 0]
    assert view(vcp=None) == XPG_ERR_SHAPE and view(vc_rows=3) == XPG_ERR_SHAPE and view(nb=0) == XPG_ERR_SHAPE and view(cus=0) == XPG_ERR_SHAPE
    assert view(lr=None) == XPG_ERR_SHAPE and view(er=None) == XPG_ERR_SHAPE and view(lr=np.array([4, -1], dtype=np.int32)) == XPG_ERR_SHAPE


def test_the_collector_compiles_and_links():
    """tests/cxx/has_solution_ragged.cpp: xpoly_amd::has_solution_all -- one ragged call -- on a stub matrix type, under
    -Wall -Wextra -Werror. Run without its input it says how it is called; tests/test_gpu_has_solution_ragged.py runs it on
    four shape classes."""
    exe = build_collector()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr


def build_collector():
    from xpoly_amd import build
    build.build()
    exe = os.path.join(ROOT, "tests", "cxx", "has_solution_ragged")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "has_solution_ragged.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "xpoly_amd"), "-lxpoly_amd", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "xpoly_amd")])
    return exe
