"""CPU suite: the route rule of xpg_mip_batch_vc_hbm_* -- which batches of MIP trees keep the LDS-resident walk, which walk
with their node tableaux in device memory, which go to the host controller -- and the sizes of the launch, through the
host-only view xpg_test_mip_hbm_plan (no device is opened); and the argument checks of the new entry points."""
import ctypes as C

import numpy as np
import pytest

import batch_geometry as bg
import batch_hbm_cases as hc
import free_var_cases as fc
from free_var_cases import F64, RAT
from tools import gen

XPG_ERR_SHAPE = -3
ROUTE_LDS, ROUTE_HBM, ROUTE_HOST = 0, 1, 2
MIP_EQ_MAX = 256                      # mip_kernels.hip.h
LDS_STATIC = 800                      # mip_tree_hbm.hip.h MIP_HBM_LDS_STATIC: the code object's group_segment_fixed_size
SCRATCH_MAX = 256 << 20
WIDE = dict(rows=50, cols=21, nfree=16)       # free_var_cases.wide_lp_f64


def _vc(kind, nv, nfree):
    return gen.vc_nonneg(nv, kind == F64, range(nfree))


def _plan(kind, vc, leq_rows, eq_rows, cols, is_bin, is_max, nb, cus=256):
    from xpoly_amd.six import mip_hbm_plan
    return mip_hbm_plan(kind, vc, leq_rows, eq_rows, cols, is_bin, is_max, nb, cus)


def _fits(kind, leq_rows, eq_rows, cols, is_bin, extra):
    from xpoly_amd._capi import lib
    return lib().xpg_test_mip_fits(C.c_int(kind), C.c_int(leq_rows), C.c_int(eq_rows), C.c_int(cols), C.c_int(int(is_bin)), C.c_int(extra))


def _rmax(leq_rows, eq_rows, n, is_bin):
    """mip_rmax (mip_host.hip.h): the rows of the largest node LP of the deepest path."""
    r = leq_rows + (0 if is_bin else n)
    if eq_rows > 0:
        r += 2 * (eq_rows + (n if is_bin else 0))
    return r


@pytest.mark.parametrize("kind", [F64, RAT])
@pytest.mark.parametrize("is_max", [True, False])
def test_a_tiny_shape_keeps_the_lds_walk(kind, is_max):
    m, nv, nfree = fc.SHAPES[0]
    assert (m, nv, nfree) == (3, 4, 1)
    rows = nv + nfree + m                                       # free_var_cases.free_var_mip
    g = _plan(kind, _vc(kind, nv, nfree), rows, 0, nv + 1, False, is_max, 64)
    rmax, n = _rmax(rows, 0, nv, False), nv + nfree
    assert _fits(kind, rows, 0, nv + 1, False, nfree) == 1
    assert g["route"] == ROUTE_LDS and g["free"] == nfree and g["slot"] == 0
    assert (g["R"], g["V"]) == ((rmax, n) if is_max else (n, rmax))
    assert g["lds"] == bg.small_lds_bytes(kind, g["R"], g["V"]) <= 64 * 1024
    assert 1 <= g["grid"] <= 64


@pytest.mark.parametrize("kind", [F64, RAT])
def test_the_wide_shape_walks_in_device_memory_in_both_directions(kind):
    rows, cols, nfree = WIDE["rows"], WIDE["cols"], WIDE["nfree"]
    vc = _vc(kind, cols - 1, nfree)
    assert _fits(F64, rows, 0, cols, False, 0) == 1 and _fits(F64, rows, 0, cols, False, nfree) == 0
    assert _fits(kind, rows, 0, cols, False, nfree) == 0
    for is_max, (R, V) in ((True, (70, 36)), (False, (36, 70))):
        g = _plan(kind, vc, rows, 0, cols, False, is_max, 16)
        assert g["route"] == ROUTE_HBM and g["free"] == nfree and (g["R"], g["V"]) == (R, V), g
        assert g["lds"] == hc.side_bytes(kind, R, V) and g["lds"] + LDS_STATIC <= bg.LDS_MAX
        assert g["ld"] % 2 == 0 and 0 <= g["ld"] - (R + V + 2) <= 1
        assert g["slot"] % 256 == 0 and 0 <= g["slot"] - R * g["ld"] * 8 < 256
        assert g["threads"] == 256 and g["grid"] == 16
        assert g["scratch"] == g["grid"] * (g["slot"] + g["ws_words"] * 8)
        assert _plan(kind, vc, rows, 0, cols, False, is_max, 1)["grid"] == 1
    # the dual alone would fit 64 KB: the LDS walk is still refused, as mip_device_fits asks both directions
    assert bg.small_lds_bytes(F64, 36, 70) <= 64 * 1024 < bg.small_lds_bytes(F64, 70, 36)
    # without the twins the same rows fit, and keep the LDS walk
    assert _plan(F64, _vc(F64, cols - 1, 0), rows, 0, cols, False, True, 16)["route"] == ROUTE_LDS


@pytest.mark.parametrize("kind", [F64, RAT])
def test_what_goes_to_the_host_controller(kind):
    rows, cols = WIDE["rows"], WIDE["cols"]
    for vc0 in fc.general_vcs(cols - 1):                        # a general vc, whatever the size
        arr = np.ascontiguousarray(vc0, dtype=np.float64) if kind == F64 else gen.to_rat(vc0)
        for r in (rows, 8):
            g = _plan(kind, arr, r, 0, cols, False, True, 16)
            assert g["route"] == ROUTE_HOST and g["grid"] == 0 and g["scratch"] == 0 and g["free"] == 0, g
    # the pivot-pair table outgrows LDS at about R + V = 960
    for is_max in (True, False):
        g = _plan(kind, _vc(kind, 200, 0), 1000, 0, 201, False, is_max, 16)
        assert g["R"] + g["V"] == 1400 and g["route"] == ROUTE_HOST and g["lds"] + LDS_STATIC > bg.LDS_MAX, g
    # the node's equality list: eq_rows + n + 2 <= 256
    nv = 60
    for eq_rows, route in ((MIP_EQ_MAX - nv - 2, ROUTE_HBM), (MIP_EQ_MAX - nv - 1, ROUTE_HOST)):
        g = _plan(kind, _vc(kind, nv, 0), 40, eq_rows, nv + 1, True, True, 16)
        assert g["route"] == route, (eq_rows, g)


def test_static_lds_is_counted_at_the_160_kb_edge():
    """Side arrays that fit 160 KB by themselves and not beside the kernel's 800 bytes are refused."""
    between, last_ok = [], None
    nv = 100
    for rows in range(700, 900):
        R, V = rows + nv, nv                                    # integer branching: one bound row per variable
        side = hc.side_bytes(F64, R, V)
        if side <= bg.LDS_MAX < side + LDS_STATIC:
            between.append(rows)
        elif side + LDS_STATIC <= bg.LDS_MAX:
            last_ok = rows
    assert between and last_ok
    for rows in between[:3]:
        assert _plan(F64, _vc(F64, nv, 0), rows, 0, nv + 1, False, True, 16)["route"] == ROUTE_HOST
    assert _plan(F64, _vc(F64, nv, 0), last_ok, 0, nv + 1, False, True, 16)["route"] == ROUTE_HBM


def test_the_grid_is_cut_by_lds_by_scratch_and_by_nb():
    rows, cols, nfree = WIDE["rows"], WIDE["cols"], WIDE["nfree"]
    vc = _vc(F64, cols - 1, nfree)
    g = _plan(F64, vc, rows, 0, cols, False, True, 5000, 256)
    assert g["grid"] == 4 * 256                                 # 16 wavefronts of 256 threads: 4 workgroups per CU
    assert _plan(F64, vc, rows, 0, cols, False, True, 5000, 64)["grid"] == 256
    assert _plan(F64, vc, rows, 0, cols, False, True, 7, 256)["grid"] == 7
    # 400 rows x 200 variables, integer branching: 600 x 802 cells = 3.8 MB slots and 2.3 MB workspaces
    g = _plan(F64, _vc(F64, 200, 0), 400, 0, 201, False, True, 5000, 256)
    each = g["slot"] + g["ws_words"] * 8
    assert g["route"] == ROUTE_HBM and g["slot"] % 256 == 0 and g["ld"] % 2 == 0
    assert g["grid"] == SCRATCH_MAX // each < 256 and g["grid"] <= 5000
    assert g["scratch"] == g["grid"] * each <= SCRATCH_MAX < (g["grid"] + 1) * each


def test_malformed_calls_and_the_raw_view():
    from xpoly_amd._capi import lib
    out = (C.c_longlong * 12)(*([-99] * 12))
    call = lambda kind, pat, m, me, cols, extra, nb, cus, n=11: lib().xpg_test_mip_hbm_plan(
        C.c_int(kind), C.c_int(pat), C.c_int(m), C.c_int(me), C.c_int(cols), C.c_int(0), C.c_int(1), C.c_int(extra), C.c_int(nb), C.c_int(cus),
        out, C.c_int(n))
    assert call(0, 1, 50, 0, 21, 16, 16, 256, n=4) == 0 and list(out)[:4] == [1, 16, 70, 36] and list(out)[4:] == [-99] * 8
    assert call(0, 1, 50, 0, 21, 16, 16, 256) == 0 and out[11] == -99
    assert call(0, 0, 50, 0, 21, 16, 16, 256) == 0 and out[0] == 2 and out[1] == 0
    assert call(0, 1, 0, 0, 21, 16, 16, 256) == XPG_ERR_SHAPE
    assert call(0, 1, 50, 0, 1, 0, 16, 256) == XPG_ERR_SHAPE
    assert call(0, 1, 50, 0, 21, 21, 16, 256) == XPG_ERR_SHAPE                     # more free variables than variables
    assert call(0, 1, 50, 0, 21, 16, 0, 256) == XPG_ERR_SHAPE                      # the view describes a launch: nb = 0 has none
    assert call(0, 1, 50, 0, 21, 16, 16, 0) == XPG_ERR_SHAPE
    assert call(2, 1, 50, 0, 21, 16, 16, 256) == XPG_ERR_SHAPE
    assert lib().xpg_test_mip_hbm_plan(0, 1, 50, 0, 21, 0, 1, 16, 16, 256, None, 11) == XPG_ERR_SHAPE
    route = (C.c_longlong * 5)()
    assert lib().xpg_mip_hbm_last_route(route, C.c_int(5)) == 0
    assert lib().xpg_mip_hbm_last_route(None, C.c_int(5)) == XPG_ERR_SHAPE
    # a NULL context or bad shapes: XPG_ERR_SHAPE, the outputs untouched
    st = np.full(4, 77, dtype=np.int32); v = np.full(4, 5.0); sol = np.full((4, 21), 6.0)
    tg, vc, leq = fc.wide_lp_f64(count=4)
    nodes = C.c_longlong(-5)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    f64 = lib().xpg_mip_batch_vc_hbm_f64
    assert f64(None, 4, 1, 0, p(tg), p(vc), None, 0, p(leq), 50, 21, None, p(st), p(v), p(sol), C.byref(nodes)) == XPG_ERR_SHAPE
    assert lib().xpg_mip_batch_vc_hbm_rat32(None, 4, 1, 0, p(tg), p(vc), None, 0, p(leq), 50, 21, None, p(st), p(v), p(sol), C.byref(nodes)) == XPG_ERR_SHAPE
    assert (st == 77).all() and (v == 5.0).all() and (sol == 6.0).all() and nodes.value == -5
