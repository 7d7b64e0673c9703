"""CPU suite: the route rule of xpg_six_batch_hbm_* -- which shapes stay LDS-resident, which get a tableau slot in device
memory, which are refused -- and the sizes of the launch. Host-only view of the library (xpg_test_batch_hbm_geometry): no
device is opened. The LDS formula of the resident route is tests/batch_geometry.py's; the rest is restated in
tests/batch_hbm_cases.py."""
import ctypes as C

import pytest

import batch_geometry as bg
import batch_hbm_cases as hc

F64, RAT = hc.F64, hc.RAT
XPG_ERR_SHAPE = -3
FIELDS = ("route", "lds", "slot", "ld", "threads", "grid", "scratch")


def _view(kind, R, V, nb, cus=256):
    from xpoly_amd.six import BATCH_HBM_FIELDS, six_batch_hbm_geometry
    assert BATCH_HBM_FIELDS == FIELDS
    return six_batch_hbm_geometry(kind, R, V, nb, cus)


def _raw(kind, R, V, nb, cus, n=7):
    from xpoly_amd._capi import lib
    out = (C.c_longlong * 8)(*([-99] * 8))
    rc = lib().xpg_test_batch_hbm_geometry(C.c_int(kind), C.c_int(R), C.c_int(V), C.c_int(nb), C.c_int(cus), out, C.c_int(n))
    return rc, list(out)


SWEEP = [(R, V) for R in (1, 7, 31, 32, 64, 99, 100, 101, 137, 260, 400) for V in (1, 24, 48, 63, 100, 101, 300, 513)]


@pytest.mark.parametrize("kind", [F64, RAT])
def test_view_equals_the_restated_rule(kind):
    routes = set()
    for R, V in SWEEP:
        for nb in (1, 5, 1000, 100000):
            for cus in (1, 64, 256):
                got, want = _view(kind, R, V, nb, cus), hc.geometry(kind, R, V, nb, cus)
                assert got == want, (kind, R, V, nb, cus, got, want)
                routes.add(got["route"])
                if got["route"] == hc.ROUTE_LDS:
                    g = bg.geometry(kind, R, V, nb, cus)
                    assert (got["lds"], got["threads"], got["grid"]) == (g.lds, g.threads, g.grid) and not g.refused
                if got["route"] == hc.ROUTE_HBM:
                    assert got["ld"] % 2 == 0 and got["ld"] >= V + R + 2 and got["ld"] - (V + R + 2) <= 1
                    assert got["slot"] % 256 == 0 and got["slot"] >= R * got["ld"] * 8
                    assert 1 <= got["grid"] <= nb and got["scratch"] == got["grid"] * got["slot"] <= hc.SCRATCH_MAX
                    assert got["lds"] + bg.SMALL_LDS_STATIC <= hc.LDS_MAX
                    assert 256 <= got["threads"] <= 1024 and got["threads"] % 64 == 0
    assert routes == {hc.ROUTE_LDS, hc.ROUTE_HBM}


@pytest.mark.parametrize("is_max", [True, False])
@pytest.mark.parametrize("kind", [F64, RAT])
def test_the_lds_edge(kind, is_max):
    """Per family of shapes, the largest one xpg_six_batch_* accepts stays LDS-resident with that entry point's geometry, and
    the next one -- the first it refuses -- is the first to get a slot. The direction only swaps what the caller's arrays are
    called: the rule sees the shape as solved."""
    for name, fam in bg.LIMIT_FAMILIES.items():
        k = bg.largest_accepted(kind, fam)
        for kk, route in ((k, hc.ROUTE_LDS), (k + 1, hc.ROUTE_HBM)):
            R, V = fam(kk)
            m, cols = bg.caller_shape(is_max, R, V)
            assert bg.solved_as(is_max, m, cols) == (R, V)
            got = _view(kind, R, V, 4096)
            assert got["route"] == route, (name, kk, got)
            assert bg.lds_fits(kind, R, V) == (route == hc.ROUTE_LDS)
            assert got == hc.geometry(kind, R, V, 4096)
    # the issue's example: about 100 x 100 is the first refused fp64 square (176 448 bytes)
    if kind == F64:
        assert bg.small_lds_bytes(F64, 100, 100) == 176448 and _view(F64, 100, 100, 8)["route"] == hc.ROUTE_HBM


@pytest.mark.parametrize("kind", [F64, RAT])
def test_the_grid_is_cut_to_the_scratch_cap(kind):
    """400 x 400: 2.5 MB slots, so 104 of them fill the 256 MB whatever the device could seat (one workgroup per CU there:
    the side arrays take 122 KB of LDS)."""
    g = _view(kind, 400, 400, 5000, 256)
    assert g["route"] == hc.ROUTE_HBM and g["ld"] == 802 and g["slot"] == 400 * 802 * 8
    assert g["grid"] == hc.SCRATCH_MAX // g["slot"] == 104 and g["scratch"] <= hc.SCRATCH_MAX
    assert _view(kind, 400, 400, 5000, 64)["grid"] == 64
    assert _view(kind, 400, 400, 7, 256)["grid"] == 7
    # odd widest width: one padded column
    g = _view(kind, 101, 100, 3, 256)
    assert g["ld"] == 204 and g["slot"] == (101 * 204 * 8 + 255) // 256 * 256


@pytest.mark.parametrize("kind", [F64, RAT])
def test_refused_shapes(kind):
    """The pivot-pair table (one bit per pair of columns) outgrows LDS at about R + V = 960: refused, nothing to launch."""
    g = _view(kind, 600, 600, 16)
    assert g["route"] == hc.ROUTE_REFUSED and g["grid"] == 0 and g["scratch"] == 0
    assert g["lds"] == hc.side_bytes(kind, 600, 600) and g["lds"] + bg.SMALL_LDS_STATIC > hc.LDS_MAX
    # the last accepted and the first refused square
    k = 300
    while hc.side_bytes(kind, k + 1, k + 1) + bg.SMALL_LDS_STATIC <= hc.LDS_MAX:
        k += 1
    assert k == 479
    assert _view(kind, k, k, 16)["route"] == hc.ROUTE_HBM and _view(kind, k + 1, k + 1, 16)["route"] == hc.ROUTE_REFUSED


def test_empty_and_malformed_calls():
    for kind in (F64, RAT):
        assert _raw(kind, 100, 100, 0, 256)[0] == XPG_ERR_SHAPE          # the view describes a launch: nb = 0 has none
        assert _raw(kind, 0, 100, 4, 256)[0] == XPG_ERR_SHAPE
        assert _raw(kind, 100, 0, 4, 256)[0] == XPG_ERR_SHAPE
        assert _raw(kind, 100, 100, 4, 0)[0] == XPG_ERR_SHAPE
    assert _raw(2, 100, 100, 4, 256)[0] == XPG_ERR_SHAPE
    rc, out = _raw(F64, 100, 100, 4, 256, n=3)                            # fills min(n, 7) entries
    assert rc == 0 and out[:3] == [1, hc.side_bytes(F64, 100, 100), (100 * 202 * 8 + 255) // 256 * 256] and out[3:] == [-99] * 5
    # nb = 0 through the entry points themselves returns 0 before any device work: a null handle is the only shape error left
    from xpoly_amd._capi import lib
    route = (C.c_longlong * 3)()
    assert lib().xpg_six_batch_hbm_last_route(route, C.c_int(3)) == 0
    assert lib().xpg_six_batch_hbm_last_route(None, C.c_int(3)) == XPG_ERR_SHAPE
    for name in ("xpg_six_batch_hbm_f64", "xpg_six_batch_hbm_rat32"):
        assert getattr(lib(), name)(None, 1, 0, None, None, 100, 101, 10, None, None, None) == XPG_ERR_SHAPE
