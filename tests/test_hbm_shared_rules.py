"""The three routes that solve on a tableau in device memory -- xpg_six_batch_hbm_*, xpg_six_batch_vc_hbm_*,
xpg_mip_batch_vc_hbm_* -- take ld, the tableau slot, the side arrays and the grid from one statement in csrc/batch_hbm.hip.h
(hbm_ld, hbm_slot_bytes, hbm_side_bytes, hbm_grid). Their host-only views must agree wherever they share a rule. No device."""
import pytest

import batch_geometry as bg
from batch_hbm_cases import F64, RAT
from tools import gen

ROUTE_HBM = 1
LDS_MAX, SCRATCH_MAX = 160 * 1024, 256 << 20
STATIC = {"batch": 272, "vc": 272, "mip": 800}      # SMALL_LDS_STATIC, SIX_VC_HBM_LDS_STATIC, MIP_HBM_LDS_STATIC
# (rows, variables, free variables) of a caller's problem under maxm and the (R, V) it is solved as, maxm / minm
FIRST = (55, 55, 45, (110, 100))          # past one CU's 160 KB as a plain batch too, in both directions
LDS_CUT = (100, 200, 0, (300, 200))       # side arrays past 40 KB: fewer than 4 workgroups per CU
SCRATCH_CUT = (400, 200, 0, (600, 200))   # 3.8 MB slots: fewer than 256 of them under the cap


def _plans(kind, case, is_max, nb, cus):
    """{route name: (plan, bytes of one workgroup in scratch)} for one problem shape, every plan solving the same (R, V)."""
    from xpoly_amd.six import mip_hbm_plan, six_batch_hbm_geometry, six_batch_vc_hbm_plan
    rows, nv, nfree, (R, V) = case
    if not is_max:
        R, V = V, R
    vc = gen.vc_nonneg(nv, kind == F64, range(nfree))
    batch = six_batch_hbm_geometry(kind, R, V, nb, cus)
    # integer branching adds one bound row per variable: rows + nv of them, as the vc batch is given outright
    mip = mip_hbm_plan(kind, vc, rows, 0, nv + 1, False, is_max, nb, cus)
    six = six_batch_vc_hbm_plan(kind, vc, rows + nv, 0, nv + 1, is_max, nb, cus)
    assert (mip["R"], mip["V"]) == (six["Rmax"], six["Vmax"]) == (R, V)
    for g in (batch, mip, six):
        assert g["route"] == ROUTE_HBM, g
    return {"batch": (batch, batch["slot"]), "vc": (six, six["slot"]), "mip": (mip, mip["slot"] + mip["ws_words"] * 8)}


def _grid(cus, lds, each, nb):
    per_cu = max(1, min(16 * 64 // 256, LDS_MAX // lds))
    return max(1, min(cus * per_cu, SCRATCH_MAX // each, nb))


@pytest.mark.parametrize("kind", [F64, RAT])
@pytest.mark.parametrize("is_max", [True, False])
def test_ld_slot_and_side_arrays_agree(kind, is_max):
    for case in (FIRST, LDS_CUT, SCRATCH_CUT):
        p = _plans(kind, case, is_max, 16, 256)
        batch, mip, six = p["batch"][0], p["mip"][0], p["vc"][0]
        assert batch["ld"] == mip["ld"] == six["ld"]
        assert batch["lds"] == mip["lds"] == six["lds"]
        assert batch["slot"] == mip["slot"]
        # the vc batch keeps its reshaping in front of the tableau in the same slot
        assert six["slot"] % 256 == 0 and six["slot"] > batch["slot"] - 256


@pytest.mark.parametrize("kind", [F64, RAT])
def test_one_grid_rule_describes_all_three(kind):
    seen = set()
    for case in (FIRST, LDS_CUT, SCRATCH_CUT):
        for is_max in (True, False):
            for nb, cus in ((5000, 256), (7, 256), (5000, 64), (5000, 16)):
                for name, (g, each) in _plans(kind, case, is_max, nb, cus).items():
                    lds = g["lds"] + STATIC[name]
                    assert g["grid"] == _grid(cus, lds, each, nb), (name, case, is_max, nb, cus, g)
                    assert g["scratch"] == g["grid"] * each
                    seen.add("lds" if LDS_MAX // lds < 4 else "scratch" if SCRATCH_MAX // each < cus * 4 else "nb" if nb < cus * 4 else "cus")
    assert seen == {"lds", "scratch", "nb", "cus"}


def test_where_no_cut_depends_on_the_route_the_grids_are_equal():
    """The first shape: 4 workgroups per CU by LDS under every route's static share; at 64 CUs scratch for all of them."""
    for is_max in (True, False):
        for (nb, cus), want in (((5000, 64), 256), ((7, 256), 7), ((7, 64), 7)):
            p = _plans(F64, FIRST, is_max, nb, cus)
            assert [p[k][0]["grid"] for k in ("batch", "vc", "mip")] == [want] * 3
        for name, (g, each) in _plans(F64, FIRST, is_max, 5000, 256).items():
            assert g["grid"] == min(1024, SCRATCH_MAX // each), (name, g)
    assert bg.SMALL_LDS_STATIC == STATIC["batch"]
