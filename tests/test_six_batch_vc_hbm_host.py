"""CPU suite: the route rule of xpg_six_batch_vc_hbm_* -- which batches keep the LDS-resident kernel, which get slots in device
memory, which go per problem -- and the sizes of the launch, through the host-only view xpg_test_six_batch_vc_hbm_plan (no
device is opened) against the restatement in tests/six_vc_hbm_cases.py; and what the committed GPU cases hold, from the CPU
restatement of the reference alone (answers shared with tests/test_gpu_six_batch_vc_hbm.py)."""
import ctypes as C

import numpy as np
import pytest

import batch_geometry as bg
import batch_hbm_cases as hc
import free_var_cases as fc
import six_eq_cases as sc
import six_vc_hbm_cases as vc
from six_vc_hbm_cases import F64, RAT
from tools import gen

XPG_ERR_SHAPE = -3
SHAPES = vc.PAIRS_SHAPES + vc.FOLD_SHAPES + (vc.TALL,) + tuple(vc.SUCC_SHAPES.values())


def _vc(kind, nv, nfree):
    return gen.vc_nonneg(nv, kind == F64, range(nfree))


def _view(kind, vc_arr, leq_rows, eq_rows, cols, is_max, nb, cus=256):
    from xpoly_amd.six import SIX_BATCH_VC_HBM_FIELDS, six_batch_vc_hbm_plan
    assert SIX_BATCH_VC_HBM_FIELDS == vc.FIELDS
    return six_batch_vc_hbm_plan(kind, vc_arr, leq_rows, eq_rows, cols, is_max, nb, cus)


def _view_shape(kind, shape, is_max, nb, cus=256, dev=False):
    m, me, nv, nfree = shape
    return _view(kind, None if dev else _vc(kind, nv, nfree), m, me, nv + 1, is_max, nb, cus)


@pytest.mark.parametrize("kind", [F64, RAT])
def test_view_equals_the_restated_rule(kind):
    routes = set()
    for shape in SHAPES + sc.SHAPES + ((64, 2, 64, 2), (20, 2, 20, 1), (100, 0, 100, 0), (0, 40, 60, 3)):
        for is_max in (True, False):
            for nb in (1, 64, 5000):
                for cus in (64, 256):
                    for dev in (False, True):
                        got, want = _view_shape(kind, shape, is_max, nb, cus, dev), vc.plan_of_shape(kind, shape, is_max, nb, cus, dev)
                        assert got == want, (kind, shape, is_max, nb, cus, dev, got, want)
                        routes.add(got["route"])
                        if got["route"] == vc.ROUTE_HBM:
                            R, V = got["Rmax"], got["Vmax"]
                            assert got["ld"] % 2 == 0 and 0 <= got["ld"] - (V + R + 2) <= 1
                            assert got["slot"] % 256 == 0 and got["slot"] > R * got["ld"] * 8
                            assert 1 <= got["grid"] <= nb and got["scratch"] == got["grid"] * got["slot"] <= vc.SCRATCH_MAX
                            assert got["lds"] == hc.side_bytes(kind, R, V) and got["lds"] + vc.LDS_STATIC <= vc.LDS_MAX
                            assert got["threads"] == 256
                            assert bg.small_lds_bytes(kind, R, V) > vc.SIX_VC_LDS_MAX
    assert routes == {vc.ROUTE_LDS, vc.ROUTE_HBM}


def test_the_shapes_of_the_gpu_cases_take_the_routes_their_tests_assume():
    for kind in (F64, RAT):
        for shape in (vc.FIRST, vc.ODD) + vc.FOLD_SHAPES:
            for is_max in (True, False):
                assert _view_shape(kind, shape, is_max, 64)["route"] == vc.ROUTE_HBM
        assert _view_shape(kind, vc.SPLIT, True, 64)["route"] == vc.ROUTE_LDS
        assert _view_shape(kind, vc.SPLIT, False, 64)["route"] == vc.ROUTE_HBM
        assert _view_shape(kind, vc.SPLIT, True, 64, dev=True)["route"] == vc.ROUTE_HBM     # with every variable free it is past 64 KB
        assert _view_shape(kind, vc.TALL, True, 64)["route"] == vc.ROUTE_HBM
    # the figures the cases are named by (fp64)
    assert sc.plan_bytes(60, 4, 62, 2, True) == 81808 and sc.plan_bytes(60, 4, 62, 2, False) == 77472
    assert sc.plan_bytes(30, 3, 130, 2, True) == 60256 and sc.plan_bytes(30, 3, 130, 2, False) == 191968
    # both parities of the widest width: one padded column where it is odd
    a, b = _view_shape(F64, vc.FIRST, True, 64), _view_shape(F64, vc.ODD, True, 64)
    assert (a["Vmax"] + a["Rmax"] + 2) % 2 == 0 and a["ld"] == a["Vmax"] + a["Rmax"] + 2
    assert (b["Vmax"] + b["Rmax"] + 2) % 2 == 1 and b["ld"] == b["Vmax"] + b["Rmax"] + 3
    for shape in vc.SUCC_SHAPES.values():
        assert all(_view_shape(F64, shape, d, 16)["route"] == vc.ROUTE_HBM for d in (True, False))


@pytest.mark.parametrize("is_max", [True, False])
@pytest.mark.parametrize("kind", [F64, RAT])
def test_the_64_kb_edge(kind, is_max):
    """The last square shape xpg_six_batch_vc_* takes on the device keeps that launch; the next one, which it sends to the
    per-problem route, is the first to get slots."""
    for eq_rows, nfree in ((1, 0), (2, 2)):
        nv = sc.largest_square(is_max, eq_rows, nfree, kind)
        fits, past = _view(kind, _vc(kind, nv, nfree), nv, eq_rows, nv + 1, is_max, 256), _view(kind, _vc(kind, nv + 1, nfree), nv + 1, eq_rows, nv + 2, is_max, 256)
        assert fits["route"] == vc.ROUTE_LDS and fits["lds"] == sc.plan_bytes(nv, eq_rows, nv, nfree, is_max, kind) <= vc.SIX_VC_LDS_MAX
        assert past["route"] == vc.ROUTE_HBM and sc.plan_bytes(nv + 1, eq_rows, nv + 1, nfree, is_max, kind) > vc.SIX_VC_LDS_MAX
        rc, old = sc.plan_view(_vc(kind, nv, nfree), kind, nv, eq_rows, is_max)
        assert rc == 0 and old[0] == 1 and old[4] == fits["lds"]
        rc, old = sc.plan_view(_vc(kind, nv + 1, nfree), kind, nv + 1, eq_rows, is_max)
        assert rc == 0 and old[0] == 0                              # xpg_six_batch_vc_* itself still falls back there


@pytest.mark.parametrize("kind", [F64, RAT])
def test_what_the_rule_refuses(kind):
    # a general vc: per problem whatever the size
    for vc0 in fc.general_vcs(62):
        arr = np.ascontiguousarray(vc0, dtype=np.float64) if kind == F64 else vc0
        for shape in (vc.FIRST, (5, 2, 62, 0)):
            g = _view(kind, arr, shape[0], shape[1], 63, True, 64)
            assert g["route"] == vc.ROUTE_OTHER and g["grid"] == 0 and g["scratch"] == 0 and g["nfree"] == 0
            assert g == vc.plan(kind, False, 0, shape[0], shape[1], 63, True, 64)
    # the pivot-pair table outgrows LDS at about R + V = 960
    for is_max in (True, False):
        g = _view_shape(kind, (600, 2, 500, 1), is_max, 16)
        assert g["route"] == vc.ROUTE_OTHER and g["lds"] + vc.LDS_STATIC > vc.LDS_MAX and g == vc.plan_of_shape(kind, (600, 2, 500, 1), is_max, 16)
    # more equalities than the ballots' bit masks hold (4096; their pairs alone outgrow the pair table as well)
    for is_max in (True, False):
        g = _view_shape(kind, (2, 4097, 3, 0), is_max, 16)
        assert g["route"] == vc.ROUTE_OTHER and g == vc.plan_of_shape(kind, (2, 4097, 3, 0), is_max, 16)
    # the _dev forms size for every variable free: a shape that fits with its real vc may be refused there
    m, me, nv, nfree = 400, 2, 400, 0
    assert _view_shape(kind, (m, me, nv, nfree), True, 16)["route"] == vc.ROUTE_HBM
    assert _view_shape(kind, (m, me, nv, nfree), True, 16, dev=True)["route"] == vc.ROUTE_OTHER


@pytest.mark.parametrize("kind", [F64, RAT])
def test_static_lds_is_counted_at_the_160_kb_edge(kind):
    """The side arrays alone may fill 160 KB to the byte and the launch would still fail: the kernel holds 272 bytes of its own
    (the solver's reduction scratch and the four ints of nf_*). Shapes whose side arrays fit and whose sum does not are refused."""
    assert vc.LDS_STATIC == 272
    between, last_ok = [], None
    for total in range(940, 975):                                # rows + variables of the normal form: the pair table grows with their sum,
        for rows in range(40, total - 40, 3):                    # the rows add 20 bytes each
            nv = total - rows
            side = hc.side_bytes(kind, rows + 2, nv)
            if side <= vc.LDS_MAX < side + vc.LDS_STATIC:
                between.append((rows, nv))
            elif side + vc.LDS_STATIC <= vc.LDS_MAX and (last_ok is None or side > last_ok[2]):
                last_ok = (rows, nv, side)
    assert between and last_ok and vc.LDS_MAX - last_ok[2] - vc.LDS_STATIC < 1024, (between[:3], last_ok)
    for rows, nv in between[:4]:
        g = _view_shape(kind, (rows, 1, nv, 0), True, 16)
        assert g["route"] == vc.ROUTE_OTHER and g["lds"] <= vc.LDS_MAX < g["lds"] + vc.LDS_STATIC, g
    g = _view_shape(kind, (last_ok[0], 1, last_ok[1], 0), True, 16)
    assert g["route"] == vc.ROUTE_HBM and g["lds"] == last_ok[2] and g["grid"] == 16


def test_the_grid_is_cut_by_lds_by_scratch_and_by_nb():
    g = _view_shape(F64, vc.FIRST, True, 5000, 256)
    assert g["grid"] == 4 * 256 and g["scratch"] == g["grid"] * g["slot"]             # 16 wavefronts of 256 threads: 4 per CU
    assert _view_shape(F64, vc.FIRST, True, 5000, 64)["grid"] == 256 and _view_shape(F64, vc.FIRST, True, 7, 256)["grid"] == 7
    g = _view_shape(F64, (400, 2, 398, 2), True, 5000, 256)                            # 2.6 MB slots; 122 KB of side arrays: one per CU
    assert g["route"] == vc.ROUTE_HBM and g["grid"] == min(256, vc.SCRATCH_MAX // g["slot"]) < 256 and g["scratch"] <= vc.SCRATCH_MAX


def test_malformed_calls_and_the_raw_view():
    from xpoly_amd._capi import lib
    arr = _vc(F64, 62, 2)
    p = arr.ctypes.data_as(C.c_void_p)
    out = (C.c_longlong * 11)(*([-99] * 11))
    call = lambda kind, vcp, vc_rows, m, me, cols, nb, cus, n=10: lib().xpg_test_six_batch_vc_hbm_plan(
        C.c_int(kind), vcp, C.c_int(vc_rows), C.c_int(m), C.c_int(me), C.c_int(cols), C.c_int(1), C.c_int(nb), C.c_int(cus), out, C.c_int(n))
    assert call(0, p, 62, 60, 4, 63, 64, 256, n=3) == 0 and list(out)[:3] == [1, 2, 68] and list(out)[3:] == [-99] * 8
    assert call(0, p, 61, 60, 4, 63, 64, 256) == XPG_ERR_SHAPE                      # vc_rows != cols - 1
    assert call(0, p, 62, 0, 0, 63, 64, 256) == XPG_ERR_SHAPE
    assert call(0, p, 62, 60, 4, 63, 0, 256) == XPG_ERR_SHAPE                       # the view describes a launch: nb = 0 has none
    assert call(0, p, 62, 60, 4, 63, 64, 0) == XPG_ERR_SHAPE
    assert call(2, p, 62, 60, 4, 63, 64, 256) == XPG_ERR_SHAPE
    assert call(0, None, 0, 60, 4, 63, 64, 256) == 0 and out[1] == -1               # the _dev forms' view
    route = (C.c_longlong * 5)()
    assert lib().xpg_six_batch_vc_hbm_last_route(route, C.c_int(5)) == 0
    assert lib().xpg_six_batch_vc_hbm_last_route(None, C.c_int(5)) == XPG_ERR_SHAPE
    for name in ("xpg_six_batch_vc_hbm_f64", "xpg_six_batch_vc_hbm_rat32"):
        assert getattr(lib(), name)(None, 1, 0, None, None, None, 4, None, 60, 63, 10, None, None, None) == XPG_ERR_SHAPE
    for name in ("xpg_six_batch_vc_hbm_f64_dev", "xpg_six_batch_vc_hbm_rat32_dev"):
        assert getattr(lib(), name)(None, 1, 0, None, None, None, 4, None, 60, 63, 10, None, None, None, None) == XPG_ERR_SHAPE


# ---- what the GPU cases hold, from the restatement alone ------------------------------------------------------------------
def _all_answers():
    for fam, shape, is_max in vc.F64_CASES:
        for cap in vc.CAPS:
            yield (fam, F64, cap), vc.oracle_answers(fam, shape, F64, is_max, vc.COUNT, cap)
    for is_max in (True, False):
        yield ("succ", F64, vc.NO_LIMIT), vc.oracle_answers("succ", vc.SUCC_SHAPES[is_max], F64, is_max, vc.SUCC_COUNT)
    for fam, shape, is_max in vc.RAT_CASES:
        yield (fam, RAT, vc.RAT_CAP), vc.oracle_answers(fam, shape, RAT, is_max, vc.RAT_COUNT, vc.RAT_CAP)


def test_the_oracle_statuses_cover_every_end_and_minus_7_is_the_tall_case_alone():
    seen, fold_rat_ok, pivots = set(), 0, set()
    for (fam, kind, cap), want in _all_answers():
        st = [w[0] for w in want]
        assert -7 not in st, (fam, kind, cap, st)
        seen |= set(st)
        pivots |= {w[3] for w in want}
        if fam == "fold" and kind == RAT:
            fold_rat_ok += st.count(0)
    assert seen >= {0, 2, 3, 4}, seen
    assert fold_rat_ok >= 4, fold_rat_ok                         # they carry the solution comparison for the fold
    assert len(pivots) >= 20
    for kind, count, cap in ((F64, vc.COUNT, 300), (F64, vc.COUNT, 48), (RAT, vc.RAT_COUNT, vc.RAT_CAP)):
        st = [w[0] for w in vc.oracle_answers("tall", vc.TALL, kind, True, count, cap)]
        assert all((s == -7) == (i % 2 == 1) for i, s in enumerate(st)), st
        assert len({s for s in st if s != -7}) >= 2, st


def test_the_fold_batches_are_ragged_and_the_succ_batches_succeed():
    """Even "fold" LPs substitute one equality (the normal form keeps leq_rows + 2 (eq_rows - 1) rows), odd ones none: the host
    restatement of convertEq2Ineq's choice says so. Status 0 of the block LPs comes with a non-zero optimum."""
    for shape in vc.FOLD_SHAPES:
        for is_max in (True, False):
            tg, _, eq, leq = vc.arrays("fold", shape, F64, is_max, vc.COUNT)
            for i in range(vc.COUNT):
                private = [c for c in range(shape[2]) if np.count_nonzero(eq[i, :, c]) == 1]
                assert bool(private) == (i % 2 == 0), (shape, i)
        for fam, s in (("pairs", vc.FIRST), ("pairs", vc.SPLIT)):
            _, _, eq, _ = vc.arrays(fam, s, F64, True, vc.COUNT)
            assert not any(np.count_nonzero(eq[i, :, c]) == 1 for i in range(vc.COUNT) for c in range(s[2]))
    for is_max in (True, False):
        want = vc.oracle_answers("succ", vc.SUCC_SHAPES[is_max], F64, is_max, vc.SUCC_COUNT)
        assert any(w[0] == 0 for w in want) and all(float(w[1]) != 0.0 for w in want if w[0] == 0)
