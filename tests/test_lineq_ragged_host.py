"""CPU suite: the ragged projection / levels entry points (xpg_lineq_{project,levels}_batch_ragged_rat32: systems of mixed
shapes and lists in one launch of k_fme_chain_ragged) as far as they can be checked without a device -- the symbols, the plan
of a call through the host-only view xpg_test_lineq_ragged_plan against the restatement in tests/lineq_ragged_cases.py, the
envelope against the uniform plans where all shapes agree, every error code from the plan view and the entry points (decided
before the handle is looked at), and the C++ collectors' test, which must compile and link. The answers are
tests/test_gpu_lineq_ragged.py's."""
import ctypes as C
import os
import subprocess

import numpy as np

import lineq_levels_cases as lc
import lineq_project_cases as pc
import lineq_ragged_cases as rc
from lineq_ragged_cases import XPG_ERR_SHAPE, XPG_ERR_UNSUPPORTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("xpg_lineq_project_batch_ragged_rat32", "xpg_lineq_levels_batch_ragged_rat32", "xpg_lineq_ragged_last_route",
         "xpg_test_lineq_ragged_plan")


def _lib():
    from xpoly_amd import build, _capi
    build.build()
    return _capi.lib()


def build_adapter_test():
    from xpoly_amd import build
    build.build()
    exe = os.path.join(ROOT, "tests", "cxx", "levels_nests")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "levels_nests.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "xpoly_amd"), "-lxpoly_amd", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "xpoly_amd")])
    return exe


def test_the_library_exports_the_ragged_entry_points():
    lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "xpoly_amd.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name + "(" in hdr, name
    from xpoly_amd import _capi
    assert set(NAMES) <= set(_capi.SYMBOLS)
    from xpoly_amd.lineq import Lineq
    assert callable(Lineq.project_ragged) and callable(Lineq.levels_ragged) and callable(Lineq.ragged_last_route)


def _mixed(nb):
    """nb systems drawn from the base batch's four classes and the wide one, in a fixed order of no pattern."""
    shapes = rc.SHAPES + [rc.HOMES[:3], (40, 12, [11, 10, 9, 8, 7])]
    pick = np.random.default_rng(5).integers(0, len(shapes), size=nb)
    rows = [shapes[i][0] for i in pick]; cols = [shapes[i][1] + 1 for i in pick]; elims = [shapes[i][2] for i in pick]
    return rows, cols, [c - 1 for c in cols], elims


def test_plan_view_equals_the_restated_rule_for_mixed_batches():
    _lib()
    layouts = set()
    for nb in (1, 5, 48, 4096, 4396):
        rows, cols, rhs, elims = _mixed(nb)
        for levels in (False, True):
            for cap in (0, 37, 256, 1000):
                for cap_out in (0, 8, 5000):
                    got, want = rc.plan_view(rows, cols, rhs, elims, levels, cap, cap_out), rc.plan(rows, cols, rhs, elims, levels, cap, cap_out)
                    assert got == want, (nb, levels, cap, cap_out, got, want)
                    assert got["cols"] == max(cols) and got["rows"] == max(rows) and got["cap"] >= max(rows)
                    assert 1 <= got["cap_out"] <= got["cap"] and got["cap_lds"] * got["cols"] >= got["cap"]
                    slots = sum((len(e) if levels else 1) * c for e, c in zip(elims, cols))
                    assert got["out_bytes"] == slots * got["cap_out"] * 8 and got["groups"] == 1
                    assert got["seat_bytes"] == got["grid"] * 2 * got["cap"] * got["cols"] * 8
                    layouts.add(got["cap_lds"] == got["cap"])
    assert layouts == {True, False}
    # rhs_idx NULL is the last column of each; the defaults come from the system with the MOST rows
    rows, cols, rhs, elims = [4, 9, 5], [3, 5, 4], [2, 4, 3], [[1], [3, 2, 1], [2, 1]]
    assert rc.plan_view(rows, cols, None, elims, True) == rc.plan_view(rows, cols, rhs, elims, True)
    d = rc.plan_view(rows, cols, rhs, elims, False)
    assert d["cap"] == 9 * 9 // 4 + 9 + 1 == d["cap_out"] and d["cols"] == 5
    d = rc.plan_view([4, 40], [3, 13], [2, 12], [[1], [11]], True)
    assert d["cap"] == 40 * 40 // 4 + 40 + 1 and d["cap_out"] == 4 * 40 + 16
    assert rc.plan_view([4, 40], [3, 13], [2, 12], [[1], [11]], True, 5, 0)["cap"] == 40      # never under the most rows
    # the seats do not follow nb above the grid, the output slots do
    a, b = rc.plan_view(*_mixed(4096), True, 256), rc.plan_view(*_mixed(8192), True, 256)
    assert a["seat_bytes"] == b["seat_bytes"] and b["out_bytes"] > a["out_bytes"]


def test_the_envelope_of_equal_shapes_is_the_uniform_plan():
    _lib()
    for rows, cols, n_elim in ((4, 3, 1), (9, 5, 3), (12, 7, 2), (40, 13, 5), (60, 20, 6)):
        for nb in (1, 48, 4396):
            for cap, cap_out in ((0, 0), (256, 0), (256, 40), (100, 5000)):
                elims = [list(range(cols - 2, cols - 2 - n_elim, -1))] * nb
                args = ([rows] * nb, [cols] * nb, [cols - 1] * nb, elims)
                p, u = rc.plan_view(*args, False, cap, cap_out), pc.plan_view(nb, rows, cols, cap, cap_out)
                if not isinstance(u, dict):                  # (60 x 20 at its default capacity: over 160 KB, refused alike)
                    assert p == u == rc.plan_view(*args, True, cap, cap_out) == XPG_ERR_UNSUPPORTED and (rows, cap) == (60, 0)
                    continue
                assert all(p[k] == u[k] for k in pc.PLAN_KEYS[:6]) and (p["cap"], p["cap_out"]) == (u["cap"], u["cap_out"]), (p, u)
                assert p["out_bytes"] == nb * u["cap_out"] * cols * 8
                p, u = rc.plan_view(*args, True, cap, cap_out), lc.plan_view(nb, rows, cols, n_elim, cap, cap_out)
                assert all(p[k] == u[k] for k in lc.PLAN_KEYS[:6]) and (p["cap"], p["cap_out"]) == (u["cap"], u["cap_out"]), (p, u)
                assert p["out_bytes"] == u["level_bytes"]


def test_every_error_code_comes_from_the_plan():
    _lib()
    good = ([4, 9], [3, 5], [2, 4], [[1], [3, 2, 1]])
    assert isinstance(rc.plan_view(*good, True), dict)

    def with_(b, rows=None, cols=None, rhs=None, elim=None):
        r, c, h, e = (list(x) for x in good)
        if rows is not None: r[b] = rows
        if cols is not None: c[b] = cols
        if rhs is not None: h[b] = rhs
        if elim is not None: e[b] = elim
        return r, c, h, e

    for levels in (False, True):
        view = lambda a, **k: rc.plan_view(*a, levels, **k)
        assert view(with_(1, elim=[])) == XPG_ERR_SHAPE                              # n_elim[b] <= 0
        assert view(with_(1, elim=[4])) == XPG_ERR_SHAPE and view(with_(0, elim=[1, -1])) == XPG_ERR_SHAPE   # an index outside [0, rhs_idx[b])
        assert view(with_(1, rhs=0, elim=[0])) == XPG_ERR_SHAPE and view(with_(1, rhs=5)) == XPG_ERR_SHAPE   # rhs_idx[b] outside [1, cols[b])
        assert view(with_(0, rows=0)) == XPG_ERR_SHAPE and view(with_(0, cols=1, rhs=0, elim=[0])) == XPG_ERR_SHAPE
        assert view(with_(1, elim=[3] * (rc.CHAIN_MAX + 1))) == XPG_ERR_UNSUPPORTED   # a list above 64 entries
        assert isinstance(view(with_(1, elim=[3] * rc.CHAIN_MAX)), dict)
        # a shape error anywhere wins over a list too long anywhere
        r, c, h, e = with_(0, elim=[1] * (rc.CHAIN_MAX + 1))
        e[1] = [4]
        assert view((r, c, h, e)) == XPG_ERR_SHAPE
        assert view(good, cap_rows=32768) == XPG_ERR_UNSUPPORTED                     # cap > 32767
        assert view(good, cap_rows=5000) == XPG_ERR_UNSUPPORTED                      # the envelope's layout over 160 KB
        assert view(with_(0, rows=40, cols=13, rhs=12, elim=[11]), cap_rows=1600) == XPG_ERR_UNSUPPORTED
        assert isinstance(view(with_(0, rows=40, cols=13, rhs=12, elim=[11]), cap_rows=1200), dict)
        assert isinstance(view(good, cap_rows=1600), dict)                           # the same capacity at 5 columns fits
        assert view(good, nb=0) == XPG_ERR_SHAPE and view(good, eoff=[1, 2, 5]) == XPG_ERR_SHAPE and view(good, eoff=[0, 2, 1]) == XPG_ERR_SHAPE


def test_error_codes_of_the_entry_points_need_no_handle():
    """The entry points ask the same plan before they look at the handle: a list too long comes back as XPG_ERR_UNSUPPORTED
    and not as the XPG_ERR_SHAPE of the missing handle. No device is opened, nothing is launched."""
    lib = _lib()
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    mats = np.zeros((4 * 3 + 9 * 5, 2), dtype=np.int32); mats[:, 1] = 1
    off = np.array([0, 12], dtype=np.int64)
    ooff = np.zeros(70, dtype=np.int64); orows = np.zeros(70, dtype=np.int32); ok = np.zeros(2, dtype=np.int32); steps = np.zeros(2, dtype=np.int32)

    def call(name, elims, rhs=(2, 4), nb=2):
        r, c, h, el, eo = rc._args([4, 9], [3, 5], list(rhs), elims)
        return getattr(lib, name)(None, C.c_int(nb), vp(mats), vp(r), vp(c), vp(off), vp(h), vp(el), vp(eo), C.c_int(0), C.c_int(0), C.c_int(0),
                                  None, C.c_longlong(0), None, vp(ooff), vp(orows), vp(ok), vp(steps))

    for name in NAMES[:2]:
        assert call(name, [[1], [3] * (rc.CHAIN_MAX + 1)]) == XPG_ERR_UNSUPPORTED
        assert call(name, [[1], [3] * rc.CHAIN_MAX + [4]]) == XPG_ERR_SHAPE
        assert call(name, [[1], []]) == XPG_ERR_SHAPE and call(name, [[2], [3]]) == XPG_ERR_SHAPE
        assert call(name, [[1], [3]], rhs=(2, 5)) == XPG_ERR_SHAPE and call(name, [[0], [3]], rhs=(0, 4)) == XPG_ERR_SHAPE
        assert call(name, [[1], [3, 2]]) == XPG_ERR_SHAPE                            # a good batch: the missing handle
        ooff[0] = -1
        assert call(name, [[1], [3, 2]], nb=0) == 0 and ooff[0] == 0                 # no systems: 0 with offset 0
    route = np.full(7, -1, dtype=np.int64)
    assert lib.xpg_lineq_ragged_last_route(vp(route), C.c_int(7)) == 0 and route.tolist() == [0] * 7
    route[:] = -1
    assert lib.xpg_lineq_ragged_last_route(vp(route), C.c_int(3)) == 0 and route.tolist() == [0, 0, 0, -1, -1, -1, -1]
    assert lib.xpg_lineq_ragged_last_route(None, C.c_int(7)) == XPG_ERR_SHAPE


def test_the_collectors_compile_against_a_minimal_matrix_type():
    assert os.path.exists(build_adapter_test())
