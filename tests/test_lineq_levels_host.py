"""CPU suite: the levels entry points (xpg_lineq_levels_batch_*: a projection that keeps the rows after every step, one launch
of k_fme_levels_batch) as far as they can be checked without a device -- the symbols, the plan of a call through the host-only
view xpg_test_lineq_levels_plan against the restatement in tests/lineq_levels_cases.py (the default of a level's slot included),
the error codes of both entry points (the list's rules are asked before the handle), the ABI header as C99 with the new
prototypes, and the C++ adapter test, which must compile and link. The answers are tests/test_gpu_lineq_levels.py's."""
import ctypes as C
import os
import subprocess

import numpy as np

import lineq_levels_cases as lc
import lineq_project_cases as pc
from lineq_levels_cases import XPG_ERR_SHAPE, XPG_ERR_UNSUPPORTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("xpg_lineq_levels_batch_packed_rat32", "xpg_lineq_levels_batch_rat32_dev", "xpg_lineq_levels_last_route",
         "xpg_test_lineq_levels_plan")


def _lib():
    from xpoly_amd import build, _capi
    build.build()
    return _capi.lib()


def build_adapter_test():
    from xpoly_amd import build
    build.build()
    exe = os.path.join(ROOT, "tests", "cxx", "levels_all")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "levels_all.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "xpoly_amd"), "-lxpoly_amd", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "xpoly_amd")])
    return exe


def test_the_library_exports_the_levels_entry_points():
    lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "xpoly_amd.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name + "(" in hdr, name
    from xpoly_amd import _capi
    assert set(NAMES) <= set(_capi.SYMBOLS)
    from xpoly_amd.lineq import Lineq, levels_dev
    assert callable(Lineq.levels_packed) and callable(Lineq.levels_last_route) and callable(levels_dev)


def test_plan_view_equals_the_restated_rule():
    _lib()
    layouts, defaults = set(), set()
    for rows, cols in ((1, 2), (4, 3), (6, 5), (9, 5), (12, 7), (16, 9), (40, 13), (60, 20)):
        for n_elim in (1, 2, 5, 64):
            for cap in (0, rows, 37, 256, 1000):
                for cap_out in (0, 8, 5000):
                    for nb in (1, 48, 4096, 4396, 16384):
                        got, want = lc.plan_view(nb, rows, cols, n_elim, cap, cap_out), lc.plan(nb, rows, cols, n_elim, cap, cap_out)
                        assert got == want, (rows, cols, n_elim, cap, cap_out, nb, got, want)
                        if isinstance(got, dict):
                            assert got["cap"] >= rows and 1 <= got["cap_out"] <= got["cap"] and got["cap_lds"] * cols >= got["cap"]
                            assert got["level_bytes"] == nb * n_elim * got["cap_out"] * cols * 8
                            # the walk is the projection's: the same six figures, the same capacity of an intermediate
                            p = pc.plan_view(nb, rows, cols, cap, cap_out)
                            assert all(got[k] == p[k] for k in pc.PLAN_KEYS[:6]) and got["cap"] == p["cap"]
                            layouts.add(got["cap_lds"] == got["cap"])
                            if cap_out == 0:
                                defaults.add(got["cap_out"] == got["cap"])
    assert layouts == {True, False} and defaults == {True, False}
    # the defaults: fme's worst case for an intermediate, min(cap_rows, 4 * rows + 16) for a level's slot
    d = lc.plan_view(8, 40, 13, 5)
    assert d["cap"] == 40 * 40 // 4 + 40 + 1 and d["cap_out"] == 4 * 40 + 16
    d = lc.plan_view(8, 6, 5, 2)
    assert d["cap"] == 6 * 6 // 4 + 6 + 1 == d["cap_out"]                            # the worst case is the smaller one
    assert lc.plan_view(8, 12, 7, 2, 20, 0)["cap_out"] == 20 and lc.plan_view(8, 12, 7, 2, 500, 0)["cap_out"] == 64
    assert lc.plan_view(8, 12, 7, 2, 20, 21)["cap_out"] == 20                        # above cap_rows: cap_rows
    assert lc.plan_view(8, 12, 7, 2, 5, 0)["cap"] == 12                              # never under the input's rows
    # the level slots follow nb * n_elim, the seats do not follow nb above the grid
    a, b = lc.plan_view(4096, 9, 5, 3, 256), lc.plan_view(16384, 9, 5, 3, 256)
    assert a["seat_bytes"] == b["seat_bytes"] and b["level_bytes"] == 4 * a["level_bytes"]
    # refusals of the shape alone
    assert lc.plan_view(0, 4, 3, 1) == XPG_ERR_SHAPE and lc.plan_view(4, 0, 3, 1) == XPG_ERR_SHAPE and lc.plan_view(4, 4, 1, 1) == XPG_ERR_SHAPE
    assert lc.plan_view(4, 4, 3, 0) == XPG_ERR_SHAPE and lc.plan_view(4, 4, 3, -1) == XPG_ERR_SHAPE
    assert lc.plan_view(4, 4, 3, 65) == XPG_ERR_UNSUPPORTED
    assert lc.plan_view(4, 4, 3, 1, 32768) == XPG_ERR_UNSUPPORTED                    # cap > 32767
    assert lc.plan_view(4, 40, 13, 3, 1600) == XPG_ERR_UNSUPPORTED                   # the layout of cap rows over 160 KB
    assert isinstance(lc.plan_view(4, 40, 13, 3, 1200), dict)


def test_error_codes_of_both_entry_points_need_no_handle():
    """The list's rules come from project_check, the function the projection asks, and are answered before the handle is looked
    at: a list too long comes back as XPG_ERR_UNSUPPORTED and not as the XPG_ERR_SHAPE of the missing handle. No device is
    opened, nothing is launched."""
    lib = _lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    mats = np.zeros((2, 4, 5, 2), dtype=np.int32); mats[..., 1] = 1
    off = np.zeros(2 * 65 + 1, dtype=np.int64); ok = np.zeros(2, dtype=np.int32); steps = np.zeros(2, dtype=np.int32)

    def packed(rhs, elim, n=None):
        el = np.asarray(elim, dtype=np.int32)
        return lib.xpg_lineq_levels_batch_packed_rat32(None, C.c_int(2), vp(mats), C.c_int(4), C.c_int(5), C.c_int(rhs),
                                                       vp(el) if el.size else None, C.c_int(el.size if n is None else n),
                                                       C.c_int(0), C.c_int(0), C.c_int(0), None, C.c_longlong(0), None, vp(off), vp(ok), vp(steps))

    def dev(rhs, elim, n=None):
        el = np.asarray(elim, dtype=np.int32)
        return lib.xpg_lineq_levels_batch_rat32_dev(None, C.c_int(2), None, C.c_int(4), C.c_int(5), C.c_int(rhs),
                                                    vp(el) if el.size else None, C.c_int(el.size if n is None else n), C.c_int(0),
                                                    C.c_int(8), C.c_int(8), None, None, None, None)

    for call in (packed, dev):
        assert call(4, [3] * (pc.CHAIN_MAX + 1)) == XPG_ERR_UNSUPPORTED              # more than 64 entries
        assert call(4, [3] * pc.CHAIN_MAX + [4]) == XPG_ERR_SHAPE                    # a bad index wins over the length
        assert call(4, []) == XPG_ERR_SHAPE and call(4, [3], n=0) == XPG_ERR_SHAPE and call(4, [3], n=-1) == XPG_ERR_SHAPE
        assert call(4, [4]) == XPG_ERR_SHAPE and call(4, [3, -1]) == XPG_ERR_SHAPE   # an index outside [0, rhs_idx)
        assert call(0, [0]) == XPG_ERR_SHAPE and call(5, [3]) == XPG_ERR_SHAPE       # rhs_idx outside [1, cols)
        assert call(4, [3, 2]) == XPG_ERR_SHAPE and call(4, [3, 3]) == XPG_ERR_SHAPE  # a good list: the missing handle
    route = np.full(7, -1, dtype=np.int64)
    assert lib.xpg_lineq_levels_last_route(vp(route), C.c_int(7)) == 0 and route.tolist() == [0] * 7
    route[:] = -1
    assert lib.xpg_lineq_levels_last_route(vp(route), C.c_int(3)) == 0 and route.tolist() == [0, 0, 0, -1, -1, -1, -1]
    assert lib.xpg_lineq_levels_last_route(None, C.c_int(7)) == XPG_ERR_SHAPE
    assert lib.xpg_test_lineq_levels_plan(C.c_int(4), C.c_int(4), C.c_int(3), C.c_int(1), C.c_int(0), C.c_int(0), None, C.c_int(9)) == XPG_ERR_SHAPE


def test_the_header_is_c99_with_the_new_prototypes():
    """tests/cxx/levels_abi_c99.c takes the address of every new entry point through the prototypes of the header, compiled as
    C99 under -Werror, and asks the host-only plan view: no device is opened."""
    _lib()
    exe = os.path.join(ROOT, "tests", "cxx", "levels_abi_c99")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "levels_abi_c99.c"), "-o", exe,
                           "-L", os.path.join(ROOT, "xpoly_amd"), "-lxpoly_amd", "-Wl,-rpath," + os.path.join(ROOT, "xpoly_amd")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    want = lc.plan(48, 9, 5, 3, 256, 0)
    assert r.stdout.split() == [str(want[k]) for k in lc.PLAN_KEYS], (r.stdout, want)


def test_the_adapter_test_compiles_and_links():
    assert os.path.exists(build_adapter_test())
