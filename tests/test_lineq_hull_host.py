"""CPU suite: the hull calls (xpg_lineq_hull_batch_ragged_rat32, xpg_lineq_project_union_batch_ragged_rat32: a producer launch,
then k_group_reduce, one reduce per group) as far as they can be checked without a device -- the symbols, the plan of a call
through the host-only view xpg_test_lineq_hull_plan against the restatement in tests/lineq_hull_cases.py, the golden file
(the composition run on the real reference) against the CPU checker, every argument error, the facts of the batch the GPU
cases rest on, and the C++ collectors, which must compile and link. The answers are tests/test_gpu_lineq_hull.py's."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

import lineq_bounds_cases as bc
import lineq_hull_cases as hc
from lineq_hull_cases import XPG_ERR_SHAPE, XPG_ERR_UNSUPPORTED, rows_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("xpg_lineq_hull_batch_ragged_rat32", "xpg_lineq_project_union_batch_ragged_rat32", "xpg_lineq_hull_last_route",
         "xpg_lineq_project_union_last_route", "xpg_test_lineq_hull_plan")


def _lib():
    from xpoly_amd import build, _capi
    build.build()
    return _capi.lib()


def build_collector():
    from xpoly_amd import build
    build.build()
    exe = os.path.join(ROOT, "tests", "cxx", "hull_all")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "hull_all.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "xpoly_amd"), "-lxpoly_amd", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "xpoly_amd")])
    return exe


def test_the_library_exports_the_entry_points():
    lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "xpoly_amd.h")).read()
    from xpoly_amd._capi import SYMBOLS
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name + "(" in hdr and name in SYMBOLS, name
    from xpoly_amd.lineq import Lineq
    assert callable(Lineq.hull_ragged) and callable(Lineq.project_union_ragged) and callable(Lineq.hull_ragged_last_route)
    adapter = open(os.path.join(ROOT, "include", "xpoly_amd", "lineq.hpp")).read()
    assert "ConvexHullUnionAndIntersect" in adapter and "hull_all" in adapter and "project_union_each" in adapter


def test_the_batch_the_gpu_cases_rest_on(port):
    """The facts asserted of the checker's answers before anything is asserted of a device: which groups are empty, that no
    member fails, how many rows each group gathers, which home each group gets."""
    groups, rhss, names = hc.hull_batch(port)
    assert len(groups) == hc.NG and [n for g, n in zip(groups, names) if not g] == ["empty", "c4 x0", "c0 x0", "c2 x0", "c4 x0"]
    assert all(bc.chains(port, m, r, 512, 512)[0] == 1 for g, r in zip(groups, rhss) for m in g)
    w = hc.want(port, groups, rhss, False, cap_rows=512, cap_out_rows=512)
    by = dict(zip(names, w))
    assert [by[n][5] for n in ("overlap", "aba", "disjoint", "symbols", "c3 x17", "c5 x17", "rhs cols-2")] == [9, 13, 9, 14, 81, 91, 39]
    assert sum(x[5] for x in w) == sum(1 + sum(t.shape[0] for m in g for t in bc.chains(port, m, r)[3]) for g, r in zip(groups, rhss) if g)
    sizes, rows, cols, rhs = hc.shapes_of(groups, rhss)
    for caps, dev in (((512, 0, 0), []), ((512, 16, 1000), ["c3 x17", "c5 x17", "c3 x17"]), ((512, 16, 600), [])):
        p, homes, gcaps = hc.plan_view(sizes, rows, cols, rhs, None, *caps)
        assert [names[g] for g, h in enumerate(homes) if h == hc.HOME_DEVICE] == dev, caps
        assert [g for g, h in enumerate(homes) if h == hc.HOME_NONE] == [g for g, m in enumerate(groups) if not m]
        assert all(x[5] <= c for x, c, m in zip(w, gcaps, groups) if m)                # what a group gathers is within its capacity


def test_plan_view_equals_the_restated_rule():
    _lib()
    rng = np.random.default_rng(3)
    seen = set()
    for trial in range(60):
        ng = int(rng.integers(1, 9))
        sizes = [int(rng.choice([0, 1, 2, 3, 17, 40])) for _ in range(ng)]
        rows, cols, rhs = [], [], []
        for n in sizes:
            c = int(rng.integers(2, 9)); r = int(rng.integers(1, c))
            rows += [int(x) for x in rng.integers(1, 12, size=n)]; cols += [c] * n; rhs += [r] * n
        for caps in ((0, 0, 0), (64, 8, 0), (512, 16, 1000), (512, 0, 300), (64, 4, 5000)):
            for union in (False, True):
                elims = [list(range(r - 1, -1, -1))[:max(r - 1, 1)] for r in rhs] if union else None
                got, want = hc.plan_view(sizes, rows, cols, rhs, elims, *caps), hc.plan(sizes, rows, cols, rhs, elims, *caps)
                assert got == want, (trial, sizes, caps, union, got, want)
                if isinstance(got, tuple):
                    seen |= set(got[1])
                    p, homes, gcaps = got
                    assert p["groups_lds"] + p["groups_device"] == sum(1 for n in sizes if n)
                    assert (p["slot_bytes"] > 0) == (p["groups_device"] > 0) and p["cap_hull"] >= 1
    assert seen == {hc.HOME_NONE, hc.HOME_LDS, hc.HOME_DEVICE}
    # the default cap_hull_rows: the largest lead + 2 x rhs x members, at most 32767; the union has no lead row
    assert hc.plan_view([2, 5], [4] * 7, [5] * 7, [4] * 7)[0]["cap_hull"] == 1 + 2 * 4 * 5
    assert hc.plan_view([2, 5], [4] * 7, [5] * 7, [4] * 7, [[3, 2, 1]] * 7)[0]["cap_hull"] == 2 * 4 * 5
    assert hc.plan_view([3000], [2] * 3000, [7] * 3000, None, None, 0, 0, 0) == XPG_ERR_UNSUPPORTED     # 32767 rows of scratch: over 160 KB
    assert hc.plan_view([3000], [2] * 3000, [7] * 3000, None, None, 0, 0, 4000)[0]["cap_hull"] == 4000
    # the device slots are capped at 1 GiB: the grid is lowered
    p = hc.plan_view([40] * 3000, [2] * 120000, [9] * 120000, None, None, 64, 64, 12000)[0]
    assert p["groups_device"] == 3000 and p["grid"] == (1 << 30) // (12000 * 9 * 8) < 3000 and p["slot_bytes"] <= 1 << 30
    # groups without members only
    assert hc.plan_view([0, 0], [], [], None) == hc.plan([0, 0], [], [], None)


def test_the_golden_file_against_the_checker(port):
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "g14_hull.json")))
    cases = g["cases"]
    assert len(cases) == 88 and {c["kind"] for c in cases} == {"hull", "union"}
    for c in cases:
        members = [np.array(m["cells"], dtype=np.int32).reshape(m["rows"], m["cols"], 2) for m in c["members"]]
        if c["kind"] == "hull":
            got = hc.hull(port, members, c["rhs"], bool(c["is_intersect"]))
        else:
            got = hc.project_union(port, members, c["rhs"], [c["elim"]] * len(members), bool(c["is_intersect"]))
        cols = members[0].shape[1] if members else 0
        want_rows = np.array(c["out"], dtype=np.int32).reshape(c["out_rows"], cols, 2)
        assert (got[0], got[1], got[5]) == (c["ok"], c["member"], c["gathered"]), c["name"]
        assert rows_equal(got[4], want_rows), c["name"]
    # the hull composed from the checker's fme chains is the one composed from its calc_bound
    groups, rhss, _ = hc.hull_batch(port)
    for members, rhs in zip(groups[:12], rhss[:12]):
        if members:
            res = [hc.rat([[0] * members[0].shape[1]])]
            for m in members:
                ok, bounds = port.calc_bound(m, rhs)
                assert ok
                res += [t for t in bounds if t.shape[0]]
            ok, rows = port.reduce(np.concatenate(res), rhs, False)
            w = hc.hull(port, members, rhs, False)
            assert w[0] == (1 if ok else 0) and rows_equal(w[4], rows)


def test_every_argument_error():
    lib = _lib()
    pv = hc.plan_view
    four = dict(rows=[4, 4, 5, 5], cols=[5, 5, 3, 3])
    assert isinstance(pv([2, 2], **four), tuple)
    assert pv([2, 2], [4, 4, 5, 5], [5, 4, 3, 3]) == XPG_ERR_SHAPE                             # mixed cols in a group
    assert pv([2, 2], rhs=[4, 3, 2, 2], **four) == XPG_ERR_SHAPE                               # mixed rhs_idx in a group
    assert isinstance(pv([2, 2], rhs=[3, 3, 2, 2], **four), tuple)                            # groups may differ in everything
    assert pv([2, 2], goff=[0, 3, 2], **four) == XPG_ERR_SHAPE and pv([2, 2], goff=[1, 2, 4], **four) == XPG_ERR_SHAPE   # not monotone; not from 0
    assert pv([2, 2], goff=[0, 2, 3], **four) == XPG_ERR_SHAPE and pv([2, 2], goff=[0, 2, 5], **four) == XPG_ERR_SHAPE   # not ending at n_members
    assert pv([], **four) == XPG_ERR_SHAPE                                                     # no groups, but members
    assert pv([2, 2], cap_hull_rows=32768, **four) == XPG_ERR_UNSUPPORTED
    assert isinstance(pv([2, 2], cap_hull_rows=12000, **four), tuple) and pv([2, 2], cap_hull_rows=20000, **four) == XPG_ERR_UNSUPPORTED
    assert pv([2, 2], cap_rows=32768, **four) == XPG_ERR_UNSUPPORTED                           # the producer's refusals are passed on
    assert pv([2, 2], [4, 0, 5, 5], [5, 5, 3, 3]) == XPG_ERR_SHAPE
    assert pv([2, 2], elims=[[3, 2, 1], [3, 2, 1], [1], [2]], **four) == XPG_ERR_SHAPE         # a list entry outside [0, rhs)
    assert isinstance(pv([2, 2], elims=[[3, 2, 1], [3, 2, 1], [1], [1, 0]], **four), tuple)
    # the calls themselves without a handle and with what they refuse: no device is opened, nothing is launched
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    mats = np.zeros((2 * 4 * 5, 2), dtype=np.int32); mats[..., 1] = 1
    rows, cols, offs = i32([4, 4]), i32([5, 5]), np.array([0, 20], dtype=np.int64)
    ooff = np.full(3, 7, dtype=np.int64); orows = np.zeros(2, dtype=np.int32)
    v = [np.full(2, 9, dtype=np.int32) for _ in range(4)]

    def call(ng=2, goff=(0, 1, 2), nb=2, rhs=None, cap_hull=0, ooff_=ooff, union=False, eoff=(0, 1, 2)):
        head = (None, C.c_int(ng), vp(i32(goff)), C.c_int(nb), vp(mats), vp(rows), vp(cols), vp(offs), vp(rhs))
        tail = (C.c_int(0), C.c_int(0), C.c_int(cap_hull), None, C.c_longlong(0), None, vp(ooff_), vp(orows), vp(v[0]), vp(v[1]), vp(v[2]), vp(v[3]))
        if union:
            return lib.xpg_lineq_project_union_batch_ragged_rat32(*head, vp(i32([1, 1])), None if eoff is None else vp(i32(eoff)), C.c_int(0), C.c_int(0), *tail)
        return lib.xpg_lineq_hull_batch_ragged_rat32(*head, C.c_int(0), *tail)

    for union in (False, True):
        assert call(union=union) == XPG_ERR_SHAPE                                              # no handle
        assert call(goff=(0, 2, 2), rhs=i32([4, 3]), union=union) == XPG_ERR_SHAPE
        assert call(goff=(0, 2, 1), union=union) == XPG_ERR_SHAPE and call(ng=-1, union=union) == XPG_ERR_SHAPE
        assert call(cap_hull=32768, union=union) == XPG_ERR_UNSUPPORTED                        # decided before the handle is looked at
        assert call(ooff_=None, union=union) == XPG_ERR_SHAPE
        assert call(ng=0, nb=2, union=union) == XPG_ERR_SHAPE
    assert call(union=True, eoff=None) == XPG_ERR_SHAPE
    route = np.full(10, -1, dtype=np.int64)
    for name in ("xpg_lineq_hull_last_route", "xpg_lineq_project_union_last_route"):
        assert getattr(lib, name)(vp(route), C.c_int(10)) == 0 and route.tolist() == [0] * 10
        assert getattr(lib, name)(None, C.c_int(10)) == XPG_ERR_SHAPE
    # no groups: 0, the one offset written; groups without members: answered without a handle
    assert call(ng=0, nb=0) == 0 and ooff[0] == 0 and ooff[1] == 7
    assert call(goff=(0, 0, 0), nb=0) == 0 and ooff.tolist() == [0, 0, 0] and v[0].tolist() == [1, 1] and v[1].tolist() == [-1, -1]


def test_the_collectors_compile_and_link():
    assert os.path.exists(build_collector())
