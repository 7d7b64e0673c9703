"""Lineq::has_solution with is_int_sol = true for a batch in one call that synchronises once (xpg_has_solution_int_batch_*): the
objective, both MIP walks and the verdict on the device.

Checker (tests/has_solution_int_cases.py): the CPU restatement, non-strict wherever a variable is free -- port.has_solution(...,
True, u) for the verdicts, port.mip_solve on the feasibility objective for the two statuses --, each case's answers computed once.
The status pairs are also compared, byte for byte, with what has_solution_batch(is_int_sol=True) -- the composition on the host
this call replaces -- returns on the same arrays in the same process. Every comparison is exact."""
import subprocess
import sys

import numpy as np
import pytest

import free_var_cases as fc
import has_solution_cases as hs
import has_solution_int_cases as hi
from conftest import ROOT, hooks_env, needs_hooks
from tools import gen

pytestmark = pytest.mark.gpu
XPG_ERR_SHAPE, XPG_ERR_REF_UNDEFINED = -3, -7


def _new(ctx, arrays, unique):
    from xpoly_amd.six import has_solution_int_batch, has_solution_int_last_route
    vc_arr, eq, leq = arrays
    has, st = has_solution_int_batch(ctx, leq, eq, vc_arr, unique, want_status=True)
    return has, st, has_solution_int_last_route()


def _parent(ctx, arrays, unique):
    from xpoly_amd.six import has_solution_batch
    vc_arr, eq, leq = arrays
    return has_solution_batch(ctx, leq, eq, vc_arr, True, unique, want_status=True)


def _check(ctx, arrays, want, unique, what):
    """One call against the checker and against the parent's route; returns (has, status, route)."""
    has, st, route = _new(ctx, arrays, unique)
    want_has, want_st = hi.expected(want, unique)
    old_has, old_st = _parent(ctx, arrays, unique)
    pairs = [(int(a), int(b)) for a, b in st]
    print("%s u=%d route %s verdicts %s pairs %s" % (what, unique, route, {int(h): int((has == h).sum()) for h in set(has.tolist())},
                                                     {p: pairs.count(p) for p in sorted(set(pairs))}))
    assert has.tolist() == want_has.tolist(), (what, unique)
    assert st.tolist() == want_st.tolist(), (what, unique)
    assert has.tobytes() == old_has.tobytes() and st.tobytes() == old_st.tobytes(), (what, unique)
    assert route["second"] == int((st[:, 1] != hs.NOT_RUN).sum()), route
    return has, st, route


@pytest.mark.parametrize("shape", hi.LDS_SHAPES)
def test_the_lds_route_runs_the_walk_twice(ctx, shape):
    count = 64
    arrays = hs.small_arrays(shape, count)
    want = hi.answers(("small", shape), arrays, count)
    assert len({w[:2] for w in want}) >= 2, want
    assert any(w[2] >= 1 and w[3] == 0 for w in want) and any(w[2] == 0 for w in want)    # minm decides; maxm decides
    for unique in (False, True):
        has, st, route = _check(ctx, arrays, want, unique, shape)
        assert (route["lds"], route["hbm"], route["host"]) == (count, 0, 0) and route["grid"] == route["grid2"] == count, route
        assert route["second"] > 0
        assert len(set(has.tolist())) >= 2


def test_systems_that_end_negative_pass_through_and_close(ctx):
    """(9, 2, 4, 0): more inequality rows than columns -- most systems end -7 at maxm's root (lpsol.h:1232); the marks keep them
    out of the second pass, and the few decided ones around them get their answers."""
    count = 64
    arrays = hs.small_arrays(hi.NEGATIVE_SHAPE, count)
    want = hi.answers(("small", hi.NEGATIVE_SHAPE), arrays, count)
    assert sum(1 for w in want if w[2] == XPG_ERR_REF_UNDEFINED) >= 8 and any(w[2] >= 0 for w in want), want
    for unique in (False, True):
        has, st, route = _check(ctx, arrays, want, unique, hi.NEGATIVE_SHAPE)
        assert (route["lds"], route["hbm"], route["host"]) == (count, 0, 0), route
        neg = np.array([w[2] < 0 for w in want])
        assert (has[neg] == XPG_ERR_REF_UNDEFINED).all() and (st[neg, 0] == XPG_ERR_REF_UNDEFINED).all() and (st[neg, 1] == hs.NOT_RUN).all()


@pytest.mark.parametrize("name", ["wide", "wide_eq"])
def test_the_device_memory_route_answers_a_system_in_one_workgroup(ctx, name):
    arrays = hi.wide_hs() if name == "wide" else hi.wide_hs_eq()
    want = hi.answers((name,), arrays, hi.WIDE_COUNT)
    # what the fixtures hold, asserted of the checker so that a changed generator cannot empty the comparisons: every system
    # decided (the cap on undecided ones is 0), walks that end 0, 1 and 2 in maxm and in minm, verdicts that differ
    assert all(w[0] >= 0 and w[1] >= 0 and w[2] >= 0 and (w[3] is None or w[3] >= 0) for w in want), want
    assert {w[2] for w in want} == {0, 1, 2} and {w[3] for w in want if w[3] is not None} >= ({0, 1, 2} if name == "wide" else {0, 1})
    for k in (0, 1):
        assert len({w[k] for w in want}) == 2, want
    seconds = []
    for unique in (False, True):
        has, st, route = _check(ctx, arrays, want, unique, name)
        assert (route["lds"], route["hbm"], route["host"]) == (0, hi.WIDE_COUNT, 0) and route["grid"] == hi.WIDE_COUNT and route["grid2"] == 0, route
        seconds.append(route["second"])
    assert 0 < seconds[0] < seconds[1] < hi.WIDE_COUNT           # is_unique_sol sends more systems into the second walk


def _reuse_batches():
    """[(name, arrays, the checker's answers per system)] of 32 systems each: WIDE_HS rotated between rounds of two; WIDE_HS_EQ
    the same with a negative-ending system in places 2 and 7 of every eight (both workgroups of a grid of 2 meet them)."""
    idx = hi.reuse_pick(32, 2)
    wide = hi.wide_hs()
    want_w = hi.answers(("wide",), wide, hi.WIDE_COUNT)
    out = [("wide", hi.pick(wide, idx), [want_w[i] for i in idx])]
    vc_arr, eq, leq = hi.pick(hi.wide_hs_eq(), idx)
    want_e = hi.answers(("wide_eq",), hi.wide_hs_eq(), hi.WIDE_COUNT)
    neg = hi.wide_negative()
    want_n = hi.answers(("wide_neg",), neg, hi.WIDE_COUNT)
    assert all(w[:3] == (XPG_ERR_REF_UNDEFINED,) * 3 for w in want_n), want_n
    want = [want_e[i] for i in idx]
    for k in range(32):
        if k % 8 in (2, 7):
            eq[k] = neg[1][idx[k]]; leq[k] = neg[2][idx[k]]; want[k] = want_n[idx[k]]
    out.append(("wide_eq+negative", (vc_arr, eq, leq), want))
    return out


def reuse_digest(ctx):
    """One line per (batch, is_unique_sol): the verdicts and statuses, then the route's grid."""
    out = []
    for name, arrays, _ in _reuse_batches():
        for unique in (False, True):
            has, st, route = _new(ctx, arrays, unique)
            assert route["hbm"] == 32, route
            out.append("%s %d %s %s grid=%d" % (name, unique, has.tolist(), st.tolist(), route["grid"]))
    return out


@needs_hooks
def test_a_workgroup_takes_system_after_system(ctx):
    """XPG_HS_GRID=2 (hooks build; read once per process, hence the child): two workgroups take 16 systems each in turn, through
    the slot, the workspace and the LDS block the one before used -- systems that end after maxm, after minm, or negative at
    maxm's root, and the two carves of a system behind each other. The answers are the unforced launch's and the checker's."""
    mine = reuse_digest(ctx)
    for (name, _, want), k in zip(_reuse_batches(), (0, 2)):
        for unique in (False, True):
            want_has, want_st = hi.expected(want, unique)
            assert mine[k + unique] == "%s %d %s %s grid=32" % (name, unique, want_has.tolist(), want_st.tolist()), (name, unique)
    code = ("import sys; sys.path.insert(0, 'tests')\n"
            "import xpoly_amd, test_gpu_has_solution_int as t\n"
            "ctx = xpoly_amd.Context(0)\n"
            "for line in t.reuse_digest(ctx):\n"
            "    print('D', line)\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=hooks_env(XPG_HS_GRID="2"), cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    theirs = [l[2:] for l in r.stdout.splitlines() if l.startswith("D ")]
    assert len(mine) == 4 and [m.rsplit(" grid=", 1)[0] for m in mine] == [t.rsplit(" grid=", 1)[0] for t in theirs]
    assert all(t.endswith("grid=2") for t in theirs)


def test_a_general_vc_keeps_the_host_composition(ctx):
    shape = (4, 1, 4, 0)
    _, eq, leq = hs.small_arrays(shape, 8)
    for vc0 in (gen.to_rat(v) for v in fc.general_vcs(shape[2])):
        for unique in (False, True):
            has, st, route = _new(ctx, (vc0, eq, leq), unique)
            old_has, old_st = _parent(ctx, (vc0, eq, leq), unique)
            assert has.tobytes() == old_has.tobytes() and st.tobytes() == old_st.tobytes()
            assert (route["lds"], route["hbm"], route["host"], route["grid"]) == (0, 0, 8, 0), route
            assert route["second"] == int((st[:, 1] != hs.NOT_RUN).sum())


def _ragged_case():
    """Two shape classes under one vc (cols and vc are the call's): eight rows of every WIDE_HS system -- its first six and its
    last two, where classes 1 and 3 differ; 8 + 20 rows by 36 variables fit the LDS walk -- and WIDE_HS itself."""
    vc_arr, _, leq = hi.wide_hs()
    small = (vc_arr, None, np.ascontiguousarray(leq[:, [0, 1, 2, 3, 4, 5, 48, 49]]))
    return vc_arr, small, hi.wide_hs()


def test_mixed_shapes_come_back_in_the_order_given(ctx, tmp_path):
    from xpoly_amd.six import has_solution_int_plan, has_solution_int_ragged, has_solution_int_last_route
    vc_arr, small, wide = _ragged_case()
    assert has_solution_int_plan(vc_arr, 8, 0, 21, 12)["route"] == hi.ROUTE_LDS and has_solution_int_plan(vc_arr, 50, 0, 21, 12)["route"] == hi.ROUTE_HBM
    n = 12
    want_s = hi.answers(("wide8",), small, n)
    want_w = hi.answers(("wide",), wide, n)
    leqs, want = [], []
    for i in range(n):
        leqs += [small[2][i], wide[2][i]]
        want += [want_s[i], want_w[i]]
    seconds = []
    for unique in (False, True):
        has, st = has_solution_int_ragged(ctx, leqs, None, vc_arr, unique, want_status=True)
        route = has_solution_int_last_route()
        want_has, want_st = hi.expected(want, unique)
        print("ragged u=%d route %s has %s" % (unique, route, has.tolist()))
        assert has.tolist() == want_has.tolist() and st.tolist() == want_st.tolist()
        assert (route["lds"], route["hbm"], route["host"]) == (n, n, 0) and route["second"] == int((st[:, 1] != hs.NOT_RUN).sum()), route
        seconds.append(route["second"])
    assert len(set(want_has.tolist())) >= 2 and want_has[0::2].tolist() != want_has[1::2].tolist()
    # the C++ collector in a child process: the same systems, is_unique_sol = 1
    from test_has_solution_int_host import build_collector
    exe = build_collector()
    lines = ["20 1 %d" % (2 * n), " ".join(str(int(x)) for x in vc_arr[..., 0].ravel())]
    for m in leqs:
        lines += ["%d 0" % m.shape[0], " ".join(str(int(x)) for x in m[..., 0].ravel()), ""]
    path = str(tmp_path / "systems.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = r.stdout.split()
    assert got[:2] == ["rc", "0"] and got[2] == "route" and [int(x) for x in got[3:7]] == [n, n, 0, seconds[1]]
    assert [int(x) for x in got[7:]] == want_has.tolist()


def test_lifecycle_and_shape_rules(ctx):
    from xpoly_amd._capi import lib, vp
    import ctypes as C
    vc_arr, eq, leq = hs.small_arrays((4, 1, 4, 0), 4)
    has = np.full(4, 55, dtype=np.int32); st = np.full((4, 2), 55, dtype=np.int32)
    call = lambda nb, l, lr, e, er, vc_rows, cols, rhs, h=has: lib().xpg_has_solution_int_batch_rat32(
        ctx._h, C.c_int(nb), vp(l), C.c_int(lr), vp(e), C.c_int(er), vp(vc_arr), C.c_int(vc_rows), C.c_int(cols), C.c_int(rhs), C.c_int(1),
        vp(h), vp(st))
    assert call(4, leq, 4, eq, 1, 4, 5, 3) == XPG_ERR_SHAPE and call(4, leq, 4, eq, 1, 3, 5, 4) == XPG_ERR_SHAPE    # rhs_idx != cols - 1; vc_rows != rhs_idx
    assert call(-1, leq, 4, eq, 1, 4, 5, 4) == XPG_ERR_SHAPE and call(4, leq, -4, eq, 1, 4, 5, 4) == XPG_ERR_SHAPE
    assert call(4, None, 4, eq, 1, 4, 5, 4) == XPG_ERR_SHAPE and call(4, leq, 4, None, 1, 4, 5, 4) == XPG_ERR_SHAPE  # rows without their array
    assert call(4, leq, 4, eq, 1, 4, 5, 4, h=None) == XPG_ERR_SHAPE
    assert (has == 55).all() and (st == 55).all()
    assert call(0, leq, 4, eq, 1, 4, 5, 4) == 0 and (has == 55).all()                           # nb = 0
    assert call(4, None, 0, None, 0, 4, 5, 4) == 0 and (has == 0).all() and (st == hs.NOT_RUN).all()
    assert call(4, None, 0, eq, 1, 4, 5, 4) == 0 and (has == XPG_ERR_REF_UNDEFINED).all()      # the reference sizes tgtf from leq
    assert st[:, 0].tolist() == [XPG_ERR_REF_UNDEFINED] * 4 and (st[:, 1] == hs.NOT_RUN).all()
    # out_status may be NULL
    assert lib().xpg_has_solution_int_batch_rat32(ctx._h, C.c_int(4), vp(leq), C.c_int(4), vp(eq), C.c_int(1), vp(vc_arr), C.c_int(4), C.c_int(5),
                                                  C.c_int(4), C.c_int(1), vp(has), None) == 0
    want = hi.answers(("small", (4, 1, 4, 0)), hs.small_arrays((4, 1, 4, 0), 64), 4)
    assert has.tolist() == [w[1] for w in want]
    # xpg_trim between calls on both routes: the slots and the parked blocks go back, the next call takes new ones
    wide = hi.wide_hs()
    want_w = hi.answers(("wide",), wide, hi.WIDE_COUNT)
    for arrays, w in (((vc_arr, eq, leq), want), (wide, want_w)):
        first = _new(ctx, arrays, True)
        ctx.trim()
        again = _new(ctx, arrays, True)
        assert again[0].tolist() == [x[1] for x in w] and again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
