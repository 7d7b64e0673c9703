"""Lineq::has_solution for systems of MIXED shapes under one vc in one call (xpg_has_solution_batch_ragged_rat32): every system on
the route a uniform call of its shape takes, the systems of a route in ONE launch over an index list, sized by the largest of
their own plans.

Checker (tests/has_solution_cases.py): the CPU restatement, under the cache keys tests/test_gpu_has_solution_batch.py uses, so a
shape both files test is computed once. Every comparison is exact: the verdict and both statuses, and array for array the
answers of uniform xpg_has_solution_batch_rat32 calls on the same systems."""
import subprocess
import sys

import numpy as np
import pytest

import free_var_cases as fc
import has_solution_cases as hs
import six_vc_hbm_cases as vc
from conftest import ROOT, hooks_env, needs_hooks
from tools import gen

pytestmark = pytest.mark.gpu
XPG_ERR_REF_UNDEFINED = -7
NO_ROUTE = dict(lds=0, hbm=0, host=0, second=0, grid_lds=0, grid_hbm=0, no_solve=0)

LDS_MIX = tuple((m, me, 5, 1) for m, me in ((5, 2), (2, 1), (8, 0), (3, 3), (11, 2)))      # 64 threads each; (11, 2): more rows than columns
THREAD_MIX = (((4, 1, 20, 1), 6), ((20, 2, 20, 1), 6), ((20, 12, 20, 1), 4))               # 64, 128 and 256 threads
HBM_MIX = (("pairs", vc.FIRST), ("pairs", vc.ODD), ("fold", vc.FOLD_SHAPES[0]), ("fold", vc.FOLD_SHAPES[1]))


def _ragged(ctx, systems, vc_arr, unique, max_iter=hs.NO_LIMIT, is_int=False):
    """systems: [(leq_b, eq_b or None)]. Returns (has, status, route)."""
    from xpoly_amd.six import has_solution_ragged, has_solution_ragged_last_route
    has, st = has_solution_ragged(ctx, [s[0] for s in systems], [s[1] for s in systems], vc_arr, is_int, unique, max_iter=max_iter, want_status=True)
    return has, st, has_solution_ragged_last_route()


def _uniform(ctx, arrays, unique, max_iter=hs.NO_LIMIT):
    from xpoly_amd.six import has_solution_batch
    vc_arr, eq, leq = arrays
    return has_solution_batch(ctx, leq, eq, vc_arr, False, unique, max_iter=max_iter, want_status=True)


def _interleave(groups):
    """groups: [(arrays, count)] -> the systems system 0 of every group, system 1 of every group, ... and for each its
    (group, index)."""
    systems, where = [], []
    for i in range(max(n for _, n in groups)):
        for g, ((_, eq, leq), n) in enumerate(groups):
            if i < n:
                systems.append((leq[i], None if eq is None else eq[i]))
                where.append((g, i))
    return systems, where


def _expect(wants, where, unique):
    """(has, status) the call must return: hs.expected of every group's checker answers, gathered in the systems' order."""
    per = [hs.expected(w, unique) for w in wants]
    return (np.array([per[g][0][i] for g, i in where], dtype=np.int32), np.array([per[g][1][i] for g, i in where], dtype=np.int32))


def _lds_mix():
    groups = [(hs.small_arrays(s, 16), 16) for s in LDS_MIX]
    return groups, groups[0][0][0]


def _hbm_mix():
    groups = [(hs.hbm_arrays(f, s, True), hs.HBM_COUNT) for f, s in HBM_MIX]
    return groups, groups[0][0][0]


def test_an_lds_mix_under_one_vc(ctx):
    groups, vc_arr = _lds_mix()
    for (a, _), s in zip(groups, LDS_MIX):
        assert a[0].tobytes() == vc_arr.tobytes(), s                                 # one vc
    wants = [hs.oracle_answers(("small", s), a, n) for s, (a, n) in zip(LDS_MIX, groups)]
    systems, where = _interleave(groups)
    flat = [w for ws in wants for w in ws]
    assert any(w[2] == 0 for w in flat)                                              # maxm decides
    assert any(w[2] >= 2 and w[3] == 0 for w in flat)                                # minm decides
    assert any((w[2], w[3]) == (1, 2) and w[0] == 1 and w[1] == 0 for w in flat)     # the verdict flips with is_unique_sol
    assert any(w[0] == 0 and w[1] == 0 for w in flat)
    assert any(w[0] == -7 and w[2] == -7 for w in flat)
    for unique in (False, True):
        has, st, route = _ragged(ctx, systems, vc_arr, unique)
        want_has, want_st = _expect(wants, where, unique)
        print("u=%d has %s" % (unique, has.tolist()))
        assert has.tolist() == want_has.tolist() and st.tolist() == want_st.tolist(), (unique, has.tolist(), want_has.tolist())
        second = int((want_st[:, 1] != hs.NOT_RUN).sum())
        assert route == dict(NO_ROUTE, lds=80, second=second, grid_lds=80), route    # one launch, nothing else
        for g, (a, _) in enumerate(groups):                                          # array for array the five uniform calls
            uh, us = _uniform(ctx, a, unique)
            pick = [k for k, (gg, _) in enumerate(where) if gg == g]
            assert has[pick].tobytes() == uh.tobytes() and st[pick].tobytes() == us.tobytes(), (unique, LDS_MIX[g])


def test_thread_counts_mixed_in_one_launch(ctx):
    from xpoly_amd.six import has_solution_batch_plan, has_solution_ragged_plan
    groups = [(hs.small_arrays(s, n), n) for s, n in THREAD_MIX]
    vc_arr = groups[0][0][0]
    assert [has_solution_batch_plan(vc_arr, s[0], s[1], 21, n)["threads"] for s, n in THREAD_MIX] == [64, 128, 256]
    systems, where = _interleave(groups)
    route_of, sizes = has_solution_ragged_plan(vc_arr, [len(l) for l, _ in systems], [len(e) for _, e in systems])
    assert route_of.tolist() == [hs.ROUTE_LDS] * 16 and sizes["lds_threads"] == 256 and sizes["lds_count"] == 16
    wants = [hs.oracle_answers(("small", s), a, n) for (s, _), (a, n) in zip(THREAD_MIX, groups)]
    for unique in (False, True):
        has, st, route = _ragged(ctx, systems, vc_arr, unique)
        want_has, want_st = _expect(wants, where, unique)
        assert has.tolist() == want_has.tolist() and st.tolist() == want_st.tolist(), (unique, has.tolist(), want_has.tolist())
        assert route["lds"] == 16 and route["hbm"] == 0 and route["host"] == 0 and route["grid_lds"] == 16, route


def test_a_device_memory_mix(ctx):
    groups, vc_arr = _hbm_mix()
    wants = [hs.oracle_answers((f, s, True), a, n, hs.HBM_CAP) for (f, s), (a, n) in zip(HBM_MIX, groups)]
    systems, where = _interleave(groups)
    for unique in (False, True):
        has, st, route = _ragged(ctx, systems, vc_arr, unique, hs.HBM_CAP)
        want_has, want_st = _expect(wants, where, unique)
        print("u=%d has %s" % (unique, has.tolist()))
        assert has.tolist() == want_has.tolist() and st.tolist() == want_st.tolist(), (unique, has.tolist(), want_has.tolist())
        n = 4 * hs.HBM_COUNT
        assert route == dict(NO_ROUTE, hbm=n, second=int((want_st[:, 1] != hs.NOT_RUN).sum()), grid_hbm=n), route


def test_both_routes_in_one_call(ctx):
    """The first 5 inequalities and the first equality of the FIRST systems are systems of the LDS-resident kernel; whole
    FIRST systems are the device-memory kernel's. Interleaved they are one call, two launches, and the answers of the two
    uniform calls."""
    vc_arr, eq, leq = hs.hbm_arrays("pairs", vc.FIRST, True)
    cut = (vc_arr, np.ascontiguousarray(eq[:, :1]), np.ascontiguousarray(leq[:, :5]))
    n = hs.HBM_COUNT
    systems, where = _interleave([(cut, n), ((vc_arr, eq, leq), n)])
    for unique in (False, True):
        has, st, route = _ragged(ctx, systems, vc_arr, unique, hs.HBM_CAP)
        assert route["lds"] == n and route["hbm"] == n and route["host"] == 0 and route["grid_lds"] == n and route["grid_hbm"] == n, route
        for g, arrays in enumerate((cut, (vc_arr, eq, leq))):
            uh, us = _uniform(ctx, arrays, unique, hs.HBM_CAP)
            pick = [k for k, (gg, _) in enumerate(where) if gg == g]
            assert has[pick].tobytes() == uh.tobytes() and st[pick].tobytes() == us.tobytes(), (unique, g, has[pick].tolist(), uh.tolist())
    assert len(set(has[::2].tolist())) >= 2 or len(set(has[1::2].tolist())) >= 2, has.tolist()


def stride_digest(ctx):
    """One line per call: the verdicts and statuses of the LDS mix and of the device-memory mix, both values of is_unique_sol;
    and the grids of the launches."""
    out = []
    for name, (groups, vc_arr), cap in (("lds", _lds_mix(), hs.NO_LIMIT), ("hbm", _hbm_mix(), hs.HBM_CAP)):
        systems, _ = _interleave(groups)
        for unique in (False, True):
            has, st, route = _ragged(ctx, systems, vc_arr, unique, cap)
            out.append("%s %d %s %s grid=%d,%d" % (name, unique, has.tolist(), st.tolist(), route["grid_lds"], route["grid_hbm"]))
    return out


@needs_hooks
def test_a_capped_grid_walks_systems_of_different_layouts_through_one_slot(ctx):
    """XPG_HS_GRID=2 (hooks build; read once per process, hence the children): two workgroups take 80 and 32 systems in turn,
    each through the slot, LDS block and hdr the system before used under ANOTHER layout. Sorted, a workgroup goes from large
    systems to small ones (and to and fro between shapes of equal weight); with the index lists in arrival order
    (XPG_HS_RAGGED_ARRIVAL=1) it goes both ways. The answers are those of the uncapped call."""
    mine = stride_digest(ctx)
    assert [m.rsplit("=", 1)[1] for m in mine] == ["80,0", "80,0", "0,32", "0,32"]
    code = ("import sys; sys.path.insert(0, 'tests')\n"
            "import xpoly_amd, test_gpu_has_solution_ragged as t\n"
            "ctx = xpoly_amd.Context(0)\n"
            "for line in t.stride_digest(ctx):\n"
            "    print('D', line)\n")
    for extra in ({}, {"XPG_HS_RAGGED_ARRIVAL": "1"}):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=hooks_env(XPG_HS_GRID="2", **extra), cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        theirs = [l[2:] for l in r.stdout.splitlines() if l.startswith("D ")]
        assert len(mine) == 4 and [m.rsplit(" grid=", 1)[0] for m in mine] == [t.rsplit(" grid=", 1)[0] for t in theirs], extra
        assert [t.rsplit("=", 1)[1] for t in theirs] == ["2,0", "2,0", "0,2", "0,2"], theirs


def test_order_and_edges(ctx):
    from xpoly_amd.six import has_solution
    groups = [(hs.small_arrays(s, 4), 4) for s in LDS_MIX]
    vc_arr = groups[0][0][0]
    systems, _ = _interleave(groups)
    has, st, _ = _ragged(ctx, systems, vc_arr, True)
    # permuting the systems permutes the answers
    perm = np.random.default_rng(7).permutation(len(systems))
    has2, st2, _ = _ragged(ctx, [systems[k] for k in perm], vc_arr, True)
    assert has2.tolist() == has[perm].tolist() and st2.tolist() == st[perm].tolist()
    # systems without inequalities in the middle: the single call's answers, the neighbours undisturbed
    eq2 = gen.to_rat(np.random.default_rng(31).integers(-3, 4, size=(2, 6)))
    mid = systems[:7] + [(None, None)] + systems[7:12] + [(None, eq2)] + systems[12:]
    has3, st3, route = _ragged(ctx, mid, vc_arr, True)
    keep = [k for k in range(len(mid)) if k not in (7, 13)]
    assert has3[keep].tolist() == has.tolist() and st3[keep].tolist() == st.tolist()
    assert (int(has3[7]), st3[7].tolist()) == (0, [hs.NOT_RUN, hs.NOT_RUN])
    assert (int(has3[13]), st3[13].tolist()) == (XPG_ERR_REF_UNDEFINED, [XPG_ERR_REF_UNDEFINED, hs.NOT_RUN])
    assert [has_solution(ctx, None, None, vc_arr, 5, False, True), has_solution(ctx, None, eq2, vc_arr, 5, False, True)] == [0, XPG_ERR_REF_UNDEFINED]
    assert route["lds"] == 20 and route["no_solve"] == 2 and route["host"] == 0 and route["hbm"] == 0, route
    # a general vc sends every system per system
    for vc0 in (gen.to_rat(v) for v in fc.general_vcs(5)):
        has4, st4, route = _ragged(ctx, systems[:6], vc0, True)
        assert route == dict(NO_ROUTE, host=6), route
        assert has4.tolist() == [has_solution(ctx, l, e, vc0, 5, False, True) for l, e in systems[:6]] and (st4 == hs.NOT_RUN).all()
    # no systems
    has5, st5, route = _ragged(ctx, [], vc_arr, True)
    assert len(has5) == 0 and st5.shape == (0, 2) and route == NO_ROUTE


def test_integer_solutions_go_by_shape_class(ctx):
    shapes, n = ((4, 1, 4, 0), (2, 1, 4, 0)), 16
    groups = [(hs.small_arrays(s, n), n) for s in shapes]
    vc_arr = groups[0][0][0]
    wants = [hs.int_answers(("small", s), a, n) for s, (a, _) in zip(shapes, groups)]
    systems, where = _interleave(groups)
    assert len({w for ws in wants for w in ws}) >= 2, wants
    for k, unique in enumerate((False, True)):
        has, st, route = _ragged(ctx, systems, vc_arr, unique, is_int=True)
        assert has.tolist() == [wants[g][i][k] for g, i in where], (unique, has.tolist())
        assert route["lds"] == 0 and route["hbm"] == 0 and route["host"] == 0 and route["grid_lds"] == 0 and route["grid_hbm"] == 0, route
        assert route["second"] == int((st[:, 1] != hs.NOT_RUN).sum())


def test_the_collector_makes_one_ragged_call(ctx, tmp_path):
    """tests/cxx/has_solution_ragged.cpp in a child process: four shape classes under one vc, interleaved, through
    xpoly_amd::has_solution_all -- the checker's verdicts in the order given, every system on a kernel, at most two launches."""
    from test_has_solution_ragged_host import build_collector
    exe = build_collector()
    shapes = [s for s in LDS_MIX if s[:2] != (3, 3)]
    groups = [(hs.small_arrays(s, 8), 8) for s in shapes]
    wants = [hs.oracle_answers(("small", s), a, n) for s, (a, n) in zip(shapes, groups)]
    systems, where = _interleave(groups)
    ints = lambda a: " ".join(str(int(x)) for x in a[..., 0].ravel())
    lines = ["5 0 1 %d" % len(systems), ints(groups[0][0][0])]
    for leq, eq in systems:
        lines += ["%d %d" % (len(leq), 0 if eq is None else len(eq)), ints(leq), "" if eq is None else ints(eq)]
    path = str(tmp_path / "systems.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = r.stdout.split()
    print(r.stdout)
    assert got[:2] == ["rc", "0"] and got[2] == "route"
    route = [int(x) for x in got[3:10]]
    expect = [wants[g][i][1] for g, i in where]
    assert [int(x) for x in got[10:]] == expect and len(set(expect)) >= 2
    assert route[0] + route[1] == len(systems) and route[2] == 0 and route[6] == 0, route     # no per-system answers
    assert route[0] == len(systems) and route[4] >= 1 and route[5] == 0, route              # one launch here, two at the most
