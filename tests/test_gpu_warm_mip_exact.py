"""GPU: the warm-started branch and bound (xpg_mip_warm_batch_f64, xpg_mip_warm_f64) against exact references, at every
launch geometry. tests/test_gpu_warm_mip.py holds it against scipy's HiGHS on one family (positive A and c); here the data
make the pivot rules matter -- zeros, negative entries, zero and negative right-hand sides, duplicate rows and columns, both
senses -- and every end state, the shape edges of the LDS block, a workgroup that takes several trees and a batch that is
split into several launches are run.

The references are exact (tests/warm_mip_ref.py: enumeration of the integer box, or a branch and bound on Fractions under
Bland's rule); tests/test_warm_mip_host.py holds the two against each other on the CPU, and asserts the condition under which
a case is kept: exact_bb's deepest path is at most half of the depth_cap of the launch, so that no tree outside `deep`'s
large U may end XPG_ERR_UNSUPPORTED. The returned point is checked in integer arithmetic: rounded (it lies within the
kernel's own int_tol = 1e-6 of an integer point), it satisfies A x <= b, x >= 0 exactly and c . x is the exact optimum."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import warm_mip_cases as wc
from conftest import hooks_env, needs_hooks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SUCC, UNBOUND, NO_SOL, UNSUPPORTED, ERR_SHAPE = 0, 1, 2, -4, -3
FILL = -7.25                                                 # what the output arrays hold before a call


def raw_batch(ctx, is_max, tg, leq, is_bin, nb=None, rows=None, cols=None, null=()):
    """xpg_mip_warm_batch_f64 itself, on output arrays that are filled beforehand: (rc, status, v, sol, stats)."""
    from xpoly_amd._capi import lib, vp
    n, r, c = leq.shape
    nb, rows, cols = n if nb is None else nb, r if rows is None else rows, c if cols is None else cols
    st = np.full(max(n, 1), 99, dtype=np.int32); v = np.full(max(n, 1), FILL); sol = np.full((max(n, 1), c), FILL)
    stats = (C.c_longlong * 4)(-1, -1, -1, -1)
    arg = dict(tg=vp(np.ascontiguousarray(tg)), leq=vp(np.ascontiguousarray(leq)), st=vp(st), v=vp(v), sol=vp(sol))
    for name in null:
        arg[name] = None
    rc = lib().xpg_mip_warm_batch_f64(None if "ctx" in null else ctx._h, C.c_int(nb), C.c_int(int(is_max)), arg["tg"], arg["leq"], C.c_int(rows),
                                      C.c_int(cols), C.c_int(int(is_bin)), arg["st"], arg["v"], arg["sol"], stats)
    return rc, st, v, sol, dict(nodes=stats[0], dual_pivots=stats[1], root_pivots=stats[2], max_depth=stats[3])


def batch(ctx, cases, is_max):
    tg, leq = wc.arrays(cases)
    rc, st, v, sol, stats = raw_batch(ctx, is_max, tg, leq, cases[0].is_bin)
    assert rc == 0, rc
    return st, v, sol, stats


def raw_single(ctx, case, is_max):
    from xpoly_amd._capi import lib, vp
    tg, leq = wc.arrays([case])
    v = C.c_double(FILL); sol = np.full(leq.shape[2], FILL); stats = (C.c_longlong * 4)()
    rc = lib().xpg_mip_warm_f64(ctx._h, C.c_int(int(is_max)), vp(tg[0]), vp(leq[0]), C.c_int(leq.shape[1]), C.c_int(leq.shape[2]),
                                C.c_int(case.is_bin), C.byref(v), vp(sol), stats)
    return rc, v.value, sol, dict(nodes=stats[0], dual_pivots=stats[1], root_pivots=stats[2], max_depth=stats[3])


def check_tree(case, is_max, st, v, sol):
    """One tree's status, value and point against the exact answer; no tolerance on the mathematics."""
    w = wc.want(case, is_max)
    n0 = len(case.c)
    print("%-24s %s: status %d (want %d, %s), v %r (want %s), deepest reference path %d" % (case.name, "max" if is_max else "min", st, w.status, w.by, v, w.optimum, w.deepest))
    assert st == w.status, (case.name, is_max, st, w)
    if w.status != SUCC:
        assert v == 0.0 and (sol == FILL).all(), (case.name, is_max, v, sol)          # the row is left as it was passed in
        return
    x = sol[:n0]
    assert np.abs(x - np.round(x)).max() <= 1e-6, (case.name, is_max, x)
    xi = [int(t) for t in np.round(x)]
    assert all(t >= 0 for t in xi) and (not case.is_bin or all(t <= 1 for t in xi)), (case.name, is_max, xi)
    for row, bi in zip(case.A, case.b):
        assert sum(a * t for a, t in zip(row, xi)) <= bi, (case.name, is_max, xi, row, bi)
    assert sum(cj * t for cj, t in zip(case.c, xi)) == w.optimum, (case.name, is_max, xi, w)
    assert abs(v - float(w.optimum)) <= 1e-7 * max(1.0, abs(float(w.optimum))), (case.name, is_max, v, w)
    assert sol[n0] == 1.0


def check_batch(ctx, cases, is_max):
    st, v, sol, stats = batch(ctx, cases, is_max)
    for i, k in enumerate(cases):
        check_tree(k, is_max, int(st[i]), float(v[i]), sol[i])
    roots = sum(wc.want(k, is_max).root == "optimal" for k in cases)
    cap = wc.depth_cap(cases[0])
    print("stats", stats, "depth_cap", cap)
    assert stats["nodes"] >= roots and stats["max_depth"] <= cap, (stats, roots, cap)
    if roots == 0:
        assert stats["nodes"] == 0 and stats["dual_pivots"] == 0, stats
    return st, v, sol, stats


def check_single(ctx, case, is_max, st_b, v_b):
    """The one-tree form on the same case: the exact answer again, and the batch's status and value."""
    rc, v, sol, stats = raw_single(ctx, case, is_max)
    check_tree(case, is_max, rc, v, sol)
    assert rc == st_b and abs(v - v_b) <= 1e-7 * max(1.0, abs(v_b)), (case.name, is_max, rc, st_b, v, v_b)
    return stats


def groups():
    g = [("mixed-%d-%d-%d" % s, wc.memo(wc.mixed, *s, 8), (True, False)) for s in wc.MIXED_SHAPES]
    g.append(("integral_root", wc.integral_root(5, 4, 8), (True, False)))
    g.append(("unbounded", wc.unbounded(3, 3), (True, False)))
    g.append(("root_infeasible", wc.root_infeasible(3, 4), (True, False)))
    g.append(("wide", wc.memo(wc.wide, wc.wide_n0()), (True,)))
    edge = wc.memo(wc.lds_edge, wc.lds_edge_n0())
    g.append(("lds_edge", (edge * 3)[:8], (True,)))
    g.append(("tall", [wc.tall(wc.refusal_rows())] * 2, (True, False)))
    return g


def end_states():
    """Every end state in one batch of two variables and four rows."""
    m = wc.memo(wc.mixed, 2, 2, 0, 8, 4)
    return [m[0], wc.unbounded(2, 4)[0], m[1], wc.root_infeasible(2, 4)[0], wc.deep(wc.DEEP_SMALL_U), m[2], wc.unbounded(2, 4)[1],
            wc.root_infeasible(2, 4)[1], wc.integral_root(2, 4, 2)[0], m[3], wc.integral_root(2, 4, 2)[1], wc.TRIVIAL]


GROUPS = ("mixed-1-2-0", "mixed-2-1-0", "mixed-3-2-1", "mixed-5-4-0", "mixed-6-3-1", "mixed-6-4-0", "integral_root", "unbounded", "root_infeasible", "wide",
          "lds_edge", "tall")


@pytest.mark.parametrize("name", GROUPS)
def test_every_family_reaches_the_exact_answer(ctx, name):
    """The batch form on every case of the family, the one-tree form on a sample of it, in the senses the family runs in."""
    assert tuple(g[0] for g in groups()) == GROUPS
    _, cases, senses = [g for g in groups() if g[0] == name][0]
    for is_max in senses:
        st, v, sol, stats = check_batch(ctx, cases, is_max)
        if name == "integral_root":
            assert stats["nodes"] == len(cases) and stats["dual_pivots"] == 0, stats
        sample = range(0, len(cases), 7 if name == "lds_edge" else 3)
        for i in sample:
            one = check_single(ctx, cases[i], is_max, int(st[i]), float(v[i]))
            if name == "integral_root":
                assert one["nodes"] == 1 and one["dual_pivots"] == 0, one
    if name == "unbounded":                                                # a batch that holds only trees that end at the root
        st, v, sol, stats = batch(ctx, cases, True)
        assert (st == UNBOUND).all() and stats["nodes"] == 0 and stats["dual_pivots"] == 0, (st, stats)
    if name == "root_infeasible":
        for is_max in (True, False):
            st, v, sol, stats = batch(ctx, [cases[0]] * 3, is_max)
            assert (st == NO_SOL).all() and stats["nodes"] == 0 and stats["dual_pivots"] == 0, (st, stats)
    if name == "wide":
        g = wc.geometry(2, wc.wide_n0() + 1, 0)
        assert g["wcap"] > 256 and g["depth_cap"] >= 12, g


def test_a_batch_of_every_end_state(ctx):
    cases = end_states()
    seen = set()
    for is_max in (True, False):
        st, v, sol, stats = check_batch(ctx, cases, is_max)
        seen |= set(int(s) for s in st)
        for i in range(len(cases)):
            check_single(ctx, cases[i], is_max, int(st[i]), float(v[i]))
    assert seen == {SUCC, UNBOUND, NO_SOL}, seen


def _cycled(nb):
    base = wc.memo(wc.mixed, *wc.CYCLE_SHAPE, 64)
    return [base[i % 64] for i in range(nb)]


def test_launch_geometry(ctx):
    """nb = 1, 2, 3, 65 and 257 of the 64-problem mixed set, cycled: problem i is problem i mod 64 of the 64-tree call, in
    the bytes of status, v and sol; the 64-tree call itself is held against the exact answers."""
    for is_max in (True, False):
        st0, v0, sol0, stats0 = check_batch(ctx, _cycled(64), is_max)
        assert (st0 != UNSUPPORTED).all()
        for nb in (1, 2, 3, 65, 257):
            st, v, sol, stats = batch(ctx, _cycled(nb), is_max)
            idx = np.arange(nb) % 64
            assert np.array_equal(st, st0[idx]) and v.tobytes() == v0[idx].tobytes() and sol.tobytes() == sol0[idx].tobytes(), (is_max, nb)
            assert stats["nodes"] >= (st == SUCC).sum() and stats["nodes"] >= 1 and stats["max_depth"] <= stats0["max_depth"], (nb, stats)
            if nb >= 64:
                assert stats["max_depth"] == stats0["max_depth"], (nb, stats, stats0)
        for i in range(0, 64, 7):
            check_single(ctx, _cycled(64)[i], is_max, int(st0[i]), float(v0[i]))


def test_a_tree_beyond_the_depth_fails_alone(ctx):
    """deep's large U between ordinary problems: XPG_ERR_UNSUPPORTED in its own status only, v = 0, its sol row untouched --
    and its neighbours' bytes are those of the same batch with a trivial tree in its place. The one-tree form refuses it too."""
    m = wc.memo(wc.mixed, 2, 2, 0, 8, 4)
    large, small = wc.deep(wc.DEEP_LARGE_U), wc.deep(wc.DEEP_SMALL_U)
    for is_max in (True, False):
        with_deep = m[:3] + [large] + m[3:6] + [small] + m[6:]
        plain = m[:3] + [wc.TRIVIAL] + m[3:6] + [small] + m[6:]
        st, v, sol, stats = batch(ctx, with_deep, is_max)
        st1, v1, sol1, _ = check_batch(ctx, plain, is_max)
        assert st[3] == UNSUPPORTED and v[3] == 0.0 and (sol[3] == FILL).all(), (st, v[3], sol[3])
        assert st[7] == NO_SOL and stats["max_depth"] <= 12
        keep = [i for i in range(len(plain)) if i != 3]
        assert st[keep].tobytes() == st1[keep].tobytes() and v[keep].tobytes() == v1[keep].tobytes() and sol[keep].tobytes() == sol1[keep].tobytes()
        rc, v_one, sol_one, _ = raw_single(ctx, large, is_max)
        assert rc == UNSUPPORTED and v_one == 0.0 and (sol_one == FILL).all(), (rc, v_one)
        rc, v_one, sol_one, _ = raw_single(ctx, small, is_max)
        assert rc == NO_SOL and v_one == 0.0


def test_the_first_shape_past_64_kb_is_refused_whole(ctx):
    k = wc.tall(wc.refusal_rows() + 1)
    tg, leq = wc.arrays([k, k])
    rc, st, v, sol, stats = raw_batch(ctx, True, tg, leq, 0)
    assert rc == UNSUPPORTED and (st == 99).all() and (v == FILL).all() and (sol == FILL).all() and stats["nodes"] == -1


def test_argument_paths(ctx):
    tg, leq = wc.arrays(_cycled(2))
    rc, st, v, sol, stats = raw_batch(ctx, True, tg, leq, 0, nb=0)
    assert rc == 0 and (st == 99).all() and (v == FILL).all() and (sol == FILL).all() and stats["nodes"] == -1
    for kw in (dict(nb=-1), dict(rows=0), dict(rows=-2), dict(cols=1), dict(null=("tg",)), dict(null=("leq",)), dict(null=("st",)), dict(null=("v",)),
               dict(null=("sol",)), dict(null=("ctx",))):
        rc, st, v, sol, stats = raw_batch(ctx, True, tg, leq, 0, **kw)
        assert rc == ERR_SHAPE and (st == 99).all() and (v == FILL).all() and (sol == FILL).all(), (kw, rc)
    from xpoly_amd._capi import lib, vp
    out_v = C.c_double(FILL)
    one = lambda tgp, leqp, rows, cols, vp_: lib().xpg_mip_warm_f64(ctx._h, C.c_int(1), tgp, leqp, C.c_int(rows), C.c_int(cols), C.c_int(0), vp_, None, None)
    assert one(None, vp(leq[0]), 3, 5, C.byref(out_v)) == ERR_SHAPE and one(vp(tg[0]), None, 3, 5, C.byref(out_v)) == ERR_SHAPE
    assert one(vp(tg[0]), vp(leq[0]), 0, 5, C.byref(out_v)) == ERR_SHAPE and one(vp(tg[0]), vp(leq[0]), 3, 1, C.byref(out_v)) == ERR_SHAPE
    assert one(vp(tg[0]), vp(leq[0]), 3, 5, None) == ERR_SHAPE and out_v.value == FILL
    assert one(vp(tg[0]), vp(leq[0]), 3, 5, C.byref(out_v)) == wc.want(_cycled(1)[0], True).status           # sol and stats may be NULL


# ---- the hooks build: a workgroup that takes several trees, a batch split into several launches ----

def strided_cases():
    """37 0-1 trees of six variables, ordered for a grid of two workgroups (workgroup w takes trees w, w + 2, ...): each
    takes a deep tree, then a shallow one, then one whose root is infeasible, again and again."""
    pool = sorted(wc.memo(wc.mixed, 6, 3, 1, 24), key=lambda k: -max(wc.want(k, True).deepest, wc.want(k, False).deepest))
    deep_ones, shallow_ones = pool[:8], pool[-8:]
    inf = wc.root_infeasible(6, 9)[0]._replace(is_bin=1, name="phase-one-6-9-bin")
    out = []
    for i in range(0, 8, 2):
        out += [deep_ones[i], deep_ones[i + 1], shallow_ones[i], shallow_ones[i + 1], inf, inf]
    out += out[:13]
    assert len(out) == 37
    return out


def digest(st, v, sol):
    return hashlib.sha256(st.tobytes() + v.tobytes() + sol.tobytes()).hexdigest()


def grid_digest(ctx):
    return ["%d %s" % (is_max, digest(*batch(ctx, strided_cases(), is_max)[:3])) for is_max in (True, False)]


def chunk_report(ctx):
    out = []
    for nb in (200, 201):
        for is_max in (True, False):
            st, v, sol, stats = batch(ctx, _cycled(nb), is_max)
            out.append([nb, int(is_max), digest(st, v, sol), stats])
    return out


def _child(fn_name, **env):
    code = ("import json, sys; sys.path.insert(0, 'tests')\n"
            "import xpoly_amd, test_gpu_warm_mip_exact as t\n"
            "ctx = xpoly_amd.Context(0)\n"
            "print('D', json.dumps(t.%s(ctx)))\n" % fn_name)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=hooks_env(**env), cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("D ")][0][2:])


@needs_hooks
def test_a_capped_grid_walks_the_batch_in_strides(ctx):
    """XPG_WARM_BATCH_GRID=2 (hooks build, in a child process): two workgroups take 37 trees in turn, each through the LDS
    block and the workspace slot that the tree before it left behind -- the bytes are those of the uncapped launch, which
    are held against the exact answers here."""
    cases = strided_cases()
    deepest = [max(wc.want(k, s).deepest for s in (True, False)) for k in cases]
    assert deepest[0] >= 3 and deepest[2] <= 1 and wc.want(cases[4], True).root == "infeasible", deepest
    for is_max in (True, False):
        check_batch(ctx, cases, is_max)
    mine = grid_digest(ctx)
    assert _child("grid_digest", XPG_WARM_BATCH_GRID="2") == mine and len(mine) == 2


@needs_hooks
def test_a_batch_split_into_several_launches(ctx):
    """XPG_WARM_BATCH_WS_CAP (hooks build, in a child process) at 70 trees' worth of workspace: 200 trees go in four launches
    of 50, 201 in three of 51 and a short one of 48 (the halving rule of the launch loop cannot leave 200 a short chunk) --
    status, v and sol are the bytes of the unsplit call, nodes and pivots its sums, max_depth its maximum."""
    k = _cycled(1)[0]
    rows, cols = len(k.A), len(k.c) + 1                                                # the shape that is launched
    per_tree = wc.geometry(rows, cols, 0)["tree_stride"] * 8
    assert wc.geometry(rows, cols, 0, 201)["launches"] == 1                            # this process runs without the bound
    mine = chunk_report(ctx)
    theirs = _child("chunk_report", XPG_WARM_BATCH_WS_CAP=str(70 * per_tree))
    assert theirs == json.loads(json.dumps(mine)), (theirs, mine)
    code = ("import json, sys; sys.path.insert(0, 'tests')\nimport warm_mip_cases as wc\n"
            "print('G', json.dumps([wc.geometry(%d, %d, 0, nb) for nb in (200, 201)]))\n" % (rows, cols))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=hooks_env(XPG_WARM_BATCH_WS_CAP=str(70 * per_tree)), cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    g = json.loads([l for l in r.stdout.splitlines() if l.startswith("G ")][0][2:])
    assert [(x["chunk"], x["launches"]) for x in g] == [(50, 4), (51, 4)], g
