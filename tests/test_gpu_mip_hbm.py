"""MIP trees whose node LPs are past 64 KB of LDS walked on the device (xpg_mip_batch_vc_hbm_*, k_mip_tree_hbm): one workgroup
per tree, the node tableaux in a slot in device memory, everything else k_mip_tree's walk.

Checkers (tests/mip_hbm_cases.py): the CPU restatement in non-strict mode, and the unchanged host-controller route --
mip_batch_vc on the same arrays, which is where xpg_mip_batch_vc_* sends these shapes (xpg_mip_last_route must say so). Every
comparison is exact: status, the optimum's bits, the solution's bits, the node counts. xpg_mip_hbm_last_route tells the routes
apart, whose answers are the same."""
import ctypes as C

import numpy as np
import pytest

import free_var_cases as fc
import mip_hbm_cases as mc
from free_var_cases import F64, RAT
from tools import gen

pytestmark = pytest.mark.gpu
XPG_ERR_SHAPE = -3


def _fits(kind, leq_rows, eq_rows, cols, is_bin, extra):
    from xpoly_amd._capi import lib
    return lib().xpg_test_mip_fits(C.c_int(kind), C.c_int(leq_rows), C.c_int(eq_rows), C.c_int(cols), C.c_int(int(is_bin)), C.c_int(extra))


def _hbm(ctx, kind, is_max, is_bin, tg, vc, leq, eq=None, ind=None):
    """mip_batch_vc_hbm and the route it took: ((status, v, sol, nodes), route)."""
    from xpoly_amd.six import mip_batch_vc_hbm, mip_hbm_last_route
    got = mip_batch_vc_hbm(ctx, is_max, is_bin, tg, vc, leq, eq=eq, ind=ind, kind=kind)
    return got, mip_hbm_last_route()


def _host(ctx, kind, is_max, is_bin, tg, vc, leq, eq=None, ind=None):
    """The same arrays through mip_batch_vc, which must have taken the host controller for every tree."""
    from xpoly_amd.six import mip_batch_vc, mip_last_route
    got = mip_batch_vc(ctx, is_max, is_bin, tg, vc, leq, eq=eq, rational_indicator=ind, kind=kind)
    r = mip_last_route()
    assert r == dict(device_trees=0, host_trees=len(got[0]), free_vars=0), r
    return got


def _same_bytes(a, b, what):
    assert a[0].tobytes() == b[0].tobytes(), (what, "status", a[0], b[0])
    assert a[1].tobytes() == b[1].tobytes(), (what, "v")
    assert a[2].tobytes() == b[2].tobytes(), (what, "sol")
    assert a[3] == b[3], (what, "nodes", a[3], b[3])


def _against_oracle(got, want, what, skip_undefined=False):
    """Every program against (status, v, sol, nodes) of the oracle; returns the programs compared. The sum of the node counts is
    compared when none was left out."""
    st, v, sol, nodes = got
    compared = 0
    for b, w in enumerate(want):
        if w[0] == -7 and skip_undefined:
            assert st[b] == -7, (what, b, st[b])                 # undefined in the reference: the device says so too
            continue
        assert fc.same_answer(st[b], v[b], sol[b], w), (what, b, st[b], w[:2])
        compared += 1
    if compared == len(want):
        assert nodes == sum(w[3] for w in want), (what, nodes)
    return compared


@pytest.mark.parametrize("is_max", [True, False])
def test_fp64_integer_programs_with_free_variables(ctx, port, is_max):
    """Case 1: fc.wide_lp_f64, 16 programs, the device-memory walk for all; the oracle's answers (none of them -7) and the host
    controller's, node counts included."""
    tg, vc, leq = mc.wide(F64)
    assert leq.shape == (mc.WIDE_COUNT, mc.WIDE_ROWS, mc.WIDE_COLS)
    assert _fits(F64, mc.WIDE_ROWS, 0, mc.WIDE_COLS, False, 0) == 1 and _fits(F64, mc.WIDE_ROWS, 0, mc.WIDE_COLS, False, mc.WIDE_FREE) == 0
    want = mc.wide_oracle(port, F64, is_max)
    assert all(w[0] != -7 for w in want)
    assert len({w[0] for w in want}) >= 2 and max(w[3] for w in want) > 1      # not root LPs alone
    got, route = _hbm(ctx, F64, is_max, False, tg, vc, leq)
    assert route == dict(lds=0, hbm=mc.WIDE_COUNT, host=0, free=mc.WIDE_FREE, grid=mc.WIDE_COUNT), route
    from xpoly_amd.six import mip_last_route
    assert mip_last_route() == dict(device_trees=mc.WIDE_COUNT, host_trees=0, free_vars=mc.WIDE_FREE)
    assert _against_oracle(got, want, ("wide", is_max)) == mc.WIDE_COUNT
    _same_bytes(got, _host(ctx, F64, is_max, False, tg, vc, leq), ("wide", is_max))


@pytest.mark.parametrize("is_max", [True, False])
def test_rational_integer_programs_with_free_variables(ctx, port, is_max):
    """Case 2: the same arrays as Rational (the data is integral). All 16 against the host controller; against the oracle
    all 16 as well: measured on the CPU, the restatement walks every one of these trees in under 0.1 s (16 of 16 per
    direction, well inside the 20 s the comparison may take)."""
    tg, vc, leq = mc.wide(RAT)
    want = mc.wide_oracle(port, RAT, is_max)
    assert len(want) == mc.WIDE_COUNT >= 4 and all(w[0] != -7 for w in want)
    got, route = _hbm(ctx, RAT, is_max, False, tg, vc, leq)
    assert route == dict(lds=0, hbm=mc.WIDE_COUNT, host=0, free=mc.WIDE_FREE, grid=mc.WIDE_COUNT), route
    assert _against_oracle(got, want, ("wide rational", is_max)) == mc.WIDE_COUNT
    _same_bytes(got, _host(ctx, RAT, is_max, False, tg, vc, leq), ("wide rational", is_max))


def _eq_facts(want):
    """What the oracle's answers of the EQ batch must hold for the case to mean anything: at most 25 % of ALL programs left out
    (-7), and among the decided ones at least two statuses and a tree of more than one node (0-1 branching really runs: the
    ancestors' equalities, the pairs of left-over ones, forks)."""
    undefined = [b for b, w in enumerate(want) if w[0] == -7]
    assert len(undefined) <= 0.25 * len(want), len(undefined)
    assert undefined == list(range(0, mc.EQ_COUNT, mc.EQ_RAW_EVERY))          # the raw draws, all of them
    decided = [w for w in want if w[0] != -7]
    assert len({w[0] for w in decided}) >= 2 and max(w[3] for w in decided) > 1, [(w[0], w[3]) for w in decided]


@pytest.mark.parametrize("kind", [F64, RAT])
def test_01_branching_with_equalities_at_the_root(ctx, port, kind):
    """Case 3: 0-1 programs with two root equalities, 12 variables and 52 inequalities, 52 being the smallest m_leq at which
    the LDS walk refuses mip_eq_cases.random_mip_eq(rng, m_leq, 2, 12, True). The reference is undefined at the root of EVERY
    draw of that generator at that size (more than cols dense inequalities: lpsol.h:1232 reads past the equality's row; the
    oracle returns -7 for all of them, both directions, both kinds, seeds 0 .. 7), so only 8 of the 32 programs are such
    draws and 24 are draws of 2 inequalities followed by 50 rows 0.x <= b, on which it is defined (tests/mip_hbm_cases.py EQ;
    seed 9, chosen on the CPU oracle alone: it decides 24 of 24 in both directions and both kinds, each tree in milliseconds,
    and in every one of the four runs some tree branches and two statuses occur). Skipped against the oracle: where it
    returns -7 -- 8 of 32, the cap of 25 % over the whole batch -- and there the device must return -7 too. Every program,
    skipped or not, is compared with the host controller."""
    m_leq = next(m for m in range(1, 200) if _fits(kind, m, mc.EQ_ROWS, mc.EQ_NV + 1, True, 0) == 0)
    assert m_leq == mc.EQ_M_LEQ and _fits(kind, m_leq - 1, mc.EQ_ROWS, mc.EQ_NV + 1, True, 0) == 1
    tg, vc, eq, leq = mc.eq_batch(kind)
    assert leq.shape[:3] == (mc.EQ_COUNT, m_leq, mc.EQ_NV + 1) and eq.shape[1] == mc.EQ_ROWS
    for is_max in (True, False):
        want = mc.eq_oracle(port, kind, is_max)
        _eq_facts(want)
        got, route = _hbm(ctx, kind, is_max, True, tg, vc, leq, eq=eq)
        assert route == dict(lds=0, hbm=mc.EQ_COUNT, host=0, free=0, grid=mc.EQ_COUNT), route
        compared = _against_oracle(got, want, ("eq", kind, is_max), skip_undefined=True)
        assert compared == mc.EQ_COUNT - mc.EQ_COUNT // mc.EQ_RAW_EVERY
        _same_bytes(got, _host(ctx, kind, is_max, True, tg, vc, leq, eq=eq), ("eq", kind, is_max))


@pytest.mark.parametrize("kind", [F64, RAT])
def test_a_tree_that_ends_minus_7_leaves_the_trees_after_it_alone(ctx, port, kind):
    """Case 3, the workgroup's next tree: nb = 2 x grid + 3 trees by tiling case 3's 32 programs, rotated by three from one round
    of the grid to the next. Every workgroup whose first tree is a raw draw -- ended -7 by mip_build_node before any LP --
    walks a decided program next in the same workspace, slot and LDS (and every fourth of the others walks a raw draw
    second); each tree has the answer of its source program: the oracle's, or -7 where that is the oracle's."""
    from xpoly_amd.six import mip_hbm_plan
    tg, vc, eq, leq = mc.eq_batch(kind)
    grid = mip_hbm_plan(kind, vc, mc.EQ_M_LEQ, mc.EQ_ROWS, mc.EQ_NV + 1, True, True, 1 << 20)["grid"]
    nb = 2 * grid + 3
    assert grid % mc.EQ_COUNT == 0
    pick = mc.reuse_pick(nb, grid, mc.EQ_COUNT, 3)
    after_raw = [int(pick[g + grid]) for g in range(grid) if pick[g] % mc.EQ_RAW_EVERY == 0]
    assert len(after_raw) == grid // mc.EQ_RAW_EVERY and all(b % mc.EQ_RAW_EVERY == 3 for b in after_raw)
    for is_max in (True, False):
        want = mc.eq_oracle(port, kind, is_max)
        _eq_facts(want)
        assert len({(want[b][0], want[b][3]) for b in after_raw}) >= 2          # the trees behind a -7 one are not all alike
        arrs = [np.ascontiguousarray(a[pick]) for a in (tg, leq, eq)]
        got, route = _hbm(ctx, kind, is_max, True, arrs[0], vc, arrs[1], eq=arrs[2])
        assert route["hbm"] == nb and nb >= 2 * route["grid"] + 3, route
        compared = _against_oracle(got, [want[i] for i in pick], ("eq reuse", kind, is_max), skip_undefined=True)
        assert compared == sum(int(i) % mc.EQ_RAW_EVERY != 0 for i in pick)
        small, _ = _hbm(ctx, kind, is_max, True, tg, vc, leq, eq=eq)
        assert got[0].tobytes() == small[0][pick].tobytes() and got[1].tobytes() == small[1][pick].tobytes()
        assert got[2].tobytes() == small[2][pick].tobytes()


@pytest.mark.parametrize("kind", [F64, RAT])
def test_a_rational_indicator_on_free_variables(ctx, port, kind):
    """Case 4: case 1's programs with flags on the free variables 0, 3 and 7 (mip_feed's `allow` branch): the oracle walks
    other trees than without them, and the device walks those."""
    tg, vc, leq = mc.wide(kind)
    changed = 0
    for is_max in (True, False):
        want = mc.wide_oracle(port, kind, is_max, mc.IND)
        changed += sum(a[3] != b[3] for a, b in zip(want, mc.wide_oracle(port, kind, is_max)))
        got, route = _hbm(ctx, kind, is_max, False, tg, vc, leq, ind=mc.IND)
        assert route["hbm"] == mc.WIDE_COUNT, route
        assert _against_oracle(got, want, ("ind", kind, is_max)) == mc.WIDE_COUNT
        _same_bytes(got, _host(ctx, kind, is_max, False, tg, vc, leq, ind=mc.IND), ("ind", kind, is_max))
    assert changed >= 4, changed


def test_a_workgroup_walks_tree_after_tree(ctx, port):
    """Case 5: nb = 2 x grid + 3 trees by tiling case 1's 16 programs (np.arange(nb) % 16, rotated by 5 from one round of the
    grid to the next: the grid is a multiple of 16, so a plain tiling would hand a workgroup the same program every round).
    Every workgroup walks two or three trees in the same slot and workspace; for 13 of the 16 residues, in either
    direction, the second differs from the first in status or depth. A stale forks, frame or slot shows up here."""
    from xpoly_amd.six import mip_hbm_plan
    tg, vc, leq = mc.wide(F64)
    grid = mip_hbm_plan(F64, vc, mc.WIDE_ROWS, 0, mc.WIDE_COLS, False, True, 1 << 20)["grid"]
    nb = 2 * grid + 3
    pick = mc.reuse_pick(nb, grid)
    for is_max in (True, False):
        want = mc.wide_oracle(port, F64, is_max)
        sig = [(w[0], w[3]) for w in want]
        assert sum(sig[i] != sig[(i + mc.REUSE_SHIFT) % mc.WIDE_COUNT] for i in range(mc.WIDE_COUNT)) >= 12
        got, route = _hbm(ctx, F64, is_max, False, np.ascontiguousarray(tg[pick]), vc, np.ascontiguousarray(leq[pick]))
        assert route["hbm"] == nb and nb >= 2 * route["grid"] + 3, route
        assert _against_oracle(got, [want[i] for i in pick], ("reuse", is_max)) == nb


def test_a_shape_that_fits_lds_keeps_the_lds_walk(ctx):
    """Case 6: 64 programs of shape (3, 4, 1): the bytes mip_batch_vc gives, from the same launch."""
    from xpoly_amd.six import mip_batch_vc, mip_last_route
    probs = fc.shape_problems((3, 4, 1), 64)
    for kind in (RAT, F64):
        for free, idx in fc.groups_by_free_set(probs):
            tg, vc, leq = fc.batch_arrays(probs, idx, kind)
            for is_max in (True, False):
                got, route = _hbm(ctx, kind, is_max, False, tg, vc, leq)
                assert route["lds"] == len(idx) and route["hbm"] == 0 and route["host"] == 0 and route["free"] == 1, route
                assert mip_last_route() == dict(device_trees=len(idx), host_trees=0, free_vars=1)
                other = mip_batch_vc(ctx, is_max, False, tg, vc, leq, kind=kind)
                assert mip_last_route() == dict(device_trees=len(idx), host_trees=0, free_vars=1)
                _same_bytes(got, other, ("fits", kind, free, is_max))


def test_a_general_vc_goes_to_the_host_controller(ctx, port):
    """Case 7: a diagonal of -2 and a nonzero constant are no sign patterns: the host controller under the caller's vc, the
    oracle's answers."""
    from xpoly_amd.six import mip_last_route
    nb = 16
    probs = fc.shape_problems((3, 4, 1), nb)
    tg = gen.to_rat(np.stack([p["tgtf"] for p in probs])); leq = gen.to_rat(np.stack([p["leq"] for p in probs]))
    for vc0 in fc.general_vcs(4):
        vc = gen.to_rat(vc0)
        for is_max in (True, False):
            got, route = _hbm(ctx, RAT, is_max, False, tg, vc, leq)
            assert route == dict(lds=0, hbm=0, host=nb, free=0, grid=0), route
            assert mip_last_route() == dict(device_trees=0, host_trees=nb, free_vars=0)
            with fc.non_strict(port):
                for b in range(nb):
                    want = port.mip_solve(RAT, is_max, False, tg[b], vc, None, leq[b])
                    assert want[0] != -7, b
                    assert fc.same_answer(got[0][b], got[1][b], got[2][b], want), (is_max, b, got[0][b], want[0])


def test_an_empty_batch_a_trim_and_malformed_calls(ctx):
    """Case 8: nb = 0 is no launch and no error; after xpg_trim has returned the slots a correct call gives the same bytes;
    bad shapes return XPG_ERR_SHAPE and leave the outputs alone."""
    from xpoly_amd._capi import lib
    tg, vc, leq = mc.wide(F64)
    got, route = _hbm(ctx, F64, True, False, tg[:0], vc, leq[:0])
    assert route == dict(lds=0, hbm=0, host=0, free=0, grid=0) and got[0].shape == (0,) and got[3] == 0
    first, route = _hbm(ctx, F64, True, False, tg, vc, leq)
    assert route["hbm"] == mc.WIDE_COUNT
    ctx.trim()
    again, route = _hbm(ctx, F64, True, False, tg, vc, leq)
    assert route["hbm"] == mc.WIDE_COUNT
    _same_bytes(first, again, "after trim")
    st = np.full(4, 77, dtype=np.int32); v = np.full(4, 5.0); sol = np.full((4, mc.WIDE_COLS), 6.0)
    nodes = C.c_longlong(-5)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    f = lib().xpg_mip_batch_vc_hbm_f64
    h = ctx._h
    assert f(h, -1, 1, 0, p(tg), p(vc), None, 0, p(leq), 50, 21, None, p(st), p(v), p(sol), C.byref(nodes)) == XPG_ERR_SHAPE
    assert f(h, 4, 1, 0, p(tg), p(vc), None, 0, None, 0, 21, None, p(st), p(v), p(sol), C.byref(nodes)) == XPG_ERR_SHAPE      # no rows at all
    assert f(h, 4, 1, 0, p(tg), p(vc), None, 2, p(leq), 50, 21, None, p(st), p(v), p(sol), C.byref(nodes)) == XPG_ERR_SHAPE   # eq rows without eq
    assert f(h, 4, 1, 0, p(tg), None, None, 0, p(leq), 50, 21, None, p(st), p(v), p(sol), C.byref(nodes)) == XPG_ERR_SHAPE
    assert f(h, 4, 1, 0, p(tg), p(vc), None, 0, p(leq), 50, 1, None, p(st), p(v), p(sol), C.byref(nodes)) == XPG_ERR_SHAPE
    assert (st == 77).all() and (v == 5.0).all() and (sol == 6.0).all() and nodes.value == -5


def test_one_tree_alone(ctx, port):
    """Case 9: nb = 1 of case 1: the device-memory walk with a grid of one, the answer it has inside the batch."""
    tg, vc, leq = mc.wide(F64)
    for is_max in (True, False):
        want = mc.wide_oracle(port, F64, is_max)
        b = max(range(mc.WIDE_COUNT), key=lambda i: want[i][3])   # the deepest tree
        got, route = _hbm(ctx, F64, is_max, False, tg[b:b + 1], vc, leq[b:b + 1])
        assert route == dict(lds=0, hbm=1, host=0, free=mc.WIDE_FREE, grid=1), route
        assert _against_oracle(got, [want[b]], ("one", is_max)) == 1
