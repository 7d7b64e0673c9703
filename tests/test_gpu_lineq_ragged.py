"""GPU parity of the ragged projection / levels entry points (xpg_lineq_{project,levels}_batch_ragged_rat32: systems of mixed
shapes, constant columns and lists in ONE launch of k_fme_chain_ragged) against the CPU checker's fme applied step after step
per system with its own list (tests/lineq_ragged_cases.py), against the real reference where its build is present, and against
the product's own uniform calls class by class. The base batch interleaves four shape classes of
tests/test_gpu_lineq_project.py's generator. Bit-exact: nothing is compared with a tolerance."""
import subprocess

import numpy as np
import pytest

import lineq_ragged_cases as rc
from lineq_ragged_cases import XPG_ERR_SHAPE, XPG_ERR_UNSUPPORTED, rows_equal
from tools import gen

pytestmark = pytest.mark.gpu

CAP = 256                                                    # the explicit cap_rows of the parity runs


@pytest.fixture(scope="module")
def lq(ctx):
    from xpoly_amd.lineq import Lineq
    return Lineq(ctx)


def _shape(mats, nvs, elims):
    return [m.shape[0] for m in mats], [m.shape[1] for m in mats], list(nvs), elims


def _levels_cap_out(mats, nvs, elims, cap_rows, cap_out_rows=0):
    """The cap_out_rows a levels call settles on (host-only plan view)."""
    return rc.plan_view(*_shape(mats, nvs, elims), True, cap_rows, cap_out_rows)["cap_out"]


def _check_project(got, want, tag=()):
    ok, steps, res = got
    assert len(ok) == len(want) == len(res)
    for b, w in enumerate(want):
        assert (ok[b], steps[b]) == (w[0], w[1]), tag + (b, ok[b], steps[b], w[0], w[1])
        assert rows_equal(res[b], w[2]), tag + (b,)
        assert res[b].shape[1:] == (w[2].shape[1], 2), tag + (b, res[b].shape)


def _check_levels(got, want, tag=()):
    ok, steps, levels = got
    assert len(ok) == len(want) == len(levels)
    for b, w in enumerate(want):
        assert (ok[b], steps[b]) == (w[0], w[1]), tag + (b, ok[b], steps[b], w[0], w[1])
        assert len(levels[b]) == len(w[2]), tag + (b,)
        for k, wl in enumerate(w[2]):
            assert rows_equal(levels[b][k], wl), tag + (b, k)
        if w[0] <= 0:                                        # a failed system: 0 rows at EVERY level, those before its step too
            assert all(lv.shape[0] == 0 for lv in levels[b]), tag + (b,)


def base_wants(port):
    """The stepped checker's answers for the base batch, computed once: {("project" | "levels", dark): [per system]}. What the
    parity test asks of the batch is asserted here, on the checker's answers: verdicts {0, 1}, stop steps {0, 1, 2, 3}."""
    mats, nvs, elims = rc.base_batch()
    cap_out = _levels_cap_out(mats, nvs, elims, CAP)
    out = {}
    for dark in (False, True):
        out[("project", dark)] = rc.want_project(port, mats, nvs, elims, dark, cap_rows=CAP)
        out[("levels", dark)] = rc.want_levels(port, mats, nvs, elims, dark, cap_rows=CAP, cap_out_rows=cap_out)
        for kind in ("project", "levels"):
            assert {w[0] for w in out[(kind, dark)]} == {0, 1}, (kind, dark)
            assert {w[1] for w in out[(kind, dark)]} == {0, 1, 2, 3}, (kind, dark)
    return out


@pytest.fixture(scope="module")
def base():
    return rc.base_batch()


@pytest.fixture(scope="module")
def wants(port):
    return base_wants(port)


# ---- 1. parity against the stepped checker --------------------------------------------------------------------------------------
def test_every_system_matches_the_stepped_checker(lq, base, wants):
    mats, nvs, elims = base
    assert len(mats) == 48
    for dark in (False, True):
        _check_project(lq.project_ragged(mats, nvs, elims, dark, cap_rows=CAP), wants[("project", dark)], ("project", dark))
        assert lq.ragged_last_route()["launches"] == 1
        _check_levels(lq.levels_ragged(mats, nvs, elims, dark, cap_rows=CAP), wants[("levels", dark)], ("levels", dark))
        assert lq.ragged_last_route()["launches"] == 1
        # a system that failed after its first step HAD rows at the levels before: they are gone all the same
        assert any(w[0] == 0 and w[1] > 0 and w[4] and w[4][0] > 0 for w in wants[("levels", dark)])
    # the lists default to rhs_idx-1 .. 1 of each system, the constant column to the last one
    nest = [list(range(nv - 1, 0, -1)) for nv in nvs]
    a = lq.levels_ragged(mats, nvs, nest, cap_rows=CAP)
    b = lq.levels_ragged(mats, None, None, cap_rows=CAP)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert all(len(x) == len(y) and all(rows_equal(p, q) for p, q in zip(x, y)) for x, y in zip(a[2], b[2]))


def test_every_system_matches_the_real_reference(lq, ref, base):
    """The same batch against the reference's own Lineq::fme, step after step, where its build is present."""
    mats, nvs, elims = base
    cap_out = _levels_cap_out(mats, nvs, elims, CAP)
    for dark in (False, True):
        _check_project(lq.project_ragged(mats, nvs, elims, dark, cap_rows=CAP), rc.want_project(ref, mats, nvs, elims, dark, cap_rows=CAP), (dark,))
        _check_levels(lq.levels_ragged(mats, nvs, elims, dark, cap_rows=CAP),
                      rc.want_levels(ref, mats, nvs, elims, dark, cap_rows=CAP, cap_out_rows=cap_out), (dark,))


# ---- 2. parity against the project's own uniform calls -------------------------------------------------------------------------
def test_every_class_matches_its_uniform_call(lq, base):
    mats, nvs, elims = base
    for dark in (False, True):
        pok, psteps, pres = lq.project_ragged(mats, nvs, elims, dark, cap_rows=CAP, cap_out_rows=40)
        lok, lsteps, lres = lq.levels_ragged(mats, nvs, elims, dark, cap_rows=CAP, cap_out_rows=40)
        for c, (rows, nv, el) in enumerate(rc.SHAPES):
            idx = list(range(c, 48, 4))
            cls = np.stack([mats[b] for b in idx])
            assert cls.shape[1:3] == (rows, nv + 1)
            uok, usteps, ures = lq.project_packed(cls, nv, el, dark, cap_rows=CAP, cap_out_rows=40)
            assert [pok[b] for b in idx] == uok.tolist() and [psteps[b] for b in idx] == usteps.tolist(), (dark, c)
            assert all(rows_equal(pres[b], ures[i]) for i, b in enumerate(idx)), (dark, c)
            uok, usteps, ures = lq.levels_packed(cls, nv, el, dark, cap_rows=CAP, cap_out_rows=40)
            assert [lok[b] for b in idx] == uok.tolist() and [lsteps[b] for b in idx] == usteps.tolist(), (dark, c)
            assert all(rows_equal(lres[b][k], ures[i][k]) for i, b in enumerate(idx) for k in range(len(el))), (dark, c)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


# (rows, nv, list, systems, cap_rows): a small nest, and HOMES at the capacity that puts its steps' results on both sides of cap_lds
TWINS = [(8, 5, [4, 3, 2, 1], 5, CAP), rc.HOMES + (None,)]


@pytest.mark.parametrize("rows,nv,el,nb,cap", TWINS)
def test_one_shape_gives_the_same_bits_through_the_uniform_and_the_ragged_kernels(lq, port, rows, nv, el, nb, cap):
    """The uniform and the ragged kernels run ONE walk (lineq_kernels.hip.h w_chain_walk) through two views of a system: a batch
    whose systems all share one shape gets the same plan from both calls and must come back bit for bit the same -- rows, their
    counts, ok and steps -- as a projection and with every level kept."""
    mats = rc.class_batch(rows, nv, nb)
    want = [rc.stepped(port, mats[b], nv, el) for b in range(nb)]
    needs = [n for w in want for n in w[3] if n is not None]
    both_homes = cap is None
    cap = cap or max(128, max(needs))
    cap_lds = rc.plan_view([rows] * nb, [nv + 1] * nb, None, [el] * nb, True, cap, cap)["cap_lds"]
    assert max(needs) <= cap and any(w[0] == 1 and w[2].shape[0] > 0 for w in want)
    if both_homes:                                           # results of steps in LDS and in the seat's device slots
        assert sum(n <= cap_lds for n in needs) >= 4 and sum(n > cap_lds for n in needs) >= 4, (cap_lds, sorted(needs))
    for dark in (False, True):
        uok, usteps, ures = lq.project_packed(mats, nv, el, dark, cap_rows=cap, cap_out_rows=cap)
        assert lq.project_last_route()["cap_lds"] == cap_lds
        rok, rsteps, rres = lq.project_ragged(list(mats), None, [el] * nb, dark, cap_rows=cap, cap_out_rows=cap)
        assert lq.ragged_last_route()["cap_lds"] == cap_lds
        assert np.array_equal(uok, rok) and np.array_equal(usteps, rsteps), (dark, uok, rok, usteps, rsteps)
        assert all(_same_bits(ures[b], rres[b]) for b in range(nb)), dark
        uok, usteps, ulev = lq.levels_packed(mats, nv, el, dark, cap_rows=cap, cap_out_rows=cap)
        assert lq.levels_last_route()["cap_lds"] == cap_lds
        rok, rsteps, rlev = lq.levels_ragged(list(mats), None, [el] * nb, dark, cap_rows=cap, cap_out_rows=cap)
        assert lq.ragged_last_route()["cap_lds"] == cap_lds
        assert np.array_equal(uok, rok) and np.array_equal(usteps, rsteps), (dark, uok, rok, usteps, rsteps)
        assert all(len(rlev[b]) == len(el) and _same_bits(ulev[b][k], rlev[b][k]) for b in range(nb) for k in range(len(el))), dark


# ---- 3. one launch, planned as restated ----------------------------------------------------------------------------------------
def test_four_classes_take_one_launch_and_the_restated_plan(lq, base):
    mats, nvs, elims = base
    for levels, call in ((False, lq.project_ragged), (True, lq.levels_ragged)):
        for cap, cap_out in ((0, 0), (CAP, 0), (CAP, 40)):
            call(mats, nvs, elims, cap_rows=cap, cap_out_rows=cap_out)
            route = lq.ragged_last_route()
            planned = rc.plan(*_shape(mats, nvs, elims), levels, cap, cap_out)
            assert route["launches"] == 1 and route == {k: planned[k] for k in rc.ROUTE_KEYS}, (levels, cap, cap_out, route, planned)
            assert planned["cols"] == 5 and planned["rows"] == 9 and route["grid"] == 48


# ---- 4. order independence: neighbours of one wavefront differ in layout ----------------------------------------------------------
def test_results_do_not_depend_on_the_order_of_the_systems(lq, base, wants):
    mats, nvs, elims = base
    wide = [b for b in range(48) if mats[b].shape == (9, 5, 2)]
    narrow = [b for b in range(48) if mats[b].shape == (4, 3, 2)]
    rest = [b for b in range(48) if b not in wide and b not in narrow]
    rest = [rest[i] for i in np.random.default_rng(11).permutation(len(rest))]
    shuffle = [b for pair in zip(wide, narrow) for b in pair] + rest
    assert sorted(shuffle) == list(range(48))
    shapes = [mats[b].shape[:2] for b in shuffle]
    assert any(shapes[i] == (9, 5) and shapes[i + 1] == (4, 3) for i in range(47))
    assert any(shapes[i] == (4, 3) and shapes[i + 1] == (9, 5) for i in range(47))
    # (48 systems have a workgroup each; the batch above the grid, below, is where one wavefront takes a 9 x 5 system and then
    # a 4 x 3 one on the same seat, and the other way round)
    for order in (list(range(48)), list(range(47, -1, -1)), shuffle):
        pick = lambda xs: [xs[b] for b in order]
        for dark in (False, True):
            _check_project(lq.project_ragged(pick(mats), pick(nvs), pick(elims), dark, cap_rows=CAP), pick(wants[("project", dark)]), (dark,))
            _check_levels(lq.levels_ragged(pick(mats), pick(nvs), pick(elims), dark, cap_rows=CAP), pick(wants[("levels", dark)]), (dark,))


# ---- 5. both homes of an intermediate in one launch ------------------------------------------------------------------------------
def homes_batch():
    """The (12, 6, [5, 4]) systems of tests/test_gpu_lineq_levels.py's HOMES and four 4 x 3 systems, interleaved."""
    rows, nv, el, nb = rc.HOMES
    big = rc.class_batch(rows, nv, nb)
    small = rc.class_batch(*rc.SHAPES[0][:2], 4)
    mats, nvs, elims = [], [], []
    for i in range(nb):
        mats.append(big[i]); nvs.append(nv); elims.append(list(el))
        if i % 2 == 0:
            mats.append(small[i // 2]); nvs.append(rc.SHAPES[0][1]); elims.append(list(rc.SHAPES[0][2]))
    return mats, nvs, elims


def homes_wants(port):
    """(batch, cap, cap_lds, the checker's levels without a capacity): cap holds every step and its plan keeps cap_lds < cap;
    the needs of the steps whose rows are stored fall on both sides of cap_lds."""
    mats, nvs, elims = homes_batch()
    want = rc.want_levels(port, mats, nvs, elims)
    needs = [n for w in want for n in w[3] if n is not None]
    cap = max(128, max(needs))
    p = rc.plan_view(*_shape(mats, nvs, elims), True, cap, cap)
    assert p["cap_lds"] < cap and p["cols"] == 7, p
    stored = [w[3][k] for w in want if w[0] == 1 for k in range(len(w[4])) if w[4][k] > 0]
    assert any(n <= p["cap_lds"] for n in stored) and any(n > p["cap_lds"] for n in stored), (p["cap_lds"], sorted(stored))
    return (mats, nvs, elims), cap, p["cap_lds"], want


@pytest.fixture(scope="module")
def homes(port):
    return homes_wants(port)


def test_steps_in_lds_and_on_a_device_side_in_one_launch(lq, port, homes):
    (mats, nvs, elims), cap, cap_lds, want = homes
    got = lq.levels_ragged(mats, nvs, elims, cap_rows=cap, cap_out_rows=cap)
    assert lq.ragged_last_route()["cap_lds"] == cap_lds and lq.ragged_last_route()["launches"] == 1
    _check_levels(got, want)
    _check_project(lq.project_ragged(mats, nvs, elims, cap_rows=cap), rc.want_project(port, mats, nvs, elims))


# ---- 6. capacities ---------------------------------------------------------------------------------------------------------------
def test_a_short_cap_rows_is_reported_with_its_step_and_the_rest_is_packed(lq, port, homes):
    (mats, nvs, elims), _, _, want = homes
    needs = [n for w in want for n in w[3] if n is not None]
    cap = max(needs) - 1
    assert cap >= 12
    short = rc.want_levels(port, mats, nvs, elims, cap_rows=cap)
    assert any(w[0] < 0 for w in short) and any(w[0] == 1 and any(lv.shape[0] for lv in w[2]) for w in short)
    got = lq.levels_ragged(mats, nvs, elims, cap_rows=cap, cap_out_rows=cap)
    _check_levels(got, short)
    for b, w in enumerate(short):
        if w[0] < 0:
            assert -got[0][b] == w[3][w[1]] > cap and got[1][b] == w[1]
    pshort = rc.want_project(port, mats, nvs, elims, cap_rows=cap)
    pgot = lq.project_ragged(mats, nvs, elims, cap_rows=cap)
    _check_project(pgot, pshort)
    assert any(w[0] < 0 for w in pshort) and np.array_equal(pgot[0] < 0, got[0] < 0)
    # once more with the largest need reported: every step fits
    need = int(-got[0].min())
    assert need == max(needs)
    _check_levels(lq.levels_ragged(mats, nvs, elims, cap_rows=need, cap_out_rows=need), want)
    _check_project(lq.project_ragged(mats, nvs, elims, cap_rows=need), rc.want_project(port, mats, nvs, elims))


def test_a_short_output_slot_is_reported_at_an_intermediate_level(lq, port, homes):
    (mats, nvs, elims), _, _, want = homes
    cap = max(n for w in want for n in w[3] if n is not None)
    step = 0                                                 # an intermediate level of the two-step lists (chosen here, on the CPU)
    sizes = [w[4][step] for w, el in zip(want, elims) if len(el) > 1 and len(w[4]) > step]
    cap_out = max(sizes) - 1
    assert cap_out >= 1
    short = rc.want_levels(port, mats, nvs, elims, cap_rows=cap, cap_out_rows=cap_out)
    hit = [b for b, w in enumerate(short) if w[0] < 0 and w[1] == step and len(elims[b]) > 1]
    assert hit and any(w[0] == 1 and any(lv.shape[0] for lv in w[2]) for w in short)
    got = lq.levels_ragged(mats, nvs, elims, cap_rows=cap, cap_out_rows=cap_out)
    _check_levels(got, short)
    for b in hit:                                            # -rows, with cap_out_rows < rows <= cap_rows: the level, not the step
        assert cap_out < -got[0][b] <= cap and -got[0][b] == want[b][4][step] and got[1][b] == step
    # once more with the largest need reported: no level is larger (a level has at most the rows its step built)
    need = -int(got[0].min())
    assert cap_out < need <= cap and need == max(s for w in want for s in w[4])
    _check_levels(lq.levels_ragged(mats, nvs, elims, cap_rows=cap, cap_out_rows=need), want)


# ---- 7. seats above the grid -------------------------------------------------------------------------------------------------------
def test_seats_are_reused_above_the_grid(lq, base, wants):
    mats, nvs, elims = base
    nb = 4096 + 300
    # workgroup j takes system j and then system 4096 + j: the tail runs through the 48 backwards, so that the second system of a
    # seat is of ANOTHER class than the first -- a 4 x 3 system after a 9 x 5 one, a 9 x 5 after a 4 x 3, 5 x 4 and 6 x 5 swapped
    src = [b % 48 if b < 4096 else 47 - (b - 4096) % 48 for b in range(nb)]
    pairs = {(mats[src[j]].shape[:2], mats[src[4096 + j]].shape[:2]) for j in range(300)}
    assert pairs == {((9, 5), (4, 3)), ((4, 3), (9, 5)), ((5, 4), (6, 5)), ((6, 5), (5, 4))}, pairs
    tile = lambda xs: [xs[i] for i in src]
    ok, steps, levels = lq.levels_ragged(tile(mats), tile(nvs), tile(elims), cap_rows=CAP)
    route = lq.ragged_last_route()
    planned = rc.plan(*_shape(tile(mats), tile(nvs), tile(elims)), True, CAP)
    assert route == {k: planned[k] for k in rc.ROUTE_KEYS}, (route, planned)
    assert route["launches"] == 1 and nb > route["grid"] * route["groups"] == 4096
    want = wants[("levels", False)]
    for b in range(nb):
        w = want[src[b]]
        assert (ok[b], steps[b]) == (w[0], w[1]), b
        assert len(levels[b]) == len(w[2]) and all(rows_equal(levels[b][k], w[2][k]) for k in range(len(w[2]))), b
    pok, psteps, pres = lq.project_ragged(tile(mats), tile(nvs), tile(elims), cap_rows=CAP)
    assert lq.ragged_last_route()["launches"] == 1
    want = wants[("project", False)]
    for b in range(nb):
        w = want[src[b]]
        assert (pok[b], psteps[b]) == (w[0], w[1]) and rows_equal(pres[b], w[2]), b


# ---- 8. zeros and views --------------------------------------------------------------------------------------------------------------
def test_zero_systems_end_empty_and_views_equal_copies(lq, base):
    mats, nvs, elims = base
    zeros = [gen.to_rat(np.zeros(m.shape[:2], dtype=np.int32)) for m in mats[:8]]
    ok, steps, levels = lq.levels_ragged(zeros, nvs[:8], elims[:8])
    assert ok.tolist() == [1] * 8 and steps.tolist() == [len(e) for e in elims[:8]]
    assert all(lv.shape[0] == 0 for b in range(8) for lv in levels[b]) and [len(lv) for lv in levels] == [len(e) for e in elims[:8]]
    ok, steps, res = lq.project_ragged(zeros, nvs[:8], elims[:8])
    assert ok.tolist() == [1] * 8 and steps.tolist() == [len(e) for e in elims[:8]] and all(r.shape[0] == 0 for r in res)
    # views: read before the next packed call
    a = lq.levels_ragged(mats, nvs, elims, cap_rows=64)
    v = lq.levels_ragged(mats, nvs, elims, cap_rows=64, copy=False)
    assert np.array_equal(a[0], v[0]) and all(rows_equal(x, y) for b in range(48) for x, y in zip(a[2][b], v[2][b]))
    a = lq.project_ragged(mats, nvs, elims, cap_rows=64)
    v = lq.project_ragged(mats, nvs, elims, cap_rows=64, copy=False)
    assert np.array_equal(a[0], v[0]) and all(rows_equal(a[2][b], v[2][b]) for b in range(48))
    assert any(r.shape[0] for r in a[2])
    # no systems
    ok0, steps0, lev0 = lq.levels_ragged([], [], [])
    assert len(ok0) == 0 and lev0 == []


# ---- 9. errors launch nothing --------------------------------------------------------------------------------------------------------
def test_errors_launch_nothing(ctx, lq, base):
    import ctypes as C
    from xpoly_amd._capi import lib, vp
    mats, nvs, elims = base
    flat = np.ascontiguousarray(np.concatenate([m.reshape(-1, 2) for m in mats[:4]]))
    rows, cols, _, _ = _shape(mats[:4], nvs[:4], elims[:4])
    off = np.zeros(5, dtype=np.int64); off[1:] = np.cumsum([r * c for r, c in zip(rows, cols)])
    ooff = np.zeros(4 * 65 + 1, dtype=np.int64); orows = np.zeros(4 * 65, dtype=np.int32)
    ok = np.zeros(4, dtype=np.int32); steps = np.zeros(4, dtype=np.int32)

    def call(name, el, rhs=None, cap=0, outs=None, outs_cap=0):
        r, c, h, e, eo = rc._args(rows, cols, nvs[:4] if rhs is None else rhs, el)
        code = getattr(lib(), name)(ctx._h, C.c_int(4), vp(flat), vp(r), vp(c), vp(off), vp(h), vp(e), vp(eo), C.c_int(0), C.c_int(cap),
                                    C.c_int(0), vp(outs), C.c_longlong(outs_cap), None, vp(ooff), vp(orows), vp(ok), vp(steps))
        assert lq.ragged_last_route()["launches"] == (1 if code == 0 or outs is not None else 0), (name, code)
        return code

    for name in ("xpg_lineq_project_batch_ragged_rat32", "xpg_lineq_levels_batch_ragged_rat32"):
        good = [list(e) for e in elims[:4]]
        assert call(name, good) == 0
        with_ = lambda b, e: good[:b] + [e] + good[b + 1:]
        assert call(name, with_(2, [])) == XPG_ERR_SHAPE                              # n_elim[b] <= 0
        assert call(name, with_(3, [4])) == XPG_ERR_SHAPE and call(name, with_(1, [2, -1])) == XPG_ERR_SHAPE
        assert call(name, good, rhs=[2, 3, 4, 5]) == XPG_ERR_SHAPE and call(name, with_(0, [0]), rhs=[0, 3, 4, 4]) == XPG_ERR_SHAPE
        assert call(name, with_(3, [3] * (rc.CHAIN_MAX + 1))) == XPG_ERR_UNSUPPORTED and call(name, with_(3, [3] * rc.CHAIN_MAX)) == 0
        assert call(name, good, cap=32768) == XPG_ERR_UNSUPPORTED                     # cap > 32767
        assert call(name, good, cap=5000) == XPG_ERR_UNSUPPORTED                      # the envelope's layout over 160 KB
        # a sizing call fills the offsets; a buffer one cell short is refused with offsets, counts and verdicts filled
        nres = sum(len(e) for e in good) if "levels" in name else 4
        assert call(name, good, cap=64) == 0 and ooff[nres] > 0
        total = int(ooff[nres])
        want_off = ooff[: nres + 1].copy()
        out = np.zeros((total, 2), dtype=np.int32)
        ooff[:] = 0; steps[:] = -1
        assert call(name, good, cap=64, outs=out, outs_cap=total - 1) == XPG_ERR_SHAPE
        assert np.array_equal(ooff[: nres + 1], want_off) and (steps >= 0).all()
        assert call(name, good, cap=64, outs=out, outs_cap=total) == 0
        py = (lq.levels_ragged if "levels" in name else lq.project_ragged)(mats[:4], nvs[:4], good, cap_rows=64)[2]
        flat_res = [lv for per in py for lv in per] if "levels" in name else py
        assert all(np.array_equal(out[want_off[r]: want_off[r + 1]].reshape(flat_res[r].shape), flat_res[r]) for r in range(nres))


# ---- 10. adapter ---------------------------------------------------------------------------------------------------------------------
def test_the_collectors_answer_nests_of_three_depths_in_one_call(port, tmp_path):
    """tests/cxx/levels_nests.cpp in a child process: nests of depth 3, 4 and 6, three row classes each, through ONE
    xpoly_amd::levels_nests call and one xpoly_amd::project_each call, every entry compared in there with the adapter's own
    Lineq::fme run as the reference's loop runs it. One class -- 13 rows at depth 3, found here on the CPU by replaying the
    adapter's calls on the checker -- has a step that needs more rows than the envelope's first capacity, so the adapter calls
    again with the need reported; the program adds an empty system and a nest of depth 1, answered without a call."""
    from test_lineq_ragged_host import build_adapter_test
    exe = build_adapter_test()
    nests = rc.adapter_nests(port)
    calls, short = rc.adapter_calls(port, nests)
    assert 2 <= calls <= 4 and short == {(3, 13)}, (calls, short)
    assert {nv for nv, _ in nests} == {3, 4, 6} and len({(nv, m.shape[0]) for nv, m in nests}) == 9
    lines = ["%d" % len(nests)]
    for nv, m in nests:
        lines += ["%d %d %d" % ((nv,) + m.shape), " ".join(str(int(x)) for x in m.ravel())]
    path = str(tmp_path / "nests.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert "levels rc 0 launches 1" in out and "project rc 0 launches 1" in out and "mismatches 0" in out
    per_system = [ln.split() for ln in out if " ok " in ln]
    assert len(per_system) == len(nests) + 2
    assert all(p[8] == "1" and p[10] == "1" for p in per_system) and {p[6] for p in per_system} == {"0", "1"}
