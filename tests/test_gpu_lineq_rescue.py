"""GPU parity of the fused row-elimination entry points WHERE THE RATIONAL APPROXIMATES: the loop nests of
tests/lineq_rescue_cases.py -- tile sizes, strides and array extents for coefficients -- make a numerator or denominator leave
int32 inside the chain, the float32 `appro` rescue (scalar.hip.h) replaces the cell, and from there on the answer depends on
the order of every '+', '*' and reduction. Each of k_fme_chain_batch, k_fme_levels_batch, k_calc_bound_batch, k_fme_chain_ragged,
k_calc_bound_ragged, k_group_reduce and k_transform_levels_batch is held against the checkers' existing compositions, with the
restatement always and with the real reference where its build is present, in the all-LDS layout and in the layout past 12 KB.
Bit for bit: verdict, failing step or chain, row counts, every cell; nothing is compared with a tolerance, no case is filtered.
Every test asserts that the checker's appro_count moved on its batch and prints `entry family: port / ref / rescued`."""
import numpy as np
import pytest

import lineq_bounds_cases as bc
import lineq_bounds_ragged_cases as brc
import lineq_hull_cases as hc
import lineq_levels_cases as lc
import lineq_project_cases as pc
import lineq_ragged_cases as rc
import lineq_rescue_cases as rq
import lineq_transform_cases as tc
from lineq_rescue_cases import rows_equal

pytestmark = pytest.mark.gpu

PAST = 256                                                   # a cap_rows past the 12 KB layout at every shape of the small families
N_REF = 8                                                    # systems per family held against the reference's build directly


@pytest.fixture(scope="module")
def lq(ctx):
    from xpoly_amd.lineq import Lineq
    return Lineq(ctx)


@pytest.fixture(scope="module")
def ref_or_none():
    from oracle.checker import Ref
    return Ref() if Ref.available() else None


class Tally:
    """Systems compared with the restatement, with the reference's build, and those among the first on which the checker
    rescued at all."""
    def __init__(self, what):
        self.what, self.port, self.ref, self.rescued = what, 0, 0, 0

    def done(self, ref):
        print("%s: port %d, ref %s, rescued %d" % (self.what, self.port, self.ref if ref else "not built", self.rescued))
        assert self.port > 0 and self.rescued > 0, self.what


def _check_project(got, want, tag):
    ok, steps, res = got
    assert len(ok) == len(want) == len(res), tag
    for b, w in enumerate(want):
        assert (ok[b], steps[b]) == (w[0], w[1]), tag + (b, ok[b], steps[b], w[0], w[1])
        assert rows_equal(res[b], w[2]), tag + (b,)


def _check_levels(got, want, tag):
    ok, steps, levels = got
    assert len(ok) == len(want) == len(levels), tag
    for b, w in enumerate(want):
        assert (ok[b], steps[b]) == (w[0], w[1]), tag + (b, ok[b], steps[b], w[0], w[1])
        assert len(levels[b]) == len(w[2]), tag + (b,)
        for k, wl in enumerate(w[2]):
            assert rows_equal(levels[b][k], wl), tag + (b, k)
        if w[0] <= 0:
            assert all(lv.shape[0] == 0 for lv in levels[b]), tag + (b,)


def _check_bounds(got, want, tag):
    ok, chain, steps, bounds = got
    assert len(ok) == len(want) == len(bounds), tag
    for b, (wok, wchain, wsteps, wb) in enumerate(want):
        assert (ok[b], chain[b], steps[b]) == (wok, wchain, wsteps), tag + (b, ok[b], chain[b], steps[b], wok, wchain, wsteps)
        assert len(bounds[b]) == len(wb) and all(rows_equal(g, w) for g, w in zip(bounds[b], wb)), tag + (b,)


CHECK = {"project": _check_project, "levels": _check_levels, "bounds": _check_bounds}
WANT = {"project": rq.want_project, "levels": rq.want_levels, "bounds": rq.want_bounds}


def _uniform(lq, port, ref, family, mats, cap_rows, cap_out_rows, past):
    """project_packed, levels_packed and bounds_packed of one family at one pair of capacities: the layout asserted from the
    plan views, the answers from the checkers at the capacities the plans settle on."""
    n = rq.depth(family)
    nb, rows, cols = mats.shape[:3]
    el = rq.elim_of(n)
    plans = {"project": pc.plan_view(nb, rows, cols, cap_rows, cap_out_rows), "levels": lc.plan_view(nb, rows, cols, n - 1, cap_rows, cap_out_rows),
             "bounds": bc.plan_view(nb, rows, cols, n, cap_rows, cap_out_rows)}
    calls = {"project": lambda: lq.project_packed(mats, n, el, cap_rows=cap_rows, cap_out_rows=cap_out_rows),
             "levels": lambda: lq.levels_packed(mats, n, el, cap_rows=cap_rows, cap_out_rows=cap_out_rows),
             "bounds": lambda: lq.bounds_packed(mats, n, cap_rows=cap_rows, cap_out_rows=cap_out_rows)}
    routes = {"project": lq.project_last_route, "levels": lq.levels_last_route, "bounds": lq.bounds_last_route}
    for entry in ("project", "levels", "bounds"):
        p = plans[entry]
        if past:                                             # one factor per input row in LDS, a larger result in the seat's slots
            assert p["cap_lds"] < p["cap"], (family, entry, p)
        else:                                                # the whole result area in LDS
            assert p["cap_lds"] == p["cap"], (family, entry, p)
        t = Tally("%s_packed %s %s" % (entry, family, "past 12 KB" if past else "all LDS"))
        got = calls[entry]()
        route = routes[entry]()
        assert route["launches"] == 1 and route["cap_lds"] == p["cap_lds"], (family, entry, route, p)
        want, rescues = WANT[entry](port, mats, n, p["cap"], p["cap_out"])
        CHECK[entry](got, want, (family, entry, "port"))
        t.port, t.rescued = nb, sum(r > 0 for r in rescues)
        if ref:
            k = min(nb, N_REF)
            CHECK[entry](tuple(x[:k] for x in got), WANT[entry](ref, mats[:k], n, p["cap"], p["cap_out"])[0], (family, entry, "ref"))
            t.ref = k
        t.done(ref)
        if family != "d4_empty":
            assert all(w[0] == 1 for w in want), (family, entry)     # no capacity verdict stands in for an answer
    return plans


# ---- 1. the uniform walks in both layouts ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", rq.SMALL)
def test_the_uniform_walks_at_the_default_capacities(lq, port, ref_or_none, family):
    _uniform(lq, port, ref_or_none, family, rq.family(family), 0, 0, past=False)


@pytest.mark.parametrize("family", rq.SMALL)
def test_the_uniform_walks_past_the_lds_layout(lq, port, ref_or_none, family):
    """The same families at a cap_rows whose layout keeps cap_lds < cap rows of results in LDS. These nests' steps need 11 rows
    at the most, so their results are still built in LDS, behind a different layout; the next test puts them in the seats."""
    _uniform(lq, port, ref_or_none, family, rq.family(family), PAST, PAST, past=True)


def test_rescued_intermediates_in_the_seats_device_slots(lq, port, ref_or_none):
    """d5_wide: 14 x 7, a first step of 17 rows and later steps of hundreds -- built and reduced in the seat's device slots,
    loaded from there, stored as levels from there, held in calcBound's hold slot."""
    mats = rq.family("d5_wide", rq.WIDE_NB)
    plans = _uniform(lq, port, ref_or_none, "d5_wide", mats, rq.WIDE_CAP, rq.WIDE_CAP, past=True)
    want, rescues = rq.want_project(port, mats, 5)
    needs = [x for w in want for x in w[3]]
    assert all(r > 0 for r in rescues) and sum(x > plans["project"]["cap_lds"] for x in needs) >= rq.WIDE_NB
    bneeds = [x for m in mats for x in bc.step_needs(port, m, 5)[0].values()]
    assert sum(x > plans["bounds"]["cap_lds"] for x in bneeds) >= rq.WIDE_NB and max(bneeds) <= rq.WIDE_CAP


@pytest.mark.parametrize("nb", [1, 3, 65])
def test_lanes_and_cells_at_partial_occupancy(lq, port, nb):
    """nb = 1, 3 and 65 systems of the (30 000, 70 000) depth-4 family, tiled from its 16."""
    base = rq.family("d4_w")
    mats = np.ascontiguousarray(np.stack([base[b % rq.PER] for b in range(nb)]))
    n, el = 4, rq.elim_of(4)
    wp, rescues = rq.want_project(port, base, n)
    assert all(r > 0 for r in rescues)
    _check_project(lq.project_packed(mats, n, el), [wp[b % rq.PER] for b in range(nb)], ("project", nb))
    wl, _ = rq.want_levels(port, base, n)
    _check_levels(lq.levels_packed(mats, n, el), [wl[b % rq.PER] for b in range(nb)], ("levels", nb))
    wb, _ = rq.want_bounds(port, base, n)
    _check_bounds(lq.bounds_packed(mats, n), [wb[b % rq.PER] for b in range(nb)], ("bounds", nb))
    print("project/levels/bounds_packed d4_w nb=%d: port %d, rescued %d" % (nb, nb, nb))


# ---- 2. the device forms give the packed forms' bytes -------------------------------------------------------------------------------
def _dev(ctx, fn, mats, slots, args, n_verdicts):
    """One _dev entry: upload, enqueue, synchronise, download. slots: result slots per system; returns (rows[nb, slots],
    verdict arrays, outs[nb, slots, cap_out, cols, 2])."""
    nb, rows, cols = mats.shape[:3]
    cap, cap_out = args["cap"], args["cap_out"]
    d_m, d_o, d_r = ctx.malloc(mats.nbytes), ctx.malloc(nb * slots * cap_out * cols * 8), ctx.malloc(nb * slots * 4)
    d_v = [ctx.malloc(nb * 4) for _ in range(n_verdicts)]
    try:
        ctx.upload(d_m, mats)
        fn(d_m, d_o, d_r, d_v)
        ctx.sync()
        outs = ctx.download(np.zeros((nb, slots, cap_out, cols, 2), dtype=np.int32), d_o)
        r = ctx.download(np.zeros((nb, slots), dtype=np.int32), d_r)
        v = [ctx.download(np.zeros(nb, dtype=np.int32), p) for p in d_v]
    finally:
        for p in [d_m, d_o, d_r] + d_v:
            ctx.free(p)
    assert (r >= 0).all() and (r <= cap_out).all()
    return r, v, outs


def test_the_device_forms_give_the_packed_forms_bytes(ctx, lq, port):
    from xpoly_amd.lineq import bounds_dev, levels_dev, project_dev
    # project_dev: d5_k (rhs_idx < cols - 1)
    mats, n = rq.family("d5_k"), 5
    nb, rows, cols = mats.shape[:3]
    el = rq.elim_of(n)
    p = pc.plan_view(nb, rows, cols)
    args = dict(cap=p["cap"], cap_out=p["cap_out"])
    ok, steps, res = lq.project_packed(mats, n, el)
    r, (dok, dsteps), outs = _dev(ctx, lambda m, o, rr, v: project_dev(ctx, nb, m, rows, cols, n, el, False, p["cap"], p["cap_out"], o, rr, *v),
                                  mats, 1, args, 2)
    assert np.array_equal(ok, dok) and np.array_equal(steps, dsteps) and (ok == 1).all()
    assert all(rows_equal(res[b], outs[b, 0, : r[b, 0]]) for b in range(nb))
    _, rescues = rq.want_project(port, mats, n)
    print("project_dev d5_k: packed %d, rescued %d" % (nb, sum(x > 0 for x in rescues)))
    assert all(x > 0 for x in rescues)
    # levels_dev: d4_w
    mats, n = rq.family("d4_w"), 4
    nb, rows, cols = mats.shape[:3]
    el = rq.elim_of(n)
    p = lc.plan_view(nb, rows, cols, n - 1)
    args = dict(cap=p["cap"], cap_out=p["cap_out"])
    ok, steps, levels = lq.levels_packed(mats, n, el)
    r, (dok, dsteps), outs = _dev(ctx, lambda m, o, rr, v: levels_dev(ctx, nb, m, rows, cols, n, el, False, p["cap"], p["cap_out"], o, rr, *v),
                                  mats, n - 1, args, 2)
    assert np.array_equal(ok, dok) and np.array_equal(steps, dsteps) and (ok == 1).all()
    assert all(rows_equal(levels[b][k], outs[b, k, : r[b, k]]) for b in range(nb) for k in range(n - 1))
    _, rescues = rq.want_levels(port, mats, n)
    print("levels_dev d4_w: packed %d, rescued %d" % (nb, sum(x > 0 for x in rescues)))
    assert all(x > 0 for x in rescues)
    # bounds_dev: d5_w
    mats, n = rq.family("d5_w"), 5
    nb, rows, cols = mats.shape[:3]
    p = bc.plan_view(nb, rows, cols, n)
    args = dict(cap=p["cap"], cap_out=p["cap_out"])
    ok, chain, steps, bounds = lq.bounds_packed(mats, n)
    r, (dok, dchain, dsteps), outs = _dev(ctx, lambda m, o, rr, v: bounds_dev(ctx, nb, m, rows, cols, n, p["cap"], p["cap_out"], o, rr, *v),
                                          mats, n, args, 3)
    assert np.array_equal(ok, dok) and np.array_equal(chain, dchain) and np.array_equal(steps, dsteps) and (ok == 1).all()
    assert all(rows_equal(bounds[b][j], outs[b, j, : r[b, j]]) for b in range(nb) for j in range(n))
    _, rescues = rq.want_bounds(port, mats, n)
    print("bounds_dev d5_w: packed %d, rescued %d" % (nb, sum(x > 0 for x in rescues)))
    assert all(x > 0 for x in rescues)


# ---- 3. the ragged entries on the mixed list --------------------------------------------------------------------------------------
def _classes(names, mats):
    """{(name, shape): [indices]} -- the systems one uniform call takes."""
    out = {}
    for b, (name, m) in enumerate(zip(names, mats)):
        out.setdefault((name, m.shape), []).append(b)
    return out


@pytest.mark.parametrize("cap", [0, PAST])
def test_the_ragged_chains_on_the_mixed_list(lq, port, ref_or_none, cap):
    """Depths 3, 4 and 5, both coefficient ranges and three exact gen.random_system systems in one envelope: every system's
    answer is the checker's and the uniform call's at the same capacities -- a rescued neighbour does not disturb an exact one."""
    mats, nvs, elims, names = rq.mixed_list()
    shape = ([m.shape[0] for m in mats], [m.shape[1] for m in mats], list(nvs), elims)
    for levels, call, uniform, want_fn, check in ((False, lq.project_ragged, lq.project_packed, rc.want_project, _check_project),
                                                  (True, lq.levels_ragged, lq.levels_packed, rc.want_levels, _check_levels)):
        p = rc.plan_view(*shape, levels, cap, cap)
        assert (p["cap_lds"] < p["cap"]) if cap else (p["cap_lds"] == p["cap"]), p
        t = Tally("%s_ragged mixed %s" % ("levels" if levels else "project", "past 12 KB" if cap else "all LDS"))
        got = call(mats, nvs, elims, cap_rows=cap, cap_out_rows=cap)
        route = lq.ragged_last_route()
        assert route["launches"] == 1 and route["cap_lds"] == p["cap_lds"]
        counts, want = [], []
        for b in range(len(mats)):
            w, r = rq.counted(port, (lc.stepped_levels if levels else pc.stepped), port, mats[b], nvs[b], elims[b], False, p["cap"], p["cap_out"])
            want.append(w); counts.append(r)
        check(got, want, ("ragged", levels, cap))
        t.port, t.rescued = len(mats), sum(r > 0 for r in counts)
        assert all(r == 0 for r, nm in zip(counts, names) if nm == "exact") and t.rescued >= 15
        assert all(w[0] == 1 for w, nm in zip(want, names) if nm != "exact")
        if ref_or_none:
            check(got, want_fn(ref_or_none, mats, nvs, elims, False, p["cap"], p["cap_out"]), ("ragged", levels, cap, "ref"))
            t.ref = len(mats)
        t.done(ref_or_none)
        for (name, shp), idx in _classes(names, mats).items():
            cls = np.stack([mats[b] for b in idx])
            u = uniform(cls, nvs[idx[0]], elims[idx[0]], cap_rows=p["cap"], cap_out_rows=p["cap_out"])
            assert [got[0][b] for b in idx] == u[0].tolist() and [got[1][b] for b in idx] == u[1].tolist(), (name, levels)
            if levels:
                assert all(rows_equal(got[2][b][k], u[2][i][k]) for i, b in enumerate(idx) for k in range(len(elims[b]))), name
            else:
                assert all(rows_equal(got[2][b], u[2][i]) for i, b in enumerate(idx)), name


@pytest.mark.parametrize("cap", [0, PAST])
def test_the_ragged_bounds_on_the_mixed_list(lq, port, ref_or_none, cap):
    mats, nvs, _, names = rq.mixed_list()
    p = brc.plan_view([m.shape[0] for m in mats], [m.shape[1] for m in mats], list(nvs), cap, cap)    # d4_k, d5_k: rhs_idx < cols - 1
    assert (p["cap_lds"] < p["cap"]) if cap else (p["cap_lds"] == p["cap"]), p
    t = Tally("bounds_ragged mixed %s" % ("past 12 KB" if cap else "all LDS"))
    got = lq.bounds_ragged(mats, rhs_idx=nvs, cap_rows=cap, cap_out_rows=cap)
    route = lq.bounds_ragged_last_route()
    assert route["launches"] == 1 and route["cap_lds"] == p["cap_lds"]
    pairs = [rq.counted(port, bc.chains, port, mats[b], nvs[b], p["cap"], p["cap_out"]) for b in range(len(mats))]
    want, counts = [w for w, _ in pairs], [r for _, r in pairs]
    _check_bounds(got, want, ("bounds ragged", cap))
    t.port, t.rescued = len(mats), sum(r > 0 for r in counts)
    assert all(r == 0 for r, nm in zip(counts, names) if nm == "exact") and t.rescued == 18
    assert all(w[0] == 1 for w, nm in zip(want, names) if nm != "exact")
    if ref_or_none:
        _check_bounds(got, brc.want(ref_or_none, mats, nvs, p["cap"], p["cap_out"]), ("bounds ragged", cap, "ref"))
        t.ref = len(mats)
    t.done(ref_or_none)
    for (name, shp), idx in _classes(names, mats).items():
        u = lq.bounds_packed(np.stack([mats[b] for b in idx]), nvs[idx[0]], cap_rows=p["cap"], cap_out_rows=p["cap_out"])
        assert all(np.array_equal(got[k][idx], u[k]) for k in range(3)), name
        assert all(rows_equal(got[3][b][j], u[3][i][j]) for i, b in enumerate(idx) for j in range(nvs[b])), name


# ---- 4. the hulls -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("caps", [(64, 64, 256), (PAST, PAST, 1000)])
def test_the_hulls_of_rescued_members(lq, port, ref_or_none, caps):
    """Groups of 1, 2 and 5 rescued nests and one with an empty nest in the middle: hull_ragged and project_union_ragged, union
    and intersection. The group with the empty member gets that member's verdict and no rows (the stated deviation: the
    reference goes on with stale bounds); the others are the composition's. (64, 64, 256): every group's gather at home in
    LDS; (256, 256, 1000): the larger groups' in the device slots of k_group_reduce."""
    groups, rhss, names = rq.groups()
    sizes, rows, cols, rhs = hc.shapes_of(groups, rhss)
    elims = [[rq.elim_of(r)] * len(g) for g, r in zip(groups, rhss)]
    flat = [e for g in elims for e in g]
    for union, pl in ((False, hc.plan_view(sizes, rows, cols, rhs, None, *caps)), (True, hc.plan_view(sizes, rows, cols, rhs, flat, *caps))):
        p, homes, _ = pl
        assert (hc.HOME_DEVICE in homes) if caps[2] == 1000 else (set(homes) == {hc.HOME_LDS}), (union, homes)
        kw = dict(cap_rows=p["cap"], cap_out_rows=p["cap_out"], cap_hull=p["cap_hull"])
        for flag in (False, True):
            t = Tally("%s %s caps %s" % ("project_union_ragged" if union else "hull_ragged", "intersect" if flag else "union", caps))
            if union:
                got = lq.project_union_ragged(groups, rhss, elims, flag, False, *caps)
                want, counts = rq.want_unions(port, flag, **kw)
                rwant = rq.want_unions(ref_or_none, flag, **kw)[0] if ref_or_none else None
            else:
                got = lq.hull_ragged(groups, rhss, flag, *caps)
                want, counts = rq.want_hulls(port, flag, **kw)
                rwant = rq.want_hulls(ref_or_none, flag, **kw)[0] if ref_or_none else None
            route = lq.hull_ragged_last_route()
            assert (route["producer_launches"], route["launches"]) == (1, 1)
            hc.same(got, want, t.what)
            e = names.index("with empty")
            assert (got[0][e], got[1][e]) == (0, 1) and got[4][e].shape[0] == 0, t.what
            assert all(got[0][g] == 1 and got[4][g].shape[0] > 0 for g in range(len(groups)) if g != e), (t.what, got[0])
            t.port, t.rescued = len(groups), sum(r > 0 for r in counts)
            assert t.rescued == len(groups)
            if rwant:
                hc.same(got, rwant, t.what + " ref"); t.ref = len(groups)
            t.done(ref_or_none)


# ---- 5. the transformed nests ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("mode", [0, 1])
def test_the_transformed_nests(lq, port, ref_or_none, n, mode):
    """Every T of lineq_rescue_cases.tmats -- the skews of 75 000, the identity, the T whose determinant approximates -- against
    (30 000, 70 000) nests: one nest per T, then the shared nest, at the default capacities and past the 12 KB layout; mode 1
    takes the same matrices as multipliers. The answers are lineq_transform_cases.transformed's. exact_check of that module is
    NOT used: it states T^-1 * T == I and level0 * T == A in exact fractions, which no longer holds once the checker (and the
    reference) have approximated a cell of the product -- here the checker's bits are the specification."""
    names = list(rq.tmats(n))
    ts = np.stack([rq.tmats(n)[k] for k in names])
    nests = rq.transform_nests(n, len(names))
    for cap in (0, PAST):
        for shared in (False, True):
            a = nests[:1] if shared else nests
            p = tc.plan_view(len(ts), nests[0].shape[0], nests[0].shape[1], n, cap, 0)
            assert (p["cap_lds"] < p["cap"]) if cap else (p["cap_lds"] == p["cap"]), (n, cap, p)
            t = Tally("transform_levels_packed depth %d mode %d %s %s" % (n, mode, "shared nest" if shared else "one nest per T",
                                                                          "past 12 KB" if cap else "all LDS"))
            got = lq.transform_levels_packed(a[0] if shared else a, ts, n, mode=mode, shared_nest=shared, cap_rows=cap)
            assert lq.transform_last_route()["launches"] == 1 and lq.transform_last_route()["cap_lds"] == p["cap_lds"]
            pairs = [(a[0 if shared else b], ts[b]) for b in range(len(ts))]
            want, counts = rq.want_transformed(port, pairs, mode, p["cap"], p["cap_out"])
            tc.check(got, want, (n, mode, shared, cap, "port"))
            t.port, t.rescued = len(ts), sum(r > 0 for r in counts)
            if ref_or_none:
                tc.check(got, rq.want_transformed(ref_or_none, pairs, mode, p["cap"], p["cap_out"])[0], (n, mode, shared, cap, "ref"))
                t.ref = len(ts)
            t.done(ref_or_none)
            d = names.index("det_rescued")
            if mode == 0:                                    # kind, det and the multiplier are the checker's, the approximated det too
                for b, w in enumerate(want):
                    assert got[2][b] == w[2] and tuple(got[3][b]) == tuple(w[3]) and np.array_equal(got[4][b], w[4]), (n, names[b])
                assert got[2][d] in (1, 2) and counts[d] > 0 and all(got[2][b] == 0 for b in range(len(ts)) if b != d)
                skews = [b for b, k in enumerate(names) if k.startswith("skew")]
                assert all(counts[b] > 0 and want[b][0] == 1 for b in skews)
            else:
                assert got[3] is None and not got[2].any() and np.array_equal(got[4], ts)
