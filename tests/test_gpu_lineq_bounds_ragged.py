"""GPU parity of the ragged calcBound entry point (xpg_lineq_bounds_batch_ragged_rat32: every elimination chain of systems of
MIXED shapes in ONE launch of k_calc_bound_ragged) against the CPU checker's fme applied chain by chain at the call's
capacities (tests/lineq_bounds_ragged_cases.py want), against the reference's own build where it is present, and against the
uniform call of every shape class at the same capacities. Bit-exact: nothing is compared with a tolerance. The facts of the
batch the cases rest on -- which classes fail how, which steps have which home, which verdicts a capacity gives -- are
asserted on the checker's answers and the plan view BEFORE anything is asserted of the device."""
import subprocess

import numpy as np
import pytest

import lineq_bounds_cases as bc
import lineq_bounds_ragged_cases as rc
from lineq_bounds_ragged_cases import XPG_ERR_SHAPE, XPG_ERR_UNSUPPORTED, rows_equal
from tools import gen

pytestmark = pytest.mark.gpu

CAP = 512


@pytest.fixture(scope="module")
def lq(ctx):
    from xpoly_amd.lineq import Lineq
    return Lineq(ctx)


@pytest.fixture(scope="module")
def batch():
    return rc.mixed_batch()


@pytest.fixture(scope="module")
def wants(port, batch):
    """The chain checker's answers at cap 512 / 512, 512 / 40 and 256 / 256, computed once and left unchanged."""
    mats, nvs, _ = batch
    return {caps: rc.want(port, mats, nvs, *caps) for caps in ((512, 512), (512, 40), (256, 256))}


@pytest.fixture(scope="module")
def needs(port, batch):
    """[(needs of every step entered, needs of the prefix steps among them)] per system, run without a capacity."""
    mats, nvs, _ = batch
    return [bc.step_needs(port, mats[b], nvs[b]) for b in range(len(mats))]


def _shape(mats):
    return [m.shape[0] for m in mats], [m.shape[1] for m in mats]


def _same(got, want, what=""):
    ok, chain, steps, bounds = got
    assert len(ok) == len(want) == len(bounds)
    for b, (wok, wchain, wsteps, wb) in enumerate(want):
        assert (ok[b], chain[b], steps[b]) == (wok, wchain, wsteps), (what, b, ok[b], chain[b], steps[b], wok, wchain, wsteps)
        assert len(bounds[b]) == len(wb) and all(rows_equal(g, w) for g, w in zip(bounds[b], wb)), (what, b)
        assert all(g.shape[1:] == (wb[0].shape[1], 2) for g in bounds[b]), (what, b)


def _by_class(cls, c):
    return [b for b, k in enumerate(cls) if k == c]


def test_the_batch_is_the_one_the_cases_rest_on(batch, wants, needs):
    """No device: the generator's batch, the checker's answers and the plan view."""
    mats, nvs, cls = batch
    rows, cols = _shape(mats)
    assert len(mats) == 108 and [len(_by_class(cls, c)) for c in range(6)] == [12, 12, 12, 12, 12, 48]
    assert {(m.shape[0], m.shape[1] - 1) for m in mats} == {(r, nv) for r, nv, _ in rc.CLASSES}
    plan = rc.plan_view(rows, cols, None, CAP)
    assert (plan["cols"], plan["rows"], plan["cap_lds"]) == (6, 9, 86)               # widest: (4, 5); tallest: (9, 4)
    assert rc.plan_view(rows, cols, None, 256)["cap_lds"] == 43
    w = wants[(512, 512)]
    verdicts = lambda c, ww=w: {ww[b][:3] for b in _by_class(cls, c)}
    assert verdicts(0) == {(1, -1, 0)} and verdicts(4) == {(1, -1, 0)}
    for c in (1, 2, 3):
        assert verdicts(c) == {(0, 0, 0), (1, -1, 0)}, c
    v9 = [w[b][:3] for b in _by_class(cls, 5)]
    assert sum(v == (1, -1, 0) for v in v9) == 30 and sum(v[0] == 0 for v in v9) == 18 and all(v[0] >= 0 for v in v9)
    assert {v[1:] for v in v9 if v[0] == 0} == {(0, 0), (0, 1), (0, 2)}
    tall = lambda c: max(x.shape[0] for b in _by_class(cls, c) if w[b][0] == 1 for x in w[b][3])
    assert [tall(c) for c in (3, 0, 4, 5)] == [4, 3, 3, 2] and max(tall(c) for c in range(6)) == 4
    # the homes of the steps: only the (9, 4) systems have a step above 86 rows
    for cap, cap_lds, dev, dev_prefix in ((512, 86, 13, 3), (256, 43, 19, 6)):
        all_needs = [n for b in range(108) for n in needs[b][0].values()]
        assert all(n <= cap_lds for b in range(108) if cls[b] != 5 for n in needs[b][0].values())
        assert sum(cap_lds < n <= cap for n in all_needs) == dev, cap
        assert sum(cap_lds < n <= cap for b in range(108) for n in needs[b][1]) == dev_prefix, cap
        if cap == 512:
            assert sum(n <= cap_lds for b in _by_class(cls, 5) for n in needs[b][0].values()) == 486
            assert all(n <= cap for n in all_needs)                                  # no capacity verdict at 512
    short = wants[(256, 256)]
    cap_v = sorted(s[:3] for s in short if s[0] < 0)
    assert cap_v == [(-379, 1, 2), (-281, 3, 2)], cap_v
    assert all(short[b][:3] == w[b][:3] for b in range(108) if short[b][0] >= 0) and all(cls[b] == 5 for b in range(108) if short[b][0] < 0)


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
def test_every_system_equals_the_chain_checker(lq, batch, wants):
    mats, nvs, _ = batch
    got = lq.bounds_ragged(mats, cap_rows=CAP)
    route = lq.bounds_ragged_last_route()
    assert route["launches"] == 1 and route["steps"] == sum((nv - 1) * (nv + 2) // 2 for nv in nvs)
    _same(got, wants[(512, 512)])
    assert all(c == -1 and s == 0 for o, c, s in zip(*got[:3]) if o == 1)


def test_every_system_equals_the_real_reference(lq, ref, batch):
    """The same batch against the reference's own Lineq::fme, chain by chain, where its build is present."""
    mats, nvs, _ = batch
    _same(lq.bounds_ragged(mats, cap_rows=CAP), rc.want(ref, mats, nvs, CAP, CAP))


# ---- 2. against the uniform call -----------------------------------------------------------------------------------------------
def test_every_class_equals_its_uniform_call(lq, batch, wants):
    mats, nvs, cls = batch
    ok, chain, steps, bounds = lq.bounds_ragged(mats, cap_rows=CAP, cap_out_rows=40)
    _same((ok, chain, steps, bounds), wants[(512, 40)])
    for c, (_, nv, _) in enumerate(rc.CLASSES):
        idx = _by_class(cls, c)
        uok, uchain, usteps, ub = lq.bounds_packed(np.stack([mats[b] for b in idx]), nv, cap_rows=CAP, cap_out_rows=40)
        assert np.array_equal(ok[idx], uok) and np.array_equal(chain[idx], uchain) and np.array_equal(steps[idx], usteps), c
        for i, b in enumerate(idx):
            assert len(bounds[b]) == nv and all(rows_equal(bounds[b][j], ub[i][j]) and bounds[b][j].shape == ub[i][j].shape for j in range(nv)), (c, b)
    # rhs_idx=None is the explicit last column
    ex = lq.bounds_ragged(mats, rhs_idx=nvs, cap_rows=CAP, cap_out_rows=40)
    assert all(np.array_equal(a, b) for a, b in zip((ok, chain, steps), ex[:3]))
    assert all(rows_equal(x, y) for b in range(108) for x, y in zip(bounds[b], ex[3][b]))
    # the (6, 4) class with the constant in column cols - 2, among the others with theirs in the last
    idx = _by_class(cls, 3)
    rhs = [nv - 1 if k == 3 else nv for nv, k in zip(nvs, cls)]
    got = lq.bounds_ragged(mats, rhs_idx=rhs, cap_rows=CAP, cap_out_rows=40)
    uok, uchain, usteps, ub = lq.bounds_packed(np.stack([mats[b] for b in idx]), 3, cap_rows=CAP, cap_out_rows=40)
    assert np.array_equal(got[0][idx], uok) and np.array_equal(got[1][idx], uchain) and np.array_equal(got[2][idx], usteps)
    assert all(len(got[3][b]) == 3 and all(rows_equal(got[3][b][j], ub[i][j]) for j in range(3)) for i, b in enumerate(idx))
    others = [b for b in range(108) if cls[b] != 3]
    assert all(got[0][b] == ok[b] and all(rows_equal(x, y) for x, y in zip(got[3][b], bounds[b])) for b in others)


# (rows, nv, systems): a small nest, and the class whose steps' results lie on both sides of cap_lds (tests/test_gpu_lineq_bounds.py)
TWINS = [(8, 5, 5), (9, 4, 48)]


@pytest.mark.parametrize("rows,nv,nb", TWINS)
def test_one_shape_gives_the_same_bits_through_the_uniform_and_the_ragged_kernel(lq, port, rows, nv, nb):
    """k_calc_bound_batch and k_calc_bound_ragged run ONE walk (lineq_kernels.hip.h w_calc_bound_walk) through two views of a
    system: a batch whose systems all share one shape gets the same plan from both calls and must come back bit for bit the
    same -- rows, their counts, ok, chain and steps."""
    mats = rc.class_batch(rows, nv, nb)
    cap_lds = rc.plan_view([rows] * nb, [nv + 1] * nb, None, CAP)["cap_lds"]
    needs, prefix = [], []
    for m in mats:
        n, p = bc.step_needs(port, m, nv)
        needs += list(n.values()); prefix += p
    assert max(needs) <= CAP
    if rows == 9:                                            # results in LDS, on the seat's sides and built in its hold slot
        assert any(n <= cap_lds for n in needs) and sum(n > cap_lds for n in needs) >= 4 and sum(n > cap_lds for n in prefix) >= 2
    uok, uchain, usteps, ub = lq.bounds_packed(mats, nv, cap_rows=CAP)
    assert lq.bounds_last_route()["cap_lds"] == cap_lds
    rok, rchain, rsteps, rb = lq.bounds_ragged(list(mats), cap_rows=CAP)
    assert lq.bounds_ragged_last_route()["cap_lds"] == cap_lds
    assert np.array_equal(uok, rok) and np.array_equal(uchain, rchain) and np.array_equal(usteps, rsteps), (uok, rok, uchain, rchain, usteps, rsteps)
    assert (uok == 1).any()
    for b in range(nb):
        assert len(rb[b]) == nv and all(ub[b][j].shape == rb[b][j].shape and np.array_equal(ub[b][j], rb[b][j]) for j in range(nv)), b


# ---- 3. the route ----------------------------------------------------------------------------------------------------------------
def test_one_launch_and_the_route_is_the_restated_plan(lq, batch):
    mats, _, _ = batch
    rows, cols = _shape(mats)
    for cap, cap_out in ((CAP, 0), (CAP, 40), (256, 8), (0, 0)):
        lq.bounds_ragged(mats, cap_rows=cap, cap_out_rows=cap_out)
        route = lq.bounds_ragged_last_route()
        planned = rc.plan(rows, cols, None, cap, cap_out)
        assert route == {k: planned[k] for k in rc.ROUTE_KEYS}, (cap, cap_out, route, planned)
        assert route["launches"] == 1 and route["grid"] == 108 and route["groups"] == 1
        # the LDS of a workgroup is the envelope's -- what a uniform batch of 6 columns takes at this capacity -- and so are the seats
        assert route["sys_lds"] == bc.plan(108, 9, 6, 5, cap, cap_out)["sys_lds"]
        assert route["seat_bytes"] == route["grid"] * 3 * planned["cap"] * 6 * 8


# ---- 4. order ----------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_order_of_the_systems(lq, batch, wants):
    mats, nvs, cls = batch
    w = wants[(512, 512)]
    wide = _by_class(cls, 4)[0]
    rest = [b for b in range(108) if b != wide]
    perm = np.random.default_rng(5).permutation(108).tolist()
    for order in (perm, [wide] + rest, rest + [wide], list(range(107, -1, -1))):
        got = lq.bounds_ragged([mats[b] for b in order], cap_rows=CAP)
        assert lq.bounds_ragged_last_route()["launches"] == 1
        _same(got, [w[b] for b in order], str(order[:3]))


# ---- 5. both homes -----------------------------------------------------------------------------------------------------------------
def test_both_homes_of_a_steps_result_in_one_launch(lq, batch, wants, needs):
    mats, nvs, cls = batch
    rows, cols = _shape(mats)
    cap_lds = rc.plan_view(rows, cols, None, CAP)["cap_lds"]
    assert cap_lds == 86
    all_needs = [n for b in range(108) for n in needs[b][0].values()]
    prefix = [n for b in range(108) for n in needs[b][1]]
    assert sum(cap_lds < n <= CAP for n in all_needs) == 13 and sum(cap_lds < n <= CAP for n in prefix) == 3
    assert sum(n <= cap_lds for b in _by_class(cls, 5) for n in needs[b][0].values()) == 486
    got = lq.bounds_ragged(mats, cap_rows=CAP)
    assert lq.bounds_ragged_last_route()["cap_lds"] == cap_lds
    _same(got, wants[(512, 512)])


# ---- 6. capacity -------------------------------------------------------------------------------------------------------------------
def test_capacity_is_reported_per_chain_and_step_and_the_rest_is_packed(lq, port, batch, wants):
    mats, nvs, cls = batch
    short = wants[(256, 256)]
    hit = [b for b in range(108) if short[b][0] < 0]
    assert sorted(short[b][:3] for b in hit) == [(-379, 1, 2), (-281, 3, 2)]
    got = lq.bounds_ragged(mats, cap_rows=256)
    _same(got, short, "cap 256")
    for b in hit:
        assert -got[0][b] == bc.chain(port, mats[b], nvs[b], short[b][1])[3][short[b][2]] > 256   # the need of that chain's step
        assert all(x.shape[0] == 0 for x in got[3][b])
    assert sum(x.shape[0] for b in range(108) for x in got[3][b]) == sum(x.shape[0] for b in range(108) if b not in hit for x in wants[(512, 512)][b][3])
    # once more with the largest need reported: case 1's answers
    need = int(-got[0].min())
    assert need == 379
    _same(lq.bounds_ragged(mats, cap_rows=need), wants[(512, 512)], "need")


def test_a_short_result_slot_and_a_first_failure_above_chain_zero(lq, port, batch, wants):
    mats, nvs, cls = batch
    full = wants[(512, 512)]
    want3 = rc.want(port, mats, nvs, CAP, 3)
    got3 = lq.bounds_ragged(mats, cap_rows=CAP, cap_out_rows=3)
    hit = 0
    for b, w in enumerate(full):
        over = [j for j, x in enumerate(w[3]) if x.shape[0] > 3] if w[0] == 1 else []
        if over:
            hit += 1
            assert cls[b] == 3 and w[3][over[0]].shape[0] == 4
            assert (got3[0][b], got3[1][b], got3[2][b]) == (-4, over[0], nvs[b] - 1), b
            assert all(x.shape[0] == 0 for x in got3[3][b]), b
        else:
            assert want3[b][:3] == w[:3], b
    assert hit > 0
    _same(got3, want3, "cap_out 3")
    # ABOVE_ZERO among the others: chains 0 and 1 run, chain 2 needs 651 rows at its last step, at both capacities
    one = rc.above_zero()
    for cap in (CAP, 256):
        w1 = bc.chains(port, one, 4, cap, cap)
        assert w1[:3] == rc.ABOVE_ZERO[3]
        k = 17
        got = lq.bounds_ragged(mats[:k] + [one] + mats[k:], cap_rows=cap)
        base = wants[(cap, cap)]
        _same(got, base[:k] + [w1] + base[k:], "above zero, cap %d" % cap)
        assert (got[0][k], got[1][k], got[2][k]) == (-651, 2, 2)


# ---- 7. seats above the grid ---------------------------------------------------------------------------------------------------------
def test_seats_are_reused_above_the_grid(lq, batch, wants):
    mats, nvs, cls = batch
    nb = 4096 + 300
    # workgroup j takes system j and then system 4096 + j: 4096 = 37 * 108 + 100, so the second system of a seat is the one 100
    # further on in the batch -- of another class than the first for most seats
    src = [b % 108 for b in range(nb)]
    pairs = {(cls[src[j]], cls[src[4096 + j]]) for j in range(300)}
    assert len({p for p in pairs if p[0] != p[1]}) >= 10, pairs
    tiled = [mats[i] for i in src]
    ok, chain, steps, bounds = lq.bounds_ragged(tiled, cap_rows=CAP, copy=False)
    route = lq.bounds_ragged_last_route()
    planned = rc.plan(*_shape(tiled), None, CAP)
    assert route == {k: planned[k] for k in rc.ROUTE_KEYS}, (route, planned)
    assert route["launches"] == 1 and nb > route["grid"] * route["groups"] == 4096
    assert route["seat_bytes"] == 4096 * 3 * CAP * 6 * 8
    w = wants[(512, 512)]
    assert np.array_equal(ok, [w[i][0] for i in src]) and np.array_equal(chain, [w[i][1] for i in src])
    assert np.array_equal(steps, [w[i][2] for i in src])
    for b in range(nb):
        wb = w[src[b]][3]
        assert len(bounds[b]) == len(wb) and all(rows_equal(bounds[b][j], wb[j]) for j in range(len(wb))), b


# ---- 8. no systems, views, the two ways down, the caller's buffer ----------------------------------------------------------------------
def _c_call(ctx, mats, cap=0, cap_out=0, outs=None, outs_cap=0, rhs=None, nb=None, want_view=False):
    import ctypes as C
    from xpoly_amd._capi import lib, vp
    n = len(mats)
    flat = np.ascontiguousarray(np.concatenate([m.reshape(-1, 2) for m in mats]))
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    rows, cols = i32([m.shape[0] for m in mats]), i32([m.shape[1] for m in mats])
    off = np.zeros(n + 1, dtype=np.int64); off[1:] = np.cumsum(rows.astype(np.int64) * cols)
    nres = int((cols - 1).sum())
    ooff = np.zeros(nres + 1, dtype=np.int64); orows = np.full(nres, -7, dtype=np.int32)
    ok = np.full(n, 7, dtype=np.int32); ch = np.full(n, 7, dtype=np.int32); st = np.full(n, -7, dtype=np.int32)
    view = C.c_void_p()
    code = lib().xpg_lineq_bounds_batch_ragged_rat32(
        ctx._h, C.c_int(n if nb is None else nb), vp(flat), vp(rows), vp(cols), vp(off), None if rhs is None else vp(i32(rhs)), C.c_int(cap),
        C.c_int(cap_out), vp(outs), C.c_longlong(outs_cap), C.byref(view) if want_view else None, vp(ooff), vp(orows), vp(ok), vp(ch), vp(st))
    return code, ooff, orows, ok, ch, st


def test_no_systems_views_and_both_ways_down(ctx, lq, batch, wants):
    mats, nvs, cls = batch
    ok0, chain0, steps0, b0 = lq.bounds_ragged([])
    assert len(ok0) == 0 and len(chain0) == 0 and len(steps0) == 0 and b0 == []      # (answered before the library is called)
    code, ooff, _, _, _, _ = _c_call(ctx, mats[:2], nb=0)
    assert code == 0 and ooff[0] == 0 and lq.bounds_ragged_last_route()["launches"] == 0
    # views equal copies (read before the next packed call)
    a = lq.bounds_ragged(mats, cap_rows=CAP)
    v = lq.bounds_ragged(mats, cap_rows=CAP, copy=False)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], v[:3]))
    assert all(rows_equal(x, y) for b in range(108) for x, y in zip(a[3][b], v[3][b]))
    # slots of 8 rows come down with the counts and are packed on the host; those of 512 rows are scanned and packed on the device
    small = lq.bounds_ragged(mats, cap_rows=CAP, cap_out_rows=8)
    assert lq.bounds_ragged_last_route()["out_bytes"] <= (512 << 10)
    smallv = lq.bounds_ragged(mats, cap_rows=CAP, cap_out_rows=8, copy=False)
    assert all(rows_equal(x, y) for b in range(108) for x, y in zip(small[3][b], smallv[3][b]))
    lq.bounds_ragged(mats, cap_rows=CAP)
    assert lq.bounds_ragged_last_route()["out_bytes"] > (512 << 10)
    _same(small, wants[(512, 512)], "small slots")                                   # (no result of the batch has more than 4 rows)
    _same(a, wants[(512, 512)], "large slots")
    # a sizing call, then a buffer of exactly that size; one cell short is refused with offsets, counts and verdicts filled
    for cap_out in (8, 0):
        code, ooff, orows, ok, ch, st = _c_call(ctx, mats, CAP, cap_out)
        assert code == 0 and ooff[-1] > 0 and (orows >= 0).all()
        total = int(ooff[-1])
        out = np.zeros((total, 2), dtype=np.int32)
        code, ooff2, orows2, ok2, ch2, st2 = _c_call(ctx, mats, CAP, cap_out, outs=out, outs_cap=total - 1)
        assert code == XPG_ERR_SHAPE and lq.bounds_ragged_last_route()["launches"] == 1
        assert np.array_equal(ooff2, ooff) and np.array_equal(orows2, orows) and np.array_equal(ok2, ok) and np.array_equal(ch2, ch) and np.array_equal(st2, st)
        assert np.array_equal(ok, a[0]) and np.array_equal(ch, a[1]) and np.array_equal(st, a[2])
        code, ooff3, orows3, _, _, _ = _c_call(ctx, mats, CAP, cap_out, outs=out, outs_cap=total)
        assert code == 0 and np.array_equal(ooff3, ooff)
        r = 0
        for b in range(108):
            for j in range(nvs[b]):
                assert rows_equal(out[ooff[r]: ooff[r + 1]].reshape(-1, nvs[b] + 1, 2), a[3][b][j]) and orows[r] == a[3][b][j].shape[0], (b, j)
                r += 1


# ---- 9. errors launch nothing ----------------------------------------------------------------------------------------------------------
def test_errors_launch_nothing(ctx, lq, batch):
    mats, nvs, cls = batch
    four = mats[:6]

    def call(**kw):
        code = _c_call(ctx, four, **kw)[0]
        assert lq.bounds_ragged_last_route()["launches"] == (1 if code == 0 else 0), (kw, code)
        return code

    good = [m.shape[1] - 1 for m in four]
    assert call() == 0 and call(rhs=good) == 0
    assert call(rhs=[0] + good[1:]) == XPG_ERR_SHAPE and call(rhs=good[:5] + [four[5].shape[1]]) == XPG_ERR_SHAPE   # rhs outside [1, cols)
    assert call(nb=-1) == XPG_ERR_SHAPE
    assert call(cap=32768) == XPG_ERR_UNSUPPORTED                                     # cap > 32767
    assert call(cap=4000) == XPG_ERR_UNSUPPORTED                                      # the envelope's layout over 160 KB
    assert call(cap=64) == 0


# ---- 10. the collector -----------------------------------------------------------------------------------------------------------------
def _run_collector(exe, systems, path):
    lines = ["%d" % len(systems)]
    for m, nv in systems:
        lines += ["%d %d %d" % (m.shape[0], m.shape[1], nv), " ".join(str(int(x)) for x in np.asarray(m).ravel())]   # num den, cell by cell
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert out[0] == "rc 0 0" and "mismatches 0" in out
    per = [ln.split() for ln in out if " ok " in ln]
    assert len(per) == len(systems) and all(p[6] == "1" for p in per)
    return [int(x) for x in out[1].split()[1:]], {p[2] for p in per}


def test_the_collector_bounds_nests_of_three_depths_in_one_call(port, batch, tmp_path):
    """tests/cxx/calc_bound_each.cpp in a child process: nests of depth 2, 4 and 5 with their rows, interleaved, through
    xpoly_amd::calc_bound_each and xpoly_amd::calc_bound_all, compared in there limit for limit and ok for ok. First a batch no
    step of which exceeds the first capacity (4 x most rows + 16; the collector's calls are replayed here on the checker): ONE
    library call, and the route afterwards is that of one launch over all systems. Then the same with the (9, 4) systems of this
    file's batch among them, one of whose steps needs more: the collector calls again with the need reported."""
    from test_lineq_bounds_ragged_host import build_collector
    exe = build_collector()
    mats, nvs, cls = batch
    calm = [b for b in range(108) if cls[b] in (1, 3, 4)]
    assert {nvs[b] for b in calm} == {2, 4, 5} and len(calm) == 36
    assert rc.collector_calls(port, [mats[b] for b in calm], [nvs[b] for b in calm]) == 1
    route, verdicts = _run_collector(exe, [(mats[b], nvs[b]) for b in calm], str(tmp_path / "calm.txt"))
    assert route == [1, len(calm), sum((nvs[b] - 1) * (nvs[b] + 2) // 2 for b in calm)] and verdicts == {"0", "1"}
    # a retry: the (9, 4) class among them
    tall = calm + [b for b in range(108) if cls[b] == 5]
    assert 2 <= rc.collector_calls(port, [mats[b] for b in tall], [nvs[b] for b in tall]) <= 3
    route, verdicts = _run_collector(exe, [(mats[b], nvs[b]) for b in tall], str(tmp_path / "tall.txt"))
    assert route == [1, len(tall), sum((nvs[b] - 1) * (nvs[b] + 2) // 2 for b in tall)] and verdicts == {"0", "1"}
