"""Batches of LPs beyond one CU's LDS (xpg_six_batch_hbm_*): one workgroup per LP on a tableau in device memory, everything
else of the LDS-resident kernel unchanged.

Checkers: the CPU restatement of the reference (oracle.checker.Port().six_solve with vc = -I; tests/batch_hbm_cases.py computes
each batch's answers once) and the unchanged single-problem route SIX.maxm / minm. Every comparison is exact: status, the
optimum's bits, the solution's bits. An LP is skipped only where the restatement itself returns -7, at most 4 per 256 LPs of a
case (none of the committed inputs does).

Shapes (tests/batch_hbm_cases.py SHAPES, as solved): 100 x 100, the first past LDS; 40 x 400 wide; 260 x 48 tall; 101 x 100 of
odd widest width. 40 x 300 still fits one CU's LDS, so it runs as a case that must take the LDS kernel, and as solved 300 x 40
-- a caller's 40 x 300 arrays under minm -- on the HBM route.

max_iter bounds each solve of an LP on its own (stage 1's auxiliary LP, then the LP's): a cap that cuts stage 1 short ends the
LP SIX_NO_PRI_FEASIBLE_SOL having made cap + 1 pivots, one that cuts the LP's own loop ends it SIX_TIME_OUT. Left alone, most
LPs of the signed families run ~28 000 pivots before the pair table closes the last column, so all cases but two are capped:
fp64 at 300 and 48 iterations, Rational (4.5 ms per pivot in the restatement) at 48 and 32 on 8 LPs."""
import numpy as np
import pytest

import batch_geometry as bg
import batch_hbm_cases as hc
from batch_hbm_cases import F64, RAT
from tools import gen

pytestmark = pytest.mark.gpu
XPG_ERR_UNSUPPORTED = -4
COUNT = 64                                  # fp64 LPs per case
F64_CASES = [(name, is_max) for name in hc.SHAPES for is_max in (True, False) if (name, is_max) != ("wide300dual", True)]
RAT_CASES = [("first", True, 48), ("first", False, 48), ("odd", True, 48), ("wide", False, 32), ("tall", True, 32)]
RAT_COUNT = 8
UNBOUNDED = ("first", True, (0, 4))         # LPs of the fp64 case that end SIX_UNBOUND after ~29 000 pivots, run without a cap
SUCC_COUNT = 16


def _solve(ctx, kind, is_max, leq, tg, max_iter=hc.NO_LIMIT):
    from xpoly_amd.six import six_batch_hbm, six_batch_hbm_last_route
    st, v, sol = six_batch_hbm(ctx, kind, is_max, tg, leq, max_iter=max_iter)
    return st, v, sol, six_batch_hbm_last_route()


def _singles(ctx, kind, is_max, leq, tg, idx, max_iter=hc.NO_LIMIT):
    from xpoly_amd.six import SIX
    six = SIX(ctx, kind)
    six.set_param(0, max_iter)
    vc = gen.vc_nonneg(leq.shape[2] - 1, kind == F64)
    return [(six.maxm if is_max else six.minm)(tg[i], vc, None, leq[i]) for i in idx]


def _compare(got, want, what):
    """got = (st, v, sol) arrays, want = the restatement's list. Returns the statuses seen; skips only -7."""
    st, v, sol = got
    skipped, seen = 0, []
    for i, w in enumerate(want):
        if w[0] == -7:
            skipped += 1
            continue
        assert hc.same_answer(st[i], v[i], sol[i], w), (what, i, st[i], v[i], w[:2])
        if st[i] != 0:
            assert not sol[i].any(), (what, i)                   # written on status 0 only
        seen.append(int(w[0]))
    assert skipped <= 4 * ((len(want) + 255) // 256), (what, skipped)
    return seen


def _cut_kinds(want, cap):
    """(LPs whose stage 1 the cap cut short, LPs whose own loop it cut short) by the restatement's status and pivot count."""
    return sum(1 for w in want if w[0] == 2 and w[3] >= cap), sum(1 for w in want if w[0] == 4)


@pytest.mark.parametrize("name,is_max", F64_CASES)
def test_fp64_batches_match_the_oracle_and_the_single_calls(ctx, name, is_max):
    """64 LPs per shape and direction under two caps; the first 6 also against their single calls; LP 0 again as nb = 1.
    Every shape is past the LDS limit but 40 x 300 (hc.LDS_SHAPES), which the rule keeps LDS-resident."""
    R, V = hc.SHAPES[name]
    leq, tg = hc.mixed_batch(F64, is_max, R, V, COUNT, hc.SEEDS.get(name, 0))
    on_lds = name in hc.LDS_SHAPES
    assert bg.solved_as(is_max, leq.shape[1], leq.shape[2]) == (R, V) and bg.lds_fits(F64, R, V) == on_lds
    for cap in (300, 48):
        want = hc.oracle_answers(name, F64, is_max, leq, tg, cap)
        st, v, sol, route = _solve(ctx, F64, is_max, leq, tg, cap)
        assert (route["lds"], route["hbm"]) == ((COUNT, 0) if on_lds else (0, COUNT)) and 1 <= route["grid"] <= COUNT, route
        seen = _compare((st, v, sol), want, (name, is_max, cap))
        stage1_cut, own_cut = _cut_kinds(want, cap)
        print("%s is_max=%d cap=%d statuses %s stage-1 cut %d own loop cut %d" % (name, is_max, cap, sorted(set(seen)), stage1_cut, own_cut))
        assert stage1_cut >= 8 and own_cut >= 2, (stage1_cut, own_cut)
        one = _singles(ctx, F64, is_max, leq, tg, range(6), cap)
        for i in range(6):
            assert hc.same_answer(st[i], v[i], sol[i], one[i]), (name, is_max, cap, i, st[i], one[i][:2])
    st1, v1, sol1, route = _solve(ctx, F64, is_max, leq[:1], tg[:1], 300)
    assert route == (dict(lds=1, hbm=0, grid=1) if on_lds else dict(lds=0, hbm=1, grid=1))
    assert hc.same_answer(st1[0], v1[0], sol1[0], hc.oracle_answers(name, F64, is_max, leq, tg, 300)[0])


@pytest.mark.parametrize("is_max", [True, False])
def test_fp64_lps_that_end_succ(ctx, is_max):
    """Block-diagonal LPs past the LDS limit whose every block the reference solves: status 0 and a non-zero optimum."""
    leq, tg = hc.succ_batch(is_max, SUCC_COUNT)
    R, V = bg.solved_as(is_max, leq.shape[1], leq.shape[2])
    assert not bg.lds_fits(F64, R, V)
    want = hc.oracle_answers("succ", F64, is_max, leq, tg)
    assert [w[0] for w in want] == [0] * SUCC_COUNT and all(float(w[1]) != 0.0 for w in want)
    st, v, sol, route = _solve(ctx, F64, is_max, leq, tg)
    assert route == dict(lds=0, hbm=SUCC_COUNT, grid=SUCC_COUNT)
    _compare((st, v, sol), want, ("succ", is_max))
    one = _singles(ctx, F64, is_max, leq, tg, range(4))
    for i in range(4):
        assert hc.same_answer(st[i], v[i], sol[i], one[i]), (is_max, i, st[i], one[i][:2])


def test_fp64_unbounded_lps_without_a_cap(ctx):
    """Two LPs that run to their natural end -- SIX_UNBOUND once the pair table has closed every column, ~29 000 pivots."""
    name, is_max, idx = UNBOUNDED
    R, V = hc.SHAPES[name]
    leq, tg = hc.mixed_batch(F64, is_max, R, V, COUNT, 0)
    leq, tg = np.ascontiguousarray(leq[list(idx)]), np.ascontiguousarray(tg[list(idx)])
    want = hc.oracle_answers("unbounded", F64, is_max, leq, tg)
    assert [w[0] for w in want] == [1, 1] and min(w[3] for w in want) > 20000
    st, v, sol, route = _solve(ctx, F64, is_max, leq, tg)
    assert route == dict(lds=0, hbm=2, grid=2)
    _compare((st, v, sol), want, "unbounded")


def test_a_workgroup_reuses_its_slot_after_lps_that_ended_early(ctx):
    """nb >= 2 x grid + 3 with mixed statuses: every workgroup takes at least two LPs, most take three, and the LPs of a
    workgroup end after anything from 2 pivots to the cap."""
    R, V = hc.SHAPES["first"]
    leq, tg = hc.mixed_batch(F64, False, R, V, COUNT, 0)
    want = hc.oracle_answers("first", F64, False, leq, tg, 48)
    assert len({w[0] for w in want}) >= 3 and min(w[3] for w in want) <= 2 and max(w[3] for w in want) >= 48
    nb = 2 * 1024 + 3
    pick = np.arange(nb) % COUNT
    st, v, sol, route = _solve(ctx, F64, False, np.ascontiguousarray(leq[pick]), np.ascontiguousarray(tg[pick]), 48)
    assert route["hbm"] == nb and nb >= 2 * route["grid"] + 3, route
    _compare((st, v, sol), [want[i] for i in pick], "reuse")


@pytest.mark.parametrize("name,is_max,cap", RAT_CASES)
def test_rational_batches_match_the_oracle_and_the_single_calls(ctx, name, is_max, cap):
    R, V = hc.SHAPES[name]
    leq, tg = hc.mixed_batch(RAT, is_max, R, V, RAT_COUNT, 0)
    assert not bg.lds_fits(RAT, R, V)
    want = hc.oracle_answers(name, RAT, is_max, leq, tg, cap)
    st, v, sol, route = _solve(ctx, RAT, is_max, leq, tg, cap)
    assert route == dict(lds=0, hbm=RAT_COUNT, grid=RAT_COUNT)
    seen = _compare((st, v, sol), want, (name, is_max, cap))
    assert set(seen) >= {2, 4}, seen
    one = _singles(ctx, RAT, is_max, leq, tg, range(2), cap)
    for i in range(2):
        assert hc.same_answer(st[i], v[i], sol[i], one[i]), (name, is_max, i, st[i], one[i][:2])


@pytest.mark.parametrize("kind", [F64, RAT])
def test_dev_form_equals_the_host_form_and_counts_the_pivots(ctx, kind):
    R, V = hc.SHAPES["odd"]
    count, cap = (COUNT, 300) if kind == F64 else (RAT_COUNT, 48)
    leq, tg = hc.mixed_batch(kind, True, R, V, count, 0)
    want = hc.oracle_answers("odd", kind, True, leq, tg, cap)
    st, v, sol, _ = _solve(ctx, kind, True, leq, tg, cap)
    m, cols = leq.shape[1], leq.shape[2]
    d_leq, d_tg = ctx.malloc(leq.nbytes), ctx.malloc(tg.nbytes)
    d_st, d_v, d_sol, d_piv = ctx.malloc(count * 4), ctx.malloc(count * 8), ctx.malloc(count * cols * 8), ctx.malloc(count * 4)
    try:
        ctx.upload(d_leq, leq); ctx.upload(d_tg, tg)
        ctx.upload(d_sol, np.zeros(count * cols * 8, dtype=np.uint8))
        ctx.six_batch_hbm_dev(kind, True, count, d_tg, d_leq, m, cols, d_st, d_v, d_sol, d_piv, max_iter=cap)
        ctx.sync()
        st2 = ctx.download(np.zeros(count, dtype=np.int32), d_st)
        v2 = ctx.download(np.zeros_like(v), d_v)
        sol2 = ctx.download(np.zeros_like(sol), d_sol)
        piv = ctx.download(np.zeros(count, dtype=np.uint32), d_piv)
    finally:
        for p in (d_leq, d_tg, d_st, d_v, d_sol, d_piv):
            ctx.free(p)
    assert st2.tobytes() == st.tobytes() and v2.tobytes() == v.tobytes() and sol2.tobytes() == sol.tobytes()
    assert [int(p) for p in piv] == [w[3] for w in want]
    assert len({w[3] for w in want}) >= 2


def test_a_fitting_shape_takes_the_lds_kernel_with_the_same_bits(ctx):
    R, V = hc.FITS
    for kind, cap in ((F64, hc.NO_LIMIT), (RAT, 64)):
        assert bg.lds_fits(kind, R, V)
        for is_max in (True, False):
            leq, tg = hc.mixed_batch(kind, is_max, R, V, 32, 1)
            st, v, sol, route = _solve(ctx, kind, is_max, leq, tg, cap)
            assert route == dict(lds=32, hbm=0, grid=32)
            st0, v0, sol0 = ctx.six_batch(kind, is_max, tg, leq, max_iter=cap)
            assert st.tobytes() == st0.tobytes() and v.tobytes() == v0.tobytes() and sol.tobytes() == sol0.tobytes()
            assert len(set(st.tolist())) >= 2


def test_a_refused_shape_leaves_the_outputs_and_the_handle_alone(ctx):
    from xpoly_amd import XpgError
    from xpoly_amd.six import six_batch_hbm, six_batch_hbm_last_route
    R, V = hc.SHAPES["first"]
    leq, tg = hc.mixed_batch(F64, True, R, V, COUNT, 0)
    want = hc.oracle_answers("first", F64, True, leq, tg, 48)
    big_leq, big_tg = np.ones((2, 600, 601)), np.ones((2, 601))
    out = (np.full(2, 77, dtype=np.int32), np.full(2, 3.5), np.full((2, 601), -2.25))
    with pytest.raises(XpgError, match="XPG_ERR_UNSUPPORTED"):
        six_batch_hbm(ctx, F64, True, big_tg, big_leq, max_iter=8, out=out)
    assert (out[0] == 77).all() and (out[1] == 3.5).all() and (out[2] == -2.25).all()
    assert six_batch_hbm_last_route() == dict(lds=0, hbm=0, grid=0)
    ctx.trim()                                                   # the slots go back; the next call takes new ones
    st, v, sol, route = _solve(ctx, F64, True, leq, tg, 48)
    assert route["hbm"] == COUNT
    _compare((st, v, sol), want, "after a refusal")
    # an empty batch is no error and no launch
    st, v, sol, route = _solve(ctx, F64, True, leq[:0], tg[:0], 48)
    assert st.shape == (0,) and route == dict(lds=0, hbm=0, grid=0)


def test_the_oracle_statuses_cover_every_end():
    """What the cases above compare against, from the restatement alone (answers shared with them)."""
    seen, total, skipped = set(), 0, 0
    for name, is_max in F64_CASES:
        R, V = hc.SHAPES[name]
        leq, tg = hc.mixed_batch(F64, is_max, R, V, COUNT, hc.SEEDS.get(name, 0))
        for cap in (300, 48):
            for w in hc.oracle_answers(name, F64, is_max, leq, tg, cap):
                seen.add(w[0]); total += 1; skipped += w[0] == -7
    for is_max in (True, False):
        leq, tg = hc.succ_batch(is_max, SUCC_COUNT)
        seen |= {w[0] for w in hc.oracle_answers("succ", F64, is_max, leq, tg)}
    name, is_max, idx = UNBOUNDED
    leq, tg = hc.mixed_batch(F64, is_max, *hc.SHAPES[name], COUNT, 0)
    seen |= {w[0] for w in hc.oracle_answers("unbounded", F64, is_max, np.ascontiguousarray(leq[list(idx)]), np.ascontiguousarray(tg[list(idx)]))}
    assert seen >= {0, 1, 2, 3, 4} and skipped == 0, (seen, skipped, total)
