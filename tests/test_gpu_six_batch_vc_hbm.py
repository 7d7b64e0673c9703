"""Batches of LPs with equalities and free variables beyond 64 KB of LDS (xpg_six_batch_vc_hbm_*): SIX::normalize, the solve on a
tableau in device memory and calcFinalSolution by one workgroup per LP, in one launch.

Checkers (tests/six_vc_hbm_cases.py): the CPU restatement of the reference, non-strict (the real reference is undefined with a
free variable), each batch's answers computed once; and the unchanged single-problem route SIX.maxm / minm, which reshapes on
the host. Every comparison is exact: status, the optimum's bits, and on status 0 the solution's bits. An LP is skipped only
where the restatement itself returns -7 outside the tall case, at most 4 per 256 (none of the committed inputs does).

Families: "pairs" (twins and kept equality pairs), "fold" (a substitution on device memory in the even LPs, none in the odd
ones: ragged rows in one batch), "tall" (leq_rows > cols: the odd LPs alone end -7). max_iter bounds each solve of an LP on its
own: fp64 runs under 300 and 48, Rational (slow in the restatement) 8 LPs under 48."""
import numpy as np
import pytest

import free_var_cases as fc
import six_vc_hbm_cases as vc
from six_vc_hbm_cases import F64, RAT
from tools import gen

pytestmark = pytest.mark.gpu
NOT_COUNTED = 0xFFFFFFFF


def _solve(ctx, kind, is_max, arrs, max_iter=vc.NO_LIMIT, out=None):
    from xpoly_amd.six import six_batch_vc_hbm, six_batch_vc_hbm_last_route
    tg, vc_arr, eq, leq = arrs
    st, v, sol = six_batch_vc_hbm(ctx, kind, is_max, tg, vc_arr, leq, eq, max_iter=max_iter, out=out)
    return st, v, sol, six_batch_vc_hbm_last_route()


def _singles(ctx, kind, is_max, arrs, idx, max_iter=vc.NO_LIMIT):
    from xpoly_amd.six import SIX
    tg, vc_arr, eq, leq = arrs
    six = SIX(ctx, kind)
    six.set_param(0, max_iter)
    return [(six.maxm if is_max else six.minm)(tg[i], vc_arr, eq[i], leq[i]) for i in idx]


def _compare(got, want, what, minus_7_expected=False):
    """got = (st, v, sol) arrays, want = the restatement's list. Returns the statuses compared."""
    st, v, sol = got
    skipped, seen = 0, []
    for i, w in enumerate(want):
        if w[0] == -7 and not minus_7_expected:
            skipped += 1
            continue
        assert vc.same_answer(st[i], v[i], sol[i], w), (what, i, st[i], v[i], w[:2])
        if st[i] != 0:
            assert not sol[i].any(), (what, i)                   # written on status 0 only
        seen.append(int(w[0]))
    assert skipped <= 4 * ((len(want) + 255) // 256), (what, skipped)
    return seen


def _hbm(nb, nfree, grid=None):
    return dict(lds=0, hbm=nb, fallback=0, free=nfree, grid=nb if grid is None else grid)


@pytest.mark.parametrize("family,shape,is_max", vc.F64_CASES)
def test_fp64_batches_match_the_oracle_and_the_single_calls(ctx, family, shape, is_max):
    """64 LPs per family, shape and direction under two caps; the first 6 also against their single calls; LP 0 again as
    nb = 1. (30, 3, 130, 2) under maxm fits 64 KB: the rule keeps it on the LDS-resident kernel."""
    arrs = vc.arrays(family, shape, F64, is_max, vc.COUNT)
    on_lds = shape == vc.SPLIT and is_max
    for cap in vc.CAPS:
        want = vc.oracle_answers(family, shape, F64, is_max, vc.COUNT, cap)
        st, v, sol, route = _solve(ctx, F64, is_max, arrs, cap)
        assert route == (dict(lds=vc.COUNT, hbm=0, fallback=0, free=shape[3], grid=vc.COUNT) if on_lds else _hbm(vc.COUNT, shape[3])), route
        seen = _compare((st, v, sol), want, (family, shape, is_max, cap))
        print("%s %s is_max=%d cap=%d statuses %s" % (family, shape, is_max, cap, {s: seen.count(s) for s in sorted(set(seen))}))
        one = _singles(ctx, F64, is_max, arrs, range(6), cap)
        for i in range(6):
            assert vc.same_answer(st[i], v[i], sol[i], one[i]), (family, shape, is_max, cap, i, st[i], one[i][:2])
    st1, v1, sol1, route = _solve(ctx, F64, is_max, tuple(a if k == 1 else a[:1] for k, a in enumerate(arrs)), 300)
    assert (route["lds"], route["hbm"], route["grid"]) == ((1, 0, 1) if on_lds else (0, 1, 1)), route
    assert vc.same_answer(st1[0], v1[0], sol1[0], vc.oracle_answers(family, shape, F64, is_max, vc.COUNT, 300)[0])


@pytest.mark.parametrize("family,shape,is_max", vc.RAT_CASES)
def test_rational_batches_match_the_oracle_and_the_single_calls(ctx, family, shape, is_max):
    arrs = vc.arrays(family, shape, RAT, is_max, vc.RAT_COUNT)
    want = vc.oracle_answers(family, shape, RAT, is_max, vc.RAT_COUNT, vc.RAT_CAP)
    st, v, sol, route = _solve(ctx, RAT, is_max, arrs, vc.RAT_CAP)
    assert route == _hbm(vc.RAT_COUNT, shape[3]), route
    seen = _compare((st, v, sol), want, (family, shape, is_max))
    assert len(set(seen)) >= 2, seen
    if family == "fold" and not is_max:
        assert seen.count(0) >= 2, seen                           # the fold's solutions, bit for bit
    one = _singles(ctx, RAT, is_max, arrs, range(2), vc.RAT_CAP)
    for i in range(2):
        assert vc.same_answer(st[i], v[i], sol[i], one[i]), (family, shape, is_max, i, st[i], one[i][:2])
    st1, v1, sol1, route = _solve(ctx, RAT, is_max, tuple(a if k == 1 else a[:1] for k, a in enumerate(arrs)), vc.RAT_CAP)
    assert route == _hbm(1, shape[3]) and vc.same_answer(st1[0], v1[0], sol1[0], want[0])


@pytest.mark.parametrize("is_max", [True, False])
def test_succ_batches_without_a_cap(ctx, is_max):
    """The block LPs that end SIX_SUCC under twins and equality pairs, (96, 4, 103, 2) / (101, 4, 98, 2): no cap; status 0
    comes with a non-zero optimum."""
    shape = vc.SUCC_SHAPES[is_max]
    arrs = vc.arrays("succ", shape, F64, is_max, vc.SUCC_COUNT)
    want = vc.oracle_answers("succ", shape, F64, is_max, vc.SUCC_COUNT)
    st, v, sol, route = _solve(ctx, F64, is_max, arrs)
    assert route == _hbm(vc.SUCC_COUNT, 2), route
    seen = _compare((st, v, sol), want, ("succ", is_max))
    assert 0 in seen and all(float(v[i]) != 0.0 for i in range(vc.SUCC_COUNT) if st[i] == 0)
    one = _singles(ctx, F64, is_max, arrs, range(4))
    for i in range(4):
        assert vc.same_answer(st[i], v[i], sol[i], one[i]), (is_max, i, st[i], one[i][:2])


def _dev_call(ctx, kind, is_max, arrs, cap, like):
    """The _dev form on uploaded copies of the arrays: (status, v, sol, pivots, route); sol starts as zeros."""
    from xpoly_amd.six import six_batch_vc_hbm_last_route
    tg, vc_arr, eq, leq = arrs
    nb, cols = tg.shape[0], tg.shape[1]
    bufs = [ctx.malloc(a.nbytes) for a in (tg, vc_arr, eq, leq)]
    d_st, d_v, d_sol, d_piv = ctx.malloc(nb * 4), ctx.malloc(nb * 8), ctx.malloc(nb * cols * 8), ctx.malloc(nb * 4)
    try:
        for p, a in zip(bufs, (tg, vc_arr, eq, leq)):
            ctx.upload(p, a)
        ctx.upload(d_sol, np.zeros(nb * cols * 8, dtype=np.uint8))
        ctx.upload(d_piv, np.full(nb, 7, dtype=np.uint32))
        ctx.six_batch_vc_hbm_dev(kind, is_max, nb, bufs[0], bufs[1], bufs[2], eq.shape[1], bufs[3], leq.shape[1], cols, d_st, d_v, d_sol, d_piv,
                                 max_iter=cap)
        route = six_batch_vc_hbm_last_route()
        ctx.sync()
        st = ctx.download(np.zeros(nb, dtype=np.int32), d_st)
        v = ctx.download(np.zeros_like(like[1]), d_v)
        sol = ctx.download(np.zeros_like(like[2]), d_sol)
        piv = ctx.download(np.zeros(nb, dtype=np.uint32), d_piv)
    finally:
        for p in bufs + [d_st, d_v, d_sol, d_piv]:
            ctx.free(p)
    return st, v, sol, piv, route


@pytest.mark.parametrize("kind,family", [(F64, "pairs"), (F64, "fold"), (RAT, "fold")])
def test_dev_form_equals_the_host_form_and_counts_the_pivots(ctx, kind, family):
    shape = vc.ODD if family == "pairs" else vc.FOLD_SHAPES[1]
    count, cap = (vc.COUNT, 300) if kind == F64 else (vc.RAT_COUNT, vc.RAT_CAP)
    for is_max in (True, False):
        arrs = vc.arrays(family, shape, kind, is_max, count)
        want = vc.oracle_answers(family, shape, kind, is_max, count, cap)
        st, v, sol, _ = _solve(ctx, kind, is_max, arrs, cap)
        st2, v2, sol2, piv, route = _dev_call(ctx, kind, is_max, arrs, cap, (st, v, sol))
        assert route == _hbm(count, -1), route
        assert st2.tobytes() == st.tobytes() and v2.tobytes() == v.tobytes() and sol2.tobytes() == sol.tobytes()
        assert [int(p) for p in piv] == [w[3] for w in want]
        assert len({w[3] for w in want}) >= 2


def test_one_set_of_arrays_takes_both_kernels(ctx):
    """(30, 3, 130, 2): maximising, the normal form fits 64 KB -- the LDS-resident kernel, the bytes of six_batch_vc, and a _dev
    call's out_pivots all 0xFFFFFFFF (shrunk to one free variable there: the _dev form sizes for every variable free);
    minimising, the same arrays take the device-memory kernel."""
    from xpoly_amd.six import six_batch_vc, six_batch_last_route, six_batch_vc_hbm_plan
    arrs = vc.arrays("pairs", vc.SPLIT, F64, True, vc.COUNT)
    tg, vc_arr, eq, leq = arrs
    st, v, sol, route = _solve(ctx, F64, True, arrs, 300)
    assert route == dict(lds=vc.COUNT, hbm=0, fallback=0, free=2, grid=vc.COUNT)
    st0, v0, sol0 = six_batch_vc(ctx, F64, True, tg, vc_arr, leq, eq, max_iter=300)
    assert six_batch_last_route() == dict(device=vc.COUNT, fallback=0, free=2)
    assert st.tobytes() == st0.tobytes() and v.tobytes() == v0.tobytes() and sol.tobytes() == sol0.tobytes()
    arrs_min = vc.arrays("pairs", vc.SPLIT, F64, False, vc.COUNT)
    st, v, sol, route = _solve(ctx, F64, False, arrs_min, 300)
    assert route == _hbm(vc.COUNT, 2)
    _compare((st, v, sol), vc.oracle_answers("pairs", vc.SPLIT, F64, False, vc.COUNT, 300), "split minm")
    # a _dev call that stays LDS-resident with every variable free: the first 16 inequalities and variables of the shape
    small = (np.ascontiguousarray(np.concatenate([tg[:, :16], tg[:, -1:]], axis=1)), gen.vc_nonneg(16, True, range(2)),
             np.ascontiguousarray(np.concatenate([eq[:, :, :16], eq[:, :, -1:]], axis=2)),
             np.ascontiguousarray(np.concatenate([leq[:, :16, :16], leq[:, :16, -1:]], axis=2)))
    assert six_batch_vc_hbm_plan(F64, None, 16, 3, 17, True, vc.COUNT)["route"] == vc.ROUTE_LDS
    hs, hv, hsol, route = _solve(ctx, F64, True, small, 300)
    assert route["lds"] == vc.COUNT
    st2, v2, sol2, piv, route = _dev_call(ctx, F64, True, small, 300, (hs, hv, hsol))
    assert route == dict(lds=vc.COUNT, hbm=0, fallback=0, free=-1, grid=vc.COUNT)
    assert st2.tobytes() == hs.tobytes() and v2.tobytes() == hv.tobytes() and sol2.tobytes() == hsol.tobytes()
    assert (piv == NOT_COUNTED).all()
    # the _dev form of the whole shape is past 64 KB with every variable free: the device-memory kernel, the same bytes
    hs, hv, hsol, _ = _solve(ctx, F64, True, arrs, 300)
    st2, v2, sol2, piv, route = _dev_call(ctx, F64, True, arrs, 300, (hs, hv, hsol))
    assert route == _hbm(vc.COUNT, -1)
    assert st2.tobytes() == hs.tobytes() and v2.tobytes() == hv.tobytes() and sol2.tobytes() == hsol.tobytes()
    assert [int(p) for p in piv] == [w[3] for w in vc.oracle_answers("pairs", vc.SPLIT, F64, True, vc.COUNT, 300)]


@pytest.mark.parametrize("kind", [F64, RAT])
def test_the_tall_case_ends_minus_7_for_the_odd_lps_alone(ctx, kind):
    from xpoly_amd.six import six_batch_vc_hbm_plan
    count, cap = (vc.COUNT, 300) if kind == F64 else (vc.RAT_COUNT, vc.RAT_CAP)
    arrs = vc.arrays("tall", vc.TALL, kind, True, count)
    m, me, nv, _ = vc.TALL
    assert six_batch_vc_hbm_plan(kind, arrs[1], m, me, nv + 1, True, count)["route"] == vc.ROUTE_HBM and m > nv + 1
    want = vc.oracle_answers("tall", vc.TALL, kind, True, count, cap)
    st, v, sol, route = _solve(ctx, kind, True, arrs, cap)
    assert route == _hbm(count, 1), route
    assert [int(s) == -7 for s in st] == [i % 2 == 1 for i in range(count)]
    seen = _compare((st, v, sol), want, ("tall", kind), minus_7_expected=True)
    assert len(set(seen) - {-7}) >= 2, seen
    one = _singles(ctx, kind, True, arrs, range(4), cap)
    for i in range(4):
        assert vc.same_answer(st[i], v[i], sol[i], one[i]), (kind, i, st[i], one[i][:2])


def test_a_workgroup_reuses_its_slot_for_lps_of_different_rows_and_endings(ctx):
    """nb = 2 x grid + 3 by cycling the 64 "fold" LPs under cap 48: every workgroup takes two or three LPs, with and without a
    substitution (different row counts in the same slot), ending after anything from one pivot to the cap."""
    from xpoly_amd.six import six_batch_vc_hbm_plan
    shape = vc.FOLD_SHAPES[0]
    tg, vc_arr, eq, leq = vc.arrays("fold", shape, F64, False, vc.COUNT)
    want = vc.oracle_answers("fold", shape, F64, False, vc.COUNT, 48)
    assert len({w[0] for w in want}) >= 3 and min(w[3] for w in want) <= 2 and max(w[3] for w in want) >= 48
    grid = six_batch_vc_hbm_plan(F64, vc_arr, shape[0], shape[1], shape[2] + 1, False, 1 << 20)["grid"]
    nb = 2 * grid + 3
    pick = np.arange(nb) % vc.COUNT
    arrs = (np.ascontiguousarray(tg[pick]), vc_arr, np.ascontiguousarray(eq[pick]), np.ascontiguousarray(leq[pick]))
    st, v, sol, route = _solve(ctx, F64, False, arrs, 48)
    assert route["hbm"] == nb and nb >= 2 * route["grid"] + 3, route
    _compare((st, v, sol), [want[i] for i in pick], "reuse")


def test_a_general_vc_falls_back_per_problem(ctx):
    count = 4
    for kind in (F64, RAT):
        tg, _, eq, leq = vc.arrays("pairs", vc.FIRST, kind, True, count)
        for vc0 in fc.general_vcs(vc.FIRST[2]):
            vc_arr = gen.to_rat(vc0) if kind == RAT else np.ascontiguousarray(vc0, dtype=np.float64)
            arrs = (tg, vc_arr, eq, leq)
            st, v, sol, route = _solve(ctx, kind, True, arrs, 48)
            assert route == dict(lds=0, hbm=0, fallback=count, free=0, grid=0), route
            one = _singles(ctx, kind, True, arrs, range(count), 48)
            for i in range(count):
                assert vc.same_answer(st[i], v[i], sol[i], one[i]), (kind, i, st[i], one[i][:2])


def test_a_refused_shape_leaves_the_outputs_and_the_handle_alone(ctx):
    from xpoly_amd import XpgError
    from xpoly_amd.six import six_batch_vc_hbm_last_route, six_batch_vc_hbm_plan
    m, me, nv = 600, 2, 500
    assert six_batch_vc_hbm_plan(F64, None, m, me, nv + 1, True, 2)["route"] == vc.ROUTE_OTHER
    cols = nv + 1
    ptrs = [ctx.malloc(n) for n in (2 * cols * 8, nv * cols * 8, 2 * me * cols * 8, 2 * m * cols * 8)]
    d_st, d_v, d_sol, d_piv = ctx.malloc(2 * 4), ctx.malloc(2 * 8), ctx.malloc(2 * cols * 8), ctx.malloc(2 * 4)
    marks = (np.full(2, 77, dtype=np.int32), np.full(2, 3.5), np.full((2, cols), -2.25), np.full(2, 9, dtype=np.uint32))
    try:
        for p, a in zip((d_st, d_v, d_sol, d_piv), marks):
            ctx.upload(p, a)
        with pytest.raises(XpgError, match="XPG_ERR_UNSUPPORTED"):
            ctx.six_batch_vc_hbm_dev(F64, True, 2, ptrs[0], ptrs[1], ptrs[2], me, ptrs[3], m, cols, d_st, d_v, d_sol, d_piv, max_iter=8)
        assert six_batch_vc_hbm_last_route() == dict(lds=0, hbm=0, fallback=0, free=-1, grid=0)
        ctx.sync()
        for p, a in zip((d_st, d_v, d_sol, d_piv), marks):
            assert ctx.download(np.zeros_like(a), p).tobytes() == a.tobytes()
    finally:
        for p in ptrs + [d_st, d_v, d_sol, d_piv]:
            ctx.free(p)
    ctx.trim()                                                   # the slots go back; the next call takes new ones
    arrs = vc.arrays("pairs", vc.FIRST, F64, True, vc.COUNT)
    st, v, sol, route = _solve(ctx, F64, True, arrs, 48)
    assert route == _hbm(vc.COUNT, 2)
    _compare((st, v, sol), vc.oracle_answers("pairs", vc.FIRST, F64, True, vc.COUNT, 48), "after a refusal")


def test_an_empty_batch_is_no_launch_and_no_error(ctx):
    arrs = vc.arrays("pairs", vc.FIRST, F64, True, vc.COUNT)
    st, v, sol, route = _solve(ctx, F64, True, tuple(a if k == 1 else a[:0] for k, a in enumerate(arrs)), 48)
    assert st.shape == (0,) and route == dict(lds=0, hbm=0, fallback=0, free=0, grid=0)
    ctx.six_batch_vc_hbm_dev(F64, True, 0, 1, 1, 1, 4, 1, 60, 63, 1, 1, 1, None)          # nb = 0 returns before any pointer is used
    from xpoly_amd.six import six_batch_vc_hbm_last_route
    assert six_batch_vc_hbm_last_route() == dict(lds=0, hbm=0, fallback=0, free=-1, grid=0)
