"""Lineq::has_solution for a batch in one launch (xpg_has_solution_batch_*): the feasibility objective, SIX::normalize once, maxm,
then minm where maxm left the question open, by one workgroup per system.

Checker (tests/has_solution_cases.py): the CPU restatement, non-strict wherever a variable is free -- port.has_solution for the
verdicts, port.six_solve on the feasibility objective for the two statuses --, each case's answers computed once. Every
comparison is exact: the verdict and both statuses, XPG_HS_NOT_RUN exactly where maxm decided."""
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
XPG_ERR_UNSUPPORTED, XPG_ERR_REF_UNDEFINED = -4, -7


def _batch(ctx, arrays, unique, max_iter=hs.NO_LIMIT, is_int=False):
    from xpoly_amd.six import has_solution_batch, has_solution_batch_last_route
    vc_arr, eq, leq = arrays
    has, st = has_solution_batch(ctx, leq, eq, vc_arr, is_int, unique, max_iter=max_iter, want_status=True)
    return has, st, has_solution_batch_last_route()


def _compare(got, want, unique, what):
    """got = (has, status); want = oracle_answers' list. Returns the (maxm, minm) status pairs as the call reported them."""
    has, st = got
    want_has, want_st = hs.expected(want, unique)
    for i in range(len(want)):
        assert has[i] == want_has[i] and tuple(st[i]) == tuple(want_st[i]), (what, unique, i, int(has[i]), tuple(st[i]), want[i])
        decided_by_maxm = want[i][2] <= 0 or (want[i][2] == 1 and not unique)
        assert (st[i][1] == hs.NOT_RUN) == decided_by_maxm, (what, unique, i, tuple(st[i]))
    return [(int(a), int(b)) for a, b in st]


_lds_seen = {}


@pytest.mark.parametrize("shape,count", hs.LDS_CASES)
def test_route_0_matches_the_checker(ctx, shape, count):
    arrays = hs.small_arrays(shape, count)
    want = hs.oracle_answers(("small", shape), arrays, count)
    for unique in (False, True):
        has, st, route = _batch(ctx, arrays, unique)
        second = sum(1 for w in want if not (w[2] <= 0 or (w[2] == 1 and not unique)))
        assert route == dict(lds=count, hbm=0, host=0, second=second, grid=count), route
        pairs = _compare((has, st), want, unique, shape)
        print("%s u=%d pairs %s" % (shape, unique, {p: pairs.count(p) for p in sorted(set(pairs))}))
    _lds_seen[shape] = want


def test_route_0_cases_cover_every_way_a_system_ends(ctx):
    """What the generated systems hold, asserted so that a changed seed cannot empty the comparisons above: a system decided
    by each pass, a (1, 2) system whose verdict differs between the two values of is_unique_sol, one that ends 0, one -7."""
    want = []
    for shape, count in hs.LDS_CASES:
        want += _lds_seen.get(shape) or hs.oracle_answers(("small", shape), hs.small_arrays(shape, count), count)
    assert any(w[2] == 0 for w in want)                                              # maxm decides
    assert any(w[2] >= 2 and w[3] == 0 for w in want)                                # minm decides
    assert any((w[2], w[3]) == (1, 2) and w[0] == 1 and w[1] == 0 for w in want)
    assert any(w[0] == 0 and w[1] == 0 for w in want)
    assert any(w[0] == -7 and w[2] == -7 for w in want)


@pytest.mark.parametrize("family,shape,is_max", vc.RAT_CASES)
def test_route_1_matches_the_checker(ctx, family, shape, is_max):
    arrays = hs.hbm_arrays(family, shape, is_max)
    want = hs.oracle_answers((family, shape, is_max), arrays, hs.HBM_COUNT, hs.HBM_CAP)
    assert sum(1 for w in want if w[2] >= 2 and w[3] == 0) >= 1, want               # minm decides
    assert sum(1 for w in want if w[0] == 0) >= 1, want
    for unique in (False, True):
        has, st, route = _batch(ctx, arrays, unique, hs.HBM_CAP)
        assert route["hbm"] == hs.HBM_COUNT and route["lds"] == 0 and route["host"] == 0 and route["grid"] == hs.HBM_COUNT, route
        pairs = _compare((has, st), want, unique, (family, shape, is_max))
        print("%s %s %d u=%d pairs %s" % (family, shape, is_max, unique, {p: pairs.count(p) for p in sorted(set(pairs))}))


@pytest.mark.parametrize("shape", [(5, 2, 5, 1), (12, 3, 12, 2)])
def test_batch_equals_single_calls(ctx, shape):
    from xpoly_amd.six import has_solution
    vc_arr, eq, leq = arrays = hs.small_arrays(shape, 32)
    for unique in (False, True):
        has, _, _ = _batch(ctx, arrays, unique)
        one = [has_solution(ctx, leq[i], eq[i], vc_arr, shape[2], False, unique) for i in range(32)]
        assert [int(h) for h in has] == one, (shape, unique)


def stride_digest(ctx):
    """One line per case: the verdicts and statuses of (5, 2, 5, 1) and of the "fold" case (60, 6, 62, 2), both values of
    is_unique_sol; and the grid of the launch."""
    out = []
    for key, arrays, cap in ((("small", (5, 2, 5, 1)), hs.small_arrays((5, 2, 5, 1), 37), hs.NO_LIMIT),
                             (("fold", vc.FOLD_SHAPES[0]), hs.hbm_arrays("fold", vc.FOLD_SHAPES[0], True), hs.HBM_CAP)):
        for unique in (False, True):
            has, st, route = _batch(ctx, arrays, unique, cap)
            out.append("%s %d %s %s grid=%d" % (key, unique, has.tolist(), st.tolist(), route["grid"]))
    return out


@needs_hooks
def test_a_capped_grid_walks_the_batch_in_strides(ctx):
    """XPG_HS_GRID=2 (hooks build; read once per process, hence the child): two workgroups take 37 and 8 systems in turn, each
    through the slot, LDS block and hdr the one before used -- ragged rows, ends after either pass -- and pass 2 over what
    pass 1 left. The answers are those of the uncapped launch."""
    mine = stride_digest(ctx)
    code = ("import sys; sys.path.insert(0, 'tests')\n"
            "import xpoly_amd, test_gpu_has_solution_batch as t\n"
            "ctx = xpoly_amd.Context(0)\n"
            "for line in t.stride_digest(ctx):\n"
            "    print('D', line)\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=hooks_env(XPG_HS_GRID="2"), cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    theirs = [l[2:] for l in r.stdout.splitlines() if l.startswith("D ")]
    assert len(mine) == 4 and [m.rsplit(" grid=", 1)[0] for m in mine] == [t.rsplit(" grid=", 1)[0] for t in theirs]
    assert [m.rsplit("=", 1)[1] for m in mine] == ["37", "37", "8", "8"] and all(t.endswith("grid=2") for t in theirs)


def _dev_call(ctx, arrays, unique, max_iter=hs.NO_LIMIT):
    from xpoly_amd.six import has_solution_batch_last_route
    vc_arr, eq, leq = arrays
    nb, cols = leq.shape[0], leq.shape[2]
    bufs = [ctx.malloc(a.nbytes) for a in (leq, eq, vc_arr)]
    d_has, d_st = ctx.malloc(nb * 4), ctx.malloc(nb * 8)
    try:
        for p, a in zip(bufs, (leq, eq, vc_arr)):
            ctx.upload(p, a)
        ctx.upload(d_has, np.full(nb, 55, dtype=np.int32))
        ctx.has_solution_batch_dev(nb, bufs[0], leq.shape[1], bufs[1], eq.shape[1], bufs[2], cols, unique, d_has, d_st, max_iter=max_iter)
        route = has_solution_batch_last_route()
        ctx.sync()
        has = ctx.download(np.zeros(nb, dtype=np.int32), d_has)
        st = ctx.download(np.zeros((nb, 2), dtype=np.int32), d_st)
    finally:
        for p in bufs + [d_has, d_st]:
            ctx.free(p)
    return has, st, route


def test_dev_form_equals_the_host_form(ctx):
    from xpoly_amd import XpgError
    shape, count = (4, 1, 4, 0), 64
    arrays = hs.small_arrays(shape, count)
    for unique in (False, True):
        has, st, _ = _batch(ctx, arrays, unique)
        has2, st2, route = _dev_call(ctx, arrays, unique)
        assert route == dict(lds=count, hbm=0, host=0, second=-1, grid=count), route
        assert has2.tobytes() == has.tobytes() and st2.tobytes() == st.tobytes()
    # a general vc is known to the device alone: every system ends XPG_ERR_UNSUPPORTED
    for vc0 in fc.general_vcs(shape[2]):
        has2, st2, _ = _dev_call(ctx, (gen.to_rat(vc0), arrays[1], arrays[2]), True)
        assert (has2 == XPG_ERR_UNSUPPORTED).all() and (st2[:, 1] == hs.NOT_RUN).all()
    with pytest.raises(XpgError, match="XPG_ERR_SHAPE"):                            # is_int_sol is the host-array form's
        ctx.has_solution_batch_dev(1, 1, 4, 1, 1, 1, 5, True, 1, is_int_sol=True)


def test_a_general_vc_goes_per_system(ctx):
    from xpoly_amd.six import has_solution
    shape = (4, 1, 4, 0)
    _, eq, leq = hs.small_arrays(shape, 8)
    for vc0 in (gen.to_rat(v) for v in fc.general_vcs(shape[2])):
        has, st, route = _batch(ctx, (vc0, eq, leq), True)
        assert route == dict(lds=0, hbm=0, host=8, second=0, grid=0), route
        assert [int(h) for h in has] == [has_solution(ctx, leq[i], eq[i], vc0, shape[2], False, True) for i in range(8)]
        assert (st == hs.NOT_RUN).all()


@pytest.mark.parametrize("shape", [(4, 1, 4, 0), (5, 2, 5, 1)])
def test_integer_solutions_are_two_batched_walks(ctx, shape):
    arrays = hs.small_arrays(shape, 64)
    want = hs.int_answers(("small", shape), arrays, 64)
    assert len({w for w in want}) >= 2, want
    for k, unique in enumerate((False, True)):
        has, st, route = _batch(ctx, arrays, unique, is_int=True)
        assert [int(h) for h in has] == [w[k] for w in want], (shape, unique)
        assert route["lds"] == 0 and route["hbm"] == 0 and route["host"] == 0 and route["grid"] == 0, route     # no launch of the new kernels
        assert route["second"] == int((st[:, 1] != hs.NOT_RUN).sum())


def test_shape_rules_and_systems_without_rows(ctx):
    from xpoly_amd._capi import lib, vp
    import ctypes as C
    vc_arr, eq, leq = hs.small_arrays((4, 1, 4, 0), 4)
    has = np.full(4, 55, dtype=np.int32); st = np.full((4, 2), 55, dtype=np.int32)
    call = lambda nb, l, lr, e, er, vc_rows, cols, rhs: lib().xpg_has_solution_batch_rat32(
        ctx._h, C.c_int(nb), vp(l), C.c_int(lr), vp(e), C.c_int(er), vp(vc_arr), C.c_int(vc_rows), C.c_int(cols), C.c_int(rhs), C.c_int(0),
        C.c_int(1), C.c_uint(hs.NO_LIMIT), vp(has), vp(st))
    assert call(4, leq, 4, eq, 1, 4, 5, 3) == -3 and call(4, leq, 4, eq, 1, 3, 5, 4) == -3      # rhs_idx != cols - 1; vc_rows != rhs_idx
    assert (has == 55).all()
    assert call(0, leq, 4, eq, 1, 4, 5, 4) == 0 and (has == 55).all()                           # nb = 0
    assert call(4, None, 0, None, 0, 4, 5, 4) == 0 and (has == 0).all() and (st == hs.NOT_RUN).all()
    assert call(4, None, 0, eq, 1, 4, 5, 4) == 0 and (has == XPG_ERR_REF_UNDEFINED).all()      # the reference sizes tgtf from leq
    ctx.trim()                                                   # the slots go back; the next call takes new ones
    want = hs.oracle_answers(("small", (4, 1, 4, 0)), hs.small_arrays((4, 1, 4, 0), 4), 4)
    _compare(_batch(ctx, (vc_arr, eq, leq), True)[:2], want, True, "after trim")


@pytest.mark.parametrize("eq_rows", [0, 2])
def test_without_inequalities_every_form_ends_as_the_single_call(ctx, eq_rows):
    """leq_rows = 0 never meets a solve: no rows at all is "no solution" with neither solve run, equalities only is
    XPG_ERR_REF_UNDEFINED as verdict and as the first status (the reference sizes tgtf from leq). The host-array form, the _dev
    form and the is_int_sol = 1 form give that for every system, and xpg_has_solution_rat32 the same verdict per system."""
    from xpoly_amd._capi import lib, vp
    from xpoly_amd.six import has_solution
    import ctypes as C
    nb, cols = 3, 4
    vc_arr = gen.to_rat(gen.vc_nonneg(cols - 1, False))
    eq = gen.to_rat(np.random.default_rng(31).integers(-3, 4, size=(nb, eq_rows, cols))) if eq_rows else None
    want_has = 0 if eq_rows == 0 else XPG_ERR_REF_UNDEFINED
    want_st = (hs.NOT_RUN, hs.NOT_RUN) if eq_rows == 0 else (XPG_ERR_REF_UNDEFINED, hs.NOT_RUN)
    for unique in (False, True):
        for is_int in (0, 1):
            has = np.full(nb, 55, dtype=np.int32); st = np.full((nb, 2), 55, dtype=np.int32)
            assert lib().xpg_has_solution_batch_rat32(
                ctx._h, C.c_int(nb), None, C.c_int(0), vp(eq), C.c_int(eq_rows), vp(vc_arr), C.c_int(cols - 1), C.c_int(cols), C.c_int(cols - 1),
                C.c_int(is_int), C.c_int(int(unique)), C.c_uint(hs.NO_LIMIT), vp(has), vp(st)) == 0
            one = [has_solution(ctx, None, None if eq is None else eq[i], vc_arr, cols - 1, bool(is_int), unique) for i in range(nb)]
            print("eq_rows=%d u=%d int=%d has %s status %s single %s" % (eq_rows, unique, is_int, has.tolist(), st.tolist(), one))
            assert has.tolist() == [want_has] * nb and st.tolist() == [list(want_st)] * nb and one == [want_has] * nb
        d_eq = ctx.malloc(eq.nbytes) if eq_rows else 0
        d_vc, d_has, d_st = ctx.malloc(vc_arr.nbytes), ctx.malloc(nb * 4), ctx.malloc(nb * 8)
        try:
            if eq_rows:
                ctx.upload(d_eq, eq)
            ctx.upload(d_vc, vc_arr)
            ctx.upload(d_has, np.full(nb, 55, dtype=np.int32)); ctx.upload(d_st, np.full((nb, 2), 55, dtype=np.int32))
            ctx.has_solution_batch_dev(nb, 0, 0, d_eq, eq_rows, d_vc, cols, unique, d_has, d_st)
            ctx.sync()
            has = ctx.download(np.zeros(nb, dtype=np.int32), d_has)
            st = ctx.download(np.zeros((nb, 2), dtype=np.int32), d_st)
        finally:
            for p in [d_vc, d_has, d_st] + ([d_eq] if eq_rows else []):
                ctx.free(p)
        print("eq_rows=%d u=%d _dev has %s status %s" % (eq_rows, unique, has.tolist(), st.tolist()))
        assert has.tolist() == [want_has] * nb and st.tolist() == [list(want_st)] * nb


def test_the_collector_groups_by_shape_and_scatters_back(ctx, tmp_path):
    """tests/cxx/has_solution_all.cpp in a child process: systems of (4, 1, 4, 0) and (9, 2, 4, 0) interleaved -- one vc, two
    shape groups -- come back in the order given with the checker's verdicts."""
    from test_has_solution_batch_host import build_collector
    exe = build_collector()
    groups = [((4, 1, 4, 0), 12), ((9, 2, 4, 0), 12)]
    data = [hs.small_arrays(s, n) for s, n in groups]
    want = [hs.oracle_answers(("small", s), a, n) for (s, n), a in zip(groups, data)]
    lines, expect = ["4 0 1 24", " ".join(str(int(x)) for x in data[0][0][..., 0].ravel())], []
    for i in range(12):
        for g in range(2):
            _, eq, leq = data[g]
            lines.append("%d %d" % (leq.shape[1], eq.shape[1]))
            lines.append(" ".join(str(int(x)) for x in leq[i][..., 0].ravel()))
            lines.append(" ".join(str(int(x)) for x in eq[i][..., 0].ravel()))
            expect.append(want[g][i][1])
    path = str(tmp_path / "systems.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = r.stdout.split()
    assert got[:2] == ["rc", "0"] and [int(x) for x in got[2:]] == expect
    assert len(set(expect)) >= 2
