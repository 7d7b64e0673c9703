"""The batched LP kernel (csrc/batch_kernels.hip.h: k_batch, k_batch_ragged, sm_solve, sm_solve_lp) at every launch geometry
and loop form the host code can choose. Every case is compared bit for bit (status, value, the solution where the status is 0)
with Port (our C++ restatement), with the real reference when oracle/_ref/ is built, and -- wherever Port ends with status 0
without the float rescue, for fp64 only where the arithmetic is provably exact (the consecutive-ones family without stage 1,
tests/batch_geometry.py EXACT_FAMILIES) -- with plain exact arithmetic: the solution
is feasible in the caller's own problem, the value is c.x + c0, and it is the optimum an independent simplex on
fractions.Fraction (Bland's rule, tests/batch_geometry.py exact_max) finds. (Under minm the caller's problem is the covering
dual of the slack form that is solved; its optimum is that of the solved form by strong duality.)

The case table (tests/batch_geometry.py) is derived from a Python mirror of the launch rules; the CPU tests here check the
mirror against the library's host-only view (xpg_test_batch_geometry), that the table reaches every branch, and -- with Port
alone -- that the cases are not vacuous.

out_pivots of the _dev form: the kernel counts every SIX::pivot it performs for an LP -- stage 1's pivot of the auxiliary
variable into the basis, the pivots of stage 1's solve, the pivot that takes the auxiliary variable out again when it ended
basic, and the pivots of the LP's own solve -- and Port.pivot_count() counts the calls of its pivot(): the same events. The
test compares the two numbers LP by LP at every shape of the "dev pivots" cases, the tiny ones included."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tools import gen

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import batch_geometry as bg                             # noqa: E402
from batch_geometry import F64, RAT, CASES, Case, case_id, case_facts      # noqa: E402

XPG_ERR_UNSUPPORTED = -4
DISTINCT = 64                                            # make_lps: a batch above 64 LPs repeats its first 64


# ---- the oracles: every distinct LP is solved once per checker and session ---------------------------------------------------
_solved = {}


def oracle_results(checker, name, cs):
    """[(status, value, solution, pivots, rescues)] of the distinct LPs of a case by Port or Ref (pivots: Port only)."""
    key = (name, cs.kind, cs.is_max, cs.R, cs.V, min(cs.nb, DISTINCT), cs.stage1, cs.recipe, cs.limit, cs.label)
    if key not in _solved:
        lps = bg.make_lps(cs._replace(nb=min(cs.nb, DISTINCT)))
        tg, lq = bg.caller_arrays(cs.kind, cs.is_max, lps)
        vc = gen.vc_nonneg(tg.shape[1] - 1, kind_float=(cs.kind == F64))
        if cs.kind == RAT:
            vc = gen.to_rat(vc)
        out = []
        for i in range(len(lps)):
            a0 = checker.appro_count()
            p0 = checker.pivot_count() if name == "port" else 0
            st, v, sol = checker.six_solve(cs.kind, cs.is_max, tg[i], vc, None, lq[i], max_iter=cs.limit)
            out.append((st, np.array(v), sol, (checker.pivot_count() - p0) if name == "port" else None, checker.appro_count() - a0))
        _solved[key] = out
    return _solved[key]


def case_arrays(cs):
    lps = bg.make_lps(cs._replace(nb=min(cs.nb, DISTINCT)))
    tg, lq = bg.caller_arrays(cs.kind, cs.is_max, lps)
    if cs.nb > DISTINCT:
        reps = (cs.nb + DISTINCT - 1) // DISTINCT
        tg = np.ascontiguousarray(np.concatenate([tg] * reps)[:cs.nb]); lq = np.ascontiguousarray(np.concatenate([lq] * reps)[:cs.nb])
    return lps, tg, lq


# ---- CPU tests ------------------------------------------------------------------------------------------------------------------
def _lib():
    from xpoly_amd import build, _capi
    build.build()
    return _capi.lib()


def test_mirror_matches_the_library():
    """small_lds_bytes, the thread rule, the 5 / 4 instance rule, the grid, the refusal and the slice-eligibility terms of the
    mirror against xpg_test_batch_geometry, which returns what batch_dev itself launches with (batch_geometry)."""
    lib = _lib()
    out = (C.c_longlong * 10)()
    shapes = list(bg._shape_scan()) + [f(k) for f in bg.LIMIT_FAMILIES.values() for k in range(90, 140)] + [(24, k) for k in range(380, 400)]
    shapes += [(cs.R, cs.V) for cs in CASES]
    for kind in (F64, RAT):
        for R, V in shapes:
            for nb, cus in ((1, 256), (1281, 256), (300000, 256), (1601, 304), (700, 120)):
                assert lib.xpg_test_batch_geometry(kind, R, V, nb, cus, out, 10) == 0
                assert tuple(out) == tuple(bg.geometry(kind, R, V, nb, cus)), (kind, R, V, nb, cus)
    assert lib.xpg_test_batch_geometry(2, 4, 4, 1, 256, out, 10) == -3 and lib.xpg_test_batch_geometry(0, 0, 4, 1, 256, out, 10) == -3


def test_case_table_covers_every_branch():
    """CPU only: the mirror applied to the table."""
    facts = [(cs, case_facts(cs)) for cs in CASES]
    live = [(cs, f) for cs, f in facts if not f["geom"].refused]
    # every thread count, both instances, per kind and mode
    for kind in (F64, RAT):
        for is_max in (1, 0):
            mine = [(cs, f) for cs, f in live if cs.kind == kind and cs.is_max == is_max]
            assert {f["geom"].threads for _, f in mine} == {64, 128, 256}, (kind, is_max)
            assert {f["geom"].five for _, f in mine} == {0, 1}, (kind, is_max)
            # every ordered pair of loop forms the rules allow for this kind
            need = {p for p in bg.reachable_form_pairs() if kind == F64 or bg.SPECIALISED not in p}
            assert need <= {f["forms"] for _, f in mine}, (kind, is_max, need - {f["forms"] for _, f in mine})
    assert {p for p in bg.reachable_form_pairs() if bg.SPECIALISED in p} == {(None, bg.SPECIALISED), (bg.SPECIALISED, bg.SPECIALISED)}
    # both sides of every threshold, found from the rule and not typed in
    cells = {f["geom"].cells for _, f in live}
    assert 1024 in cells and 2048 in cells
    for lo in (1024, 2048):
        below = [f["geom"].cells for cs, f in live if cs.label == "cells below %d" % lo]
        at = [f["geom"].cells for cs, f in live if cs.label == "cells at %d" % lo]
        assert below and at and max(below) < lo <= min(at) and min(at) - max(below) <= 32, (lo, below, at)    # adjacent V at that R
        for cs, f in live:
            if cs.label == "cells below %d" % lo:
                assert f["geom"].threads == lo // 16 and bg.thread_rule(cs.R, cs.V + 1) == lo // 8, cs
    assert {cs.R for cs, _ in live if cs.label.startswith("rows ")} == {64, 65}
    for tot in (126, 127, 128, 129):
        for s1 in (0, 1):
            assert any(cs.R + cs.V == tot and cs.stage1 == s1 and f["geom"].threads >= 128 for cs, f in live), (tot, s1)
    # rhs 127 / 128 / 129 in the auxiliary solve and in the own solve, each on the form the rule gives it
    for cs, f in live:
        if cs.label.startswith("R+V ") and "64 threads" not in cs.label:
            tot = cs.R + cs.V
            own = bg.OVERLAPPED if tot <= 127 else (bg.WAVE0 if tot == 128 else bg.GENERIC)
            aux = bg.OVERLAPPED if tot + 1 <= 127 else (bg.WAVE0 if tot + 1 == 128 else bg.GENERIC)
            assert f["forms"] == ((aux if cs.stage1 else None), own), cs
    # the specialised loop and its near misses
    spec = [(cs, f) for cs, f in live if cs.label.startswith("specialised")]
    for cs, f in spec:
        is_spec = f["forms"][1] == bg.SPECIALISED
        assert is_spec == ("near miss" not in cs.label), cs
        if is_spec:
            assert (cs.kind, cs.R, cs.V, f["geom"].threads) == (F64, 32, 63, 256) and f["forms"][0] in (None, bg.SPECIALISED)
    assert {(cs.kind, cs.R, cs.V) for cs, _ in spec if "near miss" in cs.label} >= {(F64, 32, 62), (F64, 32, 64), (F64, 31, 63), (F64, 33, 63),
                                                                                     (RAT, 32, 63), (F64, 63, 32)}
    assert any(cs.label == "specialised dual" and not cs.is_max and bg.caller_shape(0, cs.R, cs.V) == (63, 33) for cs, _ in spec)
    for s1 in (0, 1):
        assert any(cs.label == "specialised" and cs.stage1 == s1 for cs, _ in spec)
    # per_cu == 5 on one side, 4 on the other, one variable apart
    for kind in (F64, RAT):
        five = [cs for cs, f in live if cs.kind == kind and cs.label == "five per CU"]
        four = [cs for cs, f in live if cs.kind == kind and cs.label == "four per CU"]
        assert five and four and five[0].V + 1 == four[0].V and five[0].R == four[0].R
        assert bg.geometry(kind, five[0].R, five[0].V, 1).per_cu == 5 and bg.geometry(kind, four[0].R, four[0].V, 1).per_cu == 4
    # fully generic, tall and wide; R > 64 and rhs > 128 separately
    assert any(cs.R > 64 and cs.R + cs.V <= 127 for cs, _ in live) and any(cs.R <= 64 and cs.R + cs.V > 128 for cs, _ in live)
    assert any(cs.R == 1 and cs.V == 1 for cs, _ in live) and any(cs.R == 1 and cs.V > 64 for cs, _ in live)
    # the accepted / refused pair of each family
    for kind in (F64, RAT):
        for fam, fn in bg.LIMIT_FAMILIES.items():
            k = bg.largest_accepted(kind, fn)
            for is_max in (1, 0):
                assert any(c.kind == kind and c.is_max == is_max and (c.R, c.V) == fn(k) and not f["geom"].refused for c, f in facts), (kind, fam)
                assert any(c.kind == kind and c.is_max == is_max and (c.R, c.V) == fn(k + 1) and f["geom"].refused for c, f in facts), (kind, fam)
    assert (bg.largest_accepted(F64, bg.LIMIT_FAMILIES["square"]), bg.largest_accepted(RAT, bg.LIMIT_FAMILIES["square"])) == (96, 96)
    for cs, f in facts:
        assert ("refused" in cs.label) == bool(f["geom"].refused), cs
    # the named finding: arrays that fit 160 KB alone but not beside the kernel's own LDS are refused, not launched
    assert any("static LDS" in cs.label and f["geom"].lds <= bg.LDS_MAX and f["geom"].refused for cs, f in facts)
    # the grid cap, one LP, the _dev form, limits
    assert any(f["stride"] for _, f in live) and any(cs.nb == 1 for cs, _ in live)
    for form in bg.FORMS:
        for s1 in (0, 1):
            assert any(cs.limit != bg.NO_LIMIT and f["forms"][1] == form and cs.stage1 == s1 for cs, f in live), (form, s1)
        assert any(cs.entry == "dev" and f["forms"][1] == form for cs, f in live), form
    # both host routes with the same LPs
    a, b = bg.route_cases()
    ma, ca = bg.caller_shape(a.is_max, a.R, a.V)
    assert bg.pinned_route(ma, ca, a.nb) and not bg.pinned_route(ma, ca, b.nb) and b.nb == a.nb + 1
    assert bg.make_lps(a)[0][1].tobytes() == bg.make_lps(b)[0][1].tobytes()
    assert all(case_facts(cs)["pinned"] for cs in CASES if cs.nb < 100)
    # slices: the sliced and the unsliced side of each eligibility term (forced: the crowding term is replaced by the hook)
    sl = {cs.label: (cs, bg.sliced(cs.kind, cs.R, cs.V, cs.nb, force=True)) for cs in bg.SLICE_CASES if cs.stage1}
    assert sl["slices R+V 127"][1] and not sl["slices R+V 128"][1] and sl["slices rows 64"][1] and not sl["slices rows 65"][1]
    assert sl["slices 128 threads"][1] and case_facts(sl["slices 128 threads"][0])["geom"].threads == 128
    assert not sl["slices 64 threads"][1] and case_facts(sl["slices 64 threads"][0])["geom"].threads == 64
    assert case_facts(sl["slices R+V 127"][0])["forms"] == (bg.WAVE0, bg.OVERLAPPED)
    assert not bg.sliced(F64, 40, 87, 24) and bg.sliced(F64, 40, 87, 5000)        # the crowding term without the hook
    # the crowding term without the hook, on the device: cases with more LPs than seats at slice-eligible shapes
    crowded = [cs for cs in CASES if cs.label == "crowded"]
    assert len(crowded) >= 2 and all(bg.sliced(cs.kind, cs.R, cs.V, cs.nb, cus=c) for cs in crowded for c in (256, 304))
    # the byte edge of the refusal rule
    e = {cs.label: case_facts(cs)["geom"] for cs in CASES if "static edge" in cs.label}
    assert e["largest static edge"].lds + bg.SMALL_LDS_STATIC == bg.LDS_MAX and not e["largest static edge"].refused
    assert e["refused static edge"].lds + bg.SMALL_LDS_STATIC == bg.LDS_MAX + 16 and e["refused static edge"].refused
    # ragged: LPs whose uniform form differs from their form beside a larger LP
    diff = 0
    for kind, is_max, R, V, s1 in bg.RAGGED_LPS:
        uni = bg.loop_forms(kind, R, V, bg.thread_rule(R, V), s1)
        for t, comp in bg.RAGGED_COMPANIONS.items():
            assert bg.ragged_threads(kind, [(R, V), comp]) == max(t, bg.thread_rule(R, V)) and bg.thread_rule(*comp) == t
            diff += uni != bg.loop_forms(kind, R, V, bg.ragged_threads(kind, [(R, V), comp]), s1)
    assert diff >= 8
    assert any((k, R, V) == (F64, 32, 63) for k, _, R, V, _ in bg.RAGGED_LPS)       # the specialised shape beside a larger LP
    assert any(bg.loop_forms(k, R, V, bg.thread_rule(R, V), s1)[1] == bg.WAVE0 and bg.loop_forms(k, R, V, 256, s1)[1] == bg.OVERLAPPED
               for k, _, R, V, s1 in bg.RAGGED_LPS)


def _claims_exact(cs):
    return set(cs.recipe) <= {"ones", "chain"} and cs.nb > 1 and (cs.kind == RAT or not cs.stage1)


def test_cases_are_not_vacuous(port):
    """CPU only, Port alone: conditions on the table, not measurements. Statuses 0, 1, 2 and 3 occur in every loop form (taken
    over the cases whose own solve uses it; 2 ends inside stage 1, so it comes from the cases with stage 1), status 4 in the
    limited cases of every form; a case made of the exact families alone has at least half of its LPs end with status 0
    without the float rescue; every accepted case has an LP with at least 10 pivots in the solve its label names: the own
    solve in a case without stage 1 (all pivots are its), stage 1's solve in a case with it. Port counts pivots per LP, not per
    solve, so stage 1's share is taken where it is certain: all pivots but the first (the auxiliary variable entering) of an
    LP that ends NO_PRI_FEASIBLE_SOL, and for any other LP the pivots but the first of the same LP under a limit of 10
    iterations per solve when that run ends NO_PRI_FEASIBLE_SOL -- the limit then struck inside stage 1's solve. Shapes with
    a single row or a single variable cannot pivot ten times and are exempt; a limited case needs an LP that reaches its
    limit instead (every limit in the table is at least 10)."""
    t0 = time.time()
    seen = {f: set() for f in bg.FORMS}
    limited = {f: set() for f in bg.FORMS}
    for cs in list(CASES) + list(bg.route_cases()) + list(bg.SLICE_CASES):
        f = case_facts(cs)
        if f["geom"].refused:
            continue
        res = oracle_results(port, "port", cs)
        own = f["forms"][1]
        (seen if cs.limit == bg.NO_LIMIT else limited)[own] |= {r[0] for r in res}
        if _claims_exact(cs):
            good = sum(1 for r in res if r[0] == 0 and r[4] == 0)
            assert 2 * good >= len(res), (case_id(cs), [r[0] for r in res])
        if min(cs.R, cs.V) == 1:
            continue
        if cs.limit != bg.NO_LIMIT:
            assert any(r[0] in (2, 4) and r[3] >= cs.limit for r in res), (case_id(cs), [(r[0], r[3]) for r in res])
            continue
        if cs.stage1:
            probe = oracle_results(port, "port", cs._replace(limit=10))       # the same LPs, 10 iterations per solve
            named = [r[3] - 1 if r[0] == 2 else (q[3] - 1 if q[0] == 2 else 0) for r, q in zip(res, probe)]
            assert max(named) >= 10, (case_id(cs), [(r[0], r[3]) for r in res], named)
        else:
            assert max(r[3] for r in res) >= 10, (case_id(cs), [(r[0], r[3]) for r in res])
    for form in bg.FORMS:
        assert {0, 1, 2, 3} <= seen[form], (form, seen[form])
        assert 4 in limited[form] and 2 in limited[form], (form, limited[form])
    print("Port over the whole table: %.1f s" % (time.time() - t0))


def test_exact_simplex_on_known_problems():
    F = bg.Fraction
    assert bg.exact_max([[1, 1], [1, 3]], [4, 6], [3, 2]) == ("optimal", F(12))
    assert bg.exact_max([[1, 2], [-1, 0]], [4, -1], [1, 1]) == ("optimal", F(4))          # x0 >= 1: through the auxiliary variable
    assert bg.exact_max([[1, 0], [-1, 0]], [1, -2], [1, 1])[0] == "infeasible"
    assert bg.exact_max([[-1, 1]], [1], [1, 0])[0] == "unbounded"
    assert bg.exact_max([[2, 1, 1], [4, 2, 3], [2, 5, 5]], [14, 28, 30], [1, 2, -1]) == ("optimal", F(13))


# ---- GPU: one case, three comparisons ---------------------------------------------------------------------------------------------
def _pattern(shape, kind):
    n = int(np.prod(shape))
    if kind == F64:
        return (-(1000.0 + np.arange(n) % 977)).reshape(shape)
    out = np.empty(tuple(shape) + (2,), dtype=np.int32)
    out[..., 0] = (-(1 + np.arange(n) % 977)).reshape(shape)
    out[..., 1] = 7
    return out


def call_host(ctx, cs, tg, lq, status, v, sol):
    """xpg_six_batch_* on caller-owned output arrays; the return code as it comes."""
    from xpoly_amd._capi import lib, vp
    nb, m, cols = lq.shape[0], lq.shape[1], lq.shape[2]
    fn = lib().xpg_six_batch_f64 if cs.kind == F64 else lib().xpg_six_batch_rat32
    return fn(ctx._h, C.c_int(int(cs.is_max)), C.c_int(nb), vp(tg), vp(lq), C.c_int(m), C.c_int(cols), C.c_uint(cs.limit),
              vp(status), vp(v), vp(sol))


def call_dev(ctx, cs, tg, lq, status, v, sol, pivots):
    """xpg_six_batch_*_dev: device arrays in and out, out_pivots included."""
    from xpoly_amd._capi import lib
    nb, m, cols = lq.shape[0], lq.shape[1], lq.shape[2]
    bufs = [ctx.malloc(a.nbytes) for a in (tg, lq, status, v, sol, pivots)]
    try:
        for p, a in zip(bufs, (tg, lq, status, v, sol, pivots)):
            ctx.upload(p, a)
        fn = lib().xpg_six_batch_f64_dev if cs.kind == F64 else lib().xpg_six_batch_rat32_dev
        rc = fn(ctx._h, C.c_int(int(cs.is_max)), C.c_int(nb), C.c_void_p(bufs[0]), C.c_void_p(bufs[1]), C.c_int(m), C.c_int(cols),
                C.c_uint(cs.limit), C.c_void_p(bufs[2]), C.c_void_p(bufs[3]), C.c_void_p(bufs[4]), C.c_void_p(bufs[5]))
        ctx.sync()
        for p, a in zip(bufs[2:], (status, v, sol, pivots)):
            ctx.download(a, p)
    finally:
        for p in bufs:
            ctx.free(p)
    return rc


def expected_arrays(cs, res, pattern_sol, v_like):
    """The arrays the call must leave: status and value of every LP, the solution where the status is 0, the caller's own
    cells everywhere else (include/xpoly_amd.h: out_sol is written on success only)."""
    idx = np.arange(cs.nb) % len(res)
    st = np.array([r[0] for r in res], dtype=np.int32)[idx]
    zero = np.zeros(v_like.shape[1:], dtype=v_like.dtype)          # (*v_out = 0 where the status is not 0; Rational: 0 / 1)
    if zero.ndim:
        zero[1] = 1
    v = np.stack([np.asarray(r[1], dtype=v_like.dtype).reshape(v_like.shape[1:]) if r[0] == 0 else zero for r in res])[idx]
    sols = np.stack([np.asarray(r[2], dtype=pattern_sol.dtype) for r in res])[idx]
    ok = (st == 0).reshape((-1,) + (1,) * (pattern_sol.ndim - 1))
    return st, v, np.where(ok, sols, pattern_sol)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def first_difference(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    rows = a.reshape(a.shape[0], -1).view(np.uint8) != b.reshape(b.shape[0], -1).view(np.uint8)
    bad = np.flatnonzero(rows.reshape(a.shape[0], -1).any(axis=1))
    return int(bad[0]) if len(bad) else -1, len(bad)


def check_exact(cs, lp, st, v, sol, c0=0):
    """Plain fractions: feasible in the caller's own problem, value = c.x + c0, value = the optimum of exact_max."""
    _, A, b, c = lp
    Fr = bg.Fraction
    x = [bg.frac(t) for t in sol[:-1]]
    val = bg.frac(v)
    assert all(t >= 0 for t in x), case_id(cs)
    Af = [[Fr(float(t)) for t in row] for row in A]
    bf, cf = [Fr(float(t)) for t in b], [Fr(float(t)) for t in c]
    if cs.is_max:                                             # maximise c.x, A x <= b
        for i in range(cs.R):
            assert sum(Af[i][j] * x[j] for j in range(cs.V) if x[j]) <= bf[i], (case_id(cs), i)
        assert val == sum(cf[j] * x[j] for j in range(cs.V)) + Fr(c0), case_id(cs)
    else:                                                     # minimise b.y, A^T y >= c
        for j in range(cs.V):
            assert sum(Af[i][j] * x[i] for i in range(cs.R) if x[i]) >= cf[j], (case_id(cs), j)
        assert val == sum(bf[i] * x[i] for i in range(cs.R)) + Fr(c0), case_id(cs)
    assert bg.exact_max(Af, bf, cf) == ("optimal", val - Fr(c0)), case_id(cs)


@pytest.fixture(scope="module")
def ref_or_none():
    from oracle.checker import Ref
    return Ref() if Ref.available() else None


def run_case(cs, ctx, port, ref, entry=None):
    """One case through the device and the three checkers; returns the device arrays."""
    from xpoly_amd import _capi
    entry = entry or cs.entry
    f = case_facts(cs)
    lps, tg, lq = case_arrays(cs)
    kind = cs.kind
    status = np.full(cs.nb, 77, dtype=np.int32)
    v = _pattern((cs.nb,), kind)
    sol0 = _pattern((cs.nb, tg.shape[1]), kind)
    sol = sol0.copy()
    pivots = np.full(cs.nb, 0xDEAD, dtype=np.uint32)
    if f["geom"].refused:                                 # refused before any launch: outputs untouched, and the handle works on
        keep = (status.copy(), v.copy())
        rc = call_host(ctx, cs, tg, lq, status, v, sol)
        assert rc == XPG_ERR_UNSUPPORTED, (case_id(cs), rc)
        assert same_bits(status, keep[0]) and same_bits(v, keep[1]) and same_bits(sol, sol0), case_id(cs)
        rc = call_dev(ctx, cs, tg, lq, status, v, sol, pivots)
        assert rc == XPG_ERR_UNSUPPORTED and same_bits(status, keep[0]) and same_bits(sol, sol0) and (pivots == 0xDEAD).all(), case_id(cs)
        small = Case(kind, cs.is_max, 12, 12, 4, 1, ("dep", "chain"), bg.NO_LIMIT, "after refusal", "host")
        run_case(small, ctx, port, None)
        print("%s: refused as XPG_ERR_UNSUPPORTED (lds %d), outputs untouched, next call matches" % (case_id(cs), f["geom"].lds))
        return None
    if entry == "host":
        rc = call_host(ctx, cs, tg, lq, status, v, sol)
    else:
        rc = call_dev(ctx, cs, tg, lq, status, v, sol, pivots)
    assert rc == 0, (case_id(cs), _capi.ERRORS.get(rc, rc))
    n = {"port": 0, "ref": 0, "exact": 0, "appro": 0}
    res = oracle_results(port, "port", cs)
    want = expected_arrays(cs, res, sol0, v)
    for name, got, exp in (("status", status, want[0]), ("value", v, want[1]), ("solution", sol, want[2])):
        if not same_bits(got, exp):
            b, cnt = first_difference(got, exp)
            pytest.fail("%s: %s differs from Port in %d of %d LPs, first LP %d (%s): device %s / %s, Port %s / %s" % (
                case_id(cs), name, cnt, cs.nb, b, lps[b % len(lps)][0], status[b], np.asarray(v[b]).tolist(), want[0][b],
                np.asarray(want[1][b]).tolist()))
    n["port"] = cs.nb
    if entry == "dev":
        wantp = np.array([r[3] for r in res], dtype=np.uint32)[np.arange(cs.nb) % len(res)]
        assert np.array_equal(pivots, wantp), (case_id(cs), pivots.tolist(), wantp.tolist())
    if ref is not None:
        rres = oracle_results(ref, "ref", cs)
        for i, (r, p) in enumerate(zip(rres, res)):
            assert r[0] == p[0] and same_bits(r[1], p[1]) and (r[0] != 0 or same_bits(r[2], p[2])), (case_id(cs), "Ref != Port", i, r[0], p[0])
        n["ref"] = cs.nb                                      # (device == Port on every LP, Port == Ref on every distinct LP)
    for i, r in enumerate(res):
        if r[0] != 0 or (kind == F64 and (cs.stage1 or lps[i][0] not in bg.EXACT_FAMILIES)):
            continue
        if r[4] != 0:
            n["appro"] += 1
            continue
        check_exact(cs, lps[i], status[i], v[i], sol[i], int(bg.c0_of(i)))        # every qualifying LP
        n["exact"] += 1
    g = f["geom"]
    print("%s threads=%d k_batch<%d> stage1=%s own=%s: port %d, ref %s, exact %d (rescue skipped %d), statuses %s" % (
        case_id(cs), g.threads, 5 if g.five else 4, f["forms"][0], f["forms"][1], n["port"], n["ref"] if ref is not None else "not built",
        n["exact"], n["appro"], np.bincount(status, minlength=5).tolist()))
    if _claims_exact(cs):
        assert 2 * n["exact"] >= len(res), "the exact check ran on %d of %d LPs: %s" % (n["exact"], len(res), case_id(cs))
    return status, v, sol


@pytest.mark.gpu
@pytest.mark.parametrize("cs", CASES, ids=[case_id(cs) for cs in CASES])
def test_kernel_at_launch_geometry(cs, ctx, port, ref_or_none):
    run_case(cs, ctx, port, ref_or_none)


@pytest.mark.gpu
def test_host_routes_leave_unsolved_rows_alone(ctx, port, ref_or_none):
    """batch_host: up to 1 MiB of input through pinned staging (out_sol copied for status 0 only), above it pageable copies
    that upload and download out_sol whole. The same LPs on both sides; on both, rows of LPs that did not end with status 0
    keep the caller's pattern (run_case compares every cell of out_sol) and such LPs exist."""
    a, b = bg.route_cases()
    ra = run_case(a, ctx, port, ref_or_none)
    rb = run_case(b, ctx, port, ref_or_none)
    assert (ra[0] != 0).sum() > 10 and (ra[0] == 0).sum() > 10
    assert same_bits(ra[0], rb[0][:a.nb]) and same_bits(ra[1], rb[1][:a.nb]) and same_bits(ra[2], rb[2][:a.nb])


@pytest.mark.gpu
def test_ragged_call_matches_uniform_call(ctx, port):
    """The same LPs through a uniform call and through ragged calls beside a companion that forces 128 and 256 threads and a
    larger LDS request: identical status, value and solution. Several of them run wave0-fast alone and overlapped beside the
    companion; the 32 x 63 fp64 LPs run the specialised loop in both (a ragged launch carves the LDS per LP)."""
    from xpoly_amd.six import six_batch_ragged
    changed = 0
    for kind, is_max, R, V, s1 in bg.RAGGED_LPS:
        cs = Case(kind, is_max, R, V, 8, s1, bg.MIX, bg.NO_LIMIT, "ragged", "host")
        lps, tg, lq = case_arrays(cs)
        st_u, v_u, sol_u = ctx.six_batch(kind, is_max, tg, lq)
        res = oracle_results(port, "port", cs)
        assert st_u.tolist() == [r[0] for r in res], case_id(cs)
        for t, comp in bg.RAGGED_COMPANIONS.items():
            cc = Case(kind, is_max, comp[0], comp[1], 2, 0, ("ones", "dense"), bg.NO_LIMIT, "ragged companion", "host")
            _, ctg, clq = case_arrays(cc)
            tgs = [ctg[0]] + [tg[i] for i in range(cs.nb)] + [ctg[1]]
            lqs = [clq[0]] + [lq[i] for i in range(cs.nb)] + [clq[1]]
            st_r, v_r, sol_r = six_batch_ragged(ctx, kind, is_max, tgs, lqs)
            assert bg.ragged_threads(kind, [(R, V), comp]) >= t
            changed += bg.loop_forms(kind, R, V, bg.thread_rule(R, V), s1) != bg.loop_forms(kind, R, V, bg.ragged_threads(kind, [(R, V), comp]), s1)
            assert same_bits(st_r[1:-1], st_u), (case_id(cs), t, st_r.tolist(), st_u.tolist())
            assert same_bits(v_r[1:-1], v_u), (case_id(cs), t)
            for i in range(cs.nb):
                if st_u[i] == 0:
                    assert same_bits(sol_r[1 + i], sol_u[i]), (case_id(cs), t, i)
            cres = oracle_results(port, "port", cc)
            assert [int(st_r[0]), int(st_r[-1])] == [r[0] for r in cres], (case_id(cs), t)
    assert changed >= 8


@pytest.mark.gpu
def test_ragged_call_refuses_what_the_uniform_call_refuses(ctx, port):
    """A ragged batch whose largest LP does not fit beside the kernel's own LDS (Rational 126 x 24: its arrays alone fit
    160 KB) is not launched by k_batch_ragged; the class route behind it refuses the LP as the uniform call does, and the
    handle works on."""
    from xpoly_amd._capi import XpgError
    from xpoly_amd.six import six_batch_ragged
    big = [cs for cs in CASES if "refused static LDS" in cs.label and cs.is_max][0]
    assert bg.small_lds_bytes(big.kind, big.R, big.V) <= bg.LDS_MAX and not bg.lds_fits(big.kind, big.R, big.V)
    small = Case(big.kind, 1, 12, 12, 4, 1, ("dep", "chain"), bg.NO_LIMIT, "ragged beside refused", "host")
    _, btg, blq = case_arrays(big)
    _, stg, slq = case_arrays(small)
    with pytest.raises(XpgError, match="XPG_ERR_UNSUPPORTED"):
        six_batch_ragged(ctx, big.kind, 1, [stg[0], btg[0]], [slq[0], blq[0]])
    st, v, sol = six_batch_ragged(ctx, small.kind, 1, list(stg), list(slq))
    assert st.tolist() == [r[0] for r in oracle_results(port, "port", small)]


def _run_worker(**env_over):
    from conftest import hooks_env
    env = hooks_env()                                    # (XPG_BATCH_SLICE_FORCE is a hook-only switch: the -DXPG_TEST_HOOKS build)
    for k in ("XPG_BATCH_SLICE", "XPG_BATCH_SLICE_FORCE"):
        env.pop(k, None)
    env.update(env_over)
    r = subprocess.run([sys.executable, os.path.join(HERE, "batch_geometry_worker.py")], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]


@pytest.mark.gpu
def test_time_slices_at_the_eligibility_edge(port):
    """Forced small slices (7 and 3 iterations per turn, stage 1's solve included) at shapes on both sides of every term of
    the eligibility rule -- R + V = 127 / 128, 64 / 65 rows, 128 / 64 threads -- and on an LP whose stage-1 solve is wave0-fast
    (rhs = 128, never sliced) while its own solve is overlapped and sliced: the same arrays as with slices off, and Port's."""
    off = _run_worker(XPG_BATCH_SLICE="0")
    assert [r["id"] for r in off] == [case_id(cs) for cs in bg.SLICE_CASES]
    for n in ("7", "3"):
        got = _run_worker(XPG_BATCH_SLICE=n, XPG_BATCH_SLICE_FORCE="1")
        for a, b, cs in zip(off, got, bg.SLICE_CASES):
            assert a == b, (n, a["id"], bg.sliced(cs.kind, cs.R, cs.V, cs.nb, force=True), a["status"], b["status"])
    for rec, cs in zip(off, bg.SLICE_CASES):
        res = oracle_results(port, "port", cs)
        assert rec["status"] == [r[0] for r in res], rec["id"]
        for i, r in enumerate(res):
            if r[0] == 0:
                assert rec["v"][16 * i:16 * i + 16] == np.asarray(r[1], dtype=np.float64 if cs.kind == F64 else np.int32).tobytes().hex(), (rec["id"], i)
        print("%s: sliced under the hook: %s, statuses %s" % (rec["id"], bg.sliced(cs.kind, cs.R, cs.V, cs.nb, force=True),
                                                              np.bincount(rec["status"], minlength=5).tolist()))
