"""CPU suite: the Python face (xpoly_amd/six.py, xpoly_amd/lineq.py) seen from below, as tests/test_lineq_collectors_host.py
sees the C++ collectors. tests/python_face_standin.py takes the library's place in xpoly_amd._capi._lib: per call it records
the entry point, every scalar with the ctypes kind the wrapper chose, every pointer as NULL or as element type, length and
contents, then what the face handed back -- each array's dtype, shape and contents, marked `view` where it views the stand-in's
buffer instead of owning its data -- or the exception that came out. The library takes no argtypes, so nothing else in the suite looks at these
choices without a device. The record is compared line for line with tests/golden/g16_python_face_trace.txt, recorded from this
project's own six.py and lineq.py before the face's shared steps (the rows-down function, the route view, the ragged pack, the
list flattening, the has_solution fronts, the paired solvers) were stated once.

`python tests/test_python_face_host.py` prints the trace."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g16_python_face_trace.txt")
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from python_face_standin import StandIn  # noqa: E402


def pairs(*shape, start=1):
    """[..., 2] (num, den) pairs: num counts up from `start`, den is 1"""
    a = np.ones(shape + (2,), dtype=np.int32)
    a[..., 0] = np.arange(start, start + int(np.prod(shape))).reshape(shape)
    return a


def record(setattr_):
    """Every scenario, in the golden file's order. setattr_(obj, name, value) is undone by the caller (monkeypatch.setattr)."""
    import xpoly_amd
    from xpoly_amd import _capi
    sb = StandIn()
    setattr_(_capi, "_lib", sb)
    ctx = xpoly_amd.Context(0)
    try:
        _scenarios(sb, ctx, setattr_)
    finally:
        ctx.close()                                             # while the stand-in is in place: its handle is none of the library's
    return sb.lines


def _scenarios(sb, ctx, setattr_):
    import xpoly_amd
    from xpoly_amd import six
    from xpoly_amd.lineq import Lineq
    F64, RAT = six.F64, six.RAT
    lq = Lineq(ctx)
    run = sb.scenario

    # ---- the six packed calls: 2 systems of 2 rows x 3 columns ----------------------------------------------------------
    A2 = pairs(2, 2, 3)
    none = np.zeros((0, 2, 3, 2), dtype=np.int32)
    packed = {
        "reduce_packed": (lambda m, **k: lq.reduce_packed(m, 2, False, **k), lambda n: n + 1, {}),
        "fme_packed": (lambda m, **k: lq.fme_packed(m, 2, 1, True, 7, **k), lambda n: n + 1, {}),
        "project_packed": (lambda m, **k: lq.project_packed(m, 2, [1, 0], True, 7, 5, **k), lambda n: n + 1, {"out_steps": [2, 1]}),
        "levels_packed": (lambda m, **k: lq.levels_packed(m, 2, [1, 0], False, None, 5, **k), lambda n: 2 * n + 1, {"out_steps": [2, 1]}),
        "calcBound_packed": (lambda m, **k: lq.calcBound_packed(m, 2, **k), lambda n: 2 * n + 1, {}),
        "bounds_packed": (lambda m, **k: lq.bounds_packed(m, 2, 9, **k), lambda n: 2 * n + 1, {"out_chain": [-1, 1], "out_steps": [0, 1]}),
    }
    for name, (fn, noff, extra) in packed.items():
        def answer(nb, extra=extra, noff=noff):
            off = np.minimum(np.arange(noff(nb)), 3)            # 1 row per result until 3 rows are out
            a = dict(row_offsets=off, out_ok=[1, -4][:nb], view=int(off[-1]) * 3 * 2)
            a.update({k: v[:nb] for k, v in extra.items()})
            return a
        copies = (None,) if name == "calcBound_packed" else (True, False)
        for copy in copies:
            kw = {} if copy is None else {"copy": copy}
            run("%s%s" % (name, "" if copy is None else " copy=%s" % copy), lambda: fn(A2, **kw), [answer(2)])
        kw = {} if name == "calcBound_packed" else {"copy": False}
        run("%s: no rows at all%s" % (name, "" if not kw else " under copy=False"), lambda: fn(A2, **kw), [dict(out_ok=[0, 0])])
        run("%s: one system given with three axes" % name, lambda: fn(A2[1]), [answer(1)])
        run("%s: nb == 0" % name, lambda: fn(none), [{}] if name in ("reduce_packed", "fme_packed", "calcBound_packed") else [])
    run("levels_packed: an empty list", lambda: lq.levels_packed(A2, 2, []), [dict(out_ok=[1, 1])])
    run("reduce: the list form", lambda: lq.reduce(A2, 2), [dict(row_offsets=[0, 1, 3], out_ok=[1, 1], view=18)])
    run("fme: the list form", lambda: lq.fme(A2, 2, 0), [dict(row_offsets=[0, 0, 2], out_ok=[0, 1], view=12)])
    run("fme: the slots route", lambda: lq.fme(A2, 2, 0, True, cap_rows=2, slots=True),
        [dict(outs=np.arange(1, 25), out_rows=[1, 2], out_ok=[1, 1])])
    run("fme: the slots route, the default capacity", lambda: lq.fme(A2[0], 2, 0, slots=True), [dict(out_rows=[0], out_ok=[0])])
    run("fme: the slots route needs more rows", lambda: lq.fme(A2, 2, 0, slots=True, cap_rows=2), [dict(out_rows=[1, -5], out_ok=[1, 1])])

    # ---- ragged systems: 2 rows x 3 columns and 1 row x 4 columns -----------------------------------------------------------
    R = [pairs(2, 3), pairs(1, 4, start=7)]
    chain = dict(out_cell_offsets=[0, 3, 7, 15], out_rows=[1, 1, 2], out_ok=[1, 1], out_steps=[1, 2], view=30)
    run("project_ragged copy=True", lambda: lq.project_ragged(R, None, [[1], [2, 1]], True, 6, 4),
        [dict(out_cell_offsets=[0, 3, 11], out_rows=[1, 2], out_ok=[1, 1], out_steps=[1, 2], view=22)])
    run("project_ragged copy=False, rhs_idx given", lambda: lq.project_ragged(R, [2, 3], [[1], [2, 1]], copy=False),
        [dict(out_cell_offsets=[0, 3, 11], out_rows=[1, 2], out_ok=[1, 1], out_steps=[1, 2], view=22)])
    run("project_ragged: no rows at all under copy=False", lambda: lq.project_ragged(R, None, [[1], [2, 1]], copy=False), [dict(out_ok=[0, -9])])
    run("project_ragged: all lists empty", lambda: lq.project_ragged(R, None, [[], []]),
        [dict(out_cell_offsets=[0, 6, 10], out_rows=[2, 1], out_ok=[1, 1], view=20)])
    run("project_ragged: a list too few", lambda: lq.project_ragged(R, None, [[1]]))
    run("project_ragged: an rhs_idx too few", lambda: lq.project_ragged(R, [2], [[1], [2, 1]]))
    run("project_ragged: no systems", lambda: lq.project_ragged([], None, []))
    run("levels_ragged: elims=None, rhs_idx=None, copy=False", lambda: lq.levels_ragged(R, None, copy=False), [chain])
    run("levels_ragged: elims=None, rhs_idx given", lambda: lq.levels_ragged(R, [2, 2], None, True, 6, 4),
        [dict(out_cell_offsets=[0, 3, 7], out_rows=[1, 1], out_ok=[1, 1], out_steps=[1, 1], view=14)])
    run("levels_ragged: all lists empty", lambda: lq.levels_ragged(R, None, [[], []]), [dict(out_ok=[1, 1])])
    run("levels_ragged: a list too many", lambda: lq.levels_ragged(R, None, [[1], [2], [1]]))
    run("levels_ragged: no systems", lambda: lq.levels_ragged([], None))
    bounds = dict(out_cell_offsets=[0, 3, 3, 11], out_rows=[1, 0, 2], out_ok=[1, 0], out_chain=[-1, 0], out_steps=[0, 1], view=22)
    run("bounds_ragged: grouped by rhs_idx[b]", lambda: lq.bounds_ragged(R, [2, 1], 8, 4), [bounds])
    run("bounds_ragged: rhs_idx=None, copy=False", lambda: lq.bounds_ragged(R, copy=False),
        [dict(out_cell_offsets=[0, 3, 3, 7, 7, 15], out_rows=[1, 0, 1, 0, 2], out_ok=[1, 1], out_chain=[-1, -1], view=30)])
    run("bounds_ragged: no rows at all under copy=False", lambda: lq.bounds_ragged(R, [2, 1], copy=False), [dict(out_ok=[0, 0])])
    run("bounds_ragged: an rhs_idx too many", lambda: lq.bounds_ragged(R, [2, 1, 1]))
    run("bounds_ragged: no systems", lambda: lq.bounds_ragged([]))
    run("reduce_ragged", lambda: lq.reduce_ragged(R, [2, 3], False), [dict(out_rows=[1, 1], out_ok=[1, 1])])
    run("reduce_ragged: rhs_idx=None", lambda: lq.reduce_ragged(R), [dict(out_rows=[2, 0], out_ok=[1, 0])])

    # ---- hulls: groups of systems ---------------------------------------------------------------------------------------------
    B3 = pairs(1, 3, start=20)
    hull = dict(out_cell_offsets=[0, 6, 10], out_rows=[2, 1], out_ok=[1, 1], out_member=[-1, -1], out_chain=[-1, -1], view=20)
    run("hull_ragged: no groups", lambda: lq.hull_ragged([]))
    run("hull_ragged: a group without members", lambda: lq.hull_ragged([[R[0], B3], []], is_intersect=True),
        [dict(out_cell_offsets=[0, 3, 3], out_rows=[1, 0], out_ok=[1, 1], view=6)])
    run("hull_ragged: groups but no members", lambda: lq.hull_ragged([[], []], None, False, 5, 6, 7), [dict(out_ok=[1, 1])])
    run("hull_ragged: rhs_idx per group, copy=False", lambda: lq.hull_ragged([[R[0], B3], [R[1]]], [2, 3], copy=False), [hull])
    run("hull_ragged: rhs_idx per member", lambda: lq.hull_ragged([[R[0], B3], [R[1]]], [2, 1, 3]), [hull])
    run("hull_ragged: an rhs_idx too many", lambda: lq.hull_ragged([[R[0], B3], [R[1]]], [2, 1, 3, 3]))
    run("hull_ragged: no rows at all under copy=False", lambda: lq.hull_ragged([[R[0]], [R[1]]], copy=False), [dict(out_ok=[0, -8], out_member=[-1, 0])])
    run("project_union_ragged", lambda: lq.project_union_ragged([[R[0], B3], [R[1]]], None, [[[1], []], [[2, 1]]], True, True, 5, 6, 7), [hull])
    run("project_union_ragged: all lists empty, copy=False", lambda: lq.project_union_ragged([[R[0]], [R[1]]], [2, 3], [[[]], [[]]], copy=False), [hull])
    run("project_union_ragged: a list too few", lambda: lq.project_union_ragged([[R[0], B3], [R[1]]], None, [[[1]], [[2, 1]]]))

    # ---- fme_ragged: one call, or a sizing call and an exact one ---------------------------------------------------------------
    def filled(call):
        call.a["out_cell_offsets"][:] = [0, 3, 7]; call.a["out_rows"][:] = [1, 1]; call.a["out_ok"][:] = [1, 1]
        if "outs" in call.a:
            call.a["outs"][:14] = np.arange(1, 15)
        return 0 if call.s["outs_cap_cells"] >= 7 else -3
    run("fme_ragged: one call", lambda: lq.fme_ragged(R, [1, 2], None, True), [filled])
    run("fme_ragged: one call, rhs_idx given, a return code", lambda: lq.fme_ragged(R, [1, 2], [2, 3]), [dict(rc=-2)])
    setattr_(Lineq, "RAGGED_FME_ONE_CALL_BYTES", 0)
    run("fme_ragged: a sizing call, then the exact one", lambda: lq.fme_ragged(R, [1, 2]), [filled, filled])
    run("fme_ragged: a sizing call that fills nothing", lambda: lq.fme_ragged(R, [1, 2]), [dict(rc=-3)])
    run("fme_ragged: a sizing call that needs nothing", lambda: lq.fme_ragged(R, [1, 2]), [dict(out_ok=[0, 0])])
    setattr_(Lineq, "RAGGED_FME_ONE_CALL_BYTES", 256 << 20)

    # ---- the views: the count passed, the keys returned ------------------------------------------------------------------------
    count = lambda call: int(call.a["out"].__setitem__(slice(None), np.arange(1, call.s["n"] + 1)) or 0)
    for name in ("project_last_route", "levels_last_route", "ragged_last_route", "bounds_last_route", "bounds_ragged_last_route",
                 "hull_ragged_last_route"):
        run("Lineq.%s" % name, getattr(Lineq, name), [count])
    run("Lineq.levels_last_route: a return code", Lineq.levels_last_route, [dict(rc=-3)])
    vc3 = pairs(3, 4)
    for name, tag, args in (("mip_last_route", "", ()), ("mip_hbm_last_route", "", ()), ("six_batch_last_route", "", ()),
                            ("six_batch_hbm_last_route", "", ()), ("six_batch_vc_hbm_last_route", "", ()), ("has_solution_batch_last_route", "", ()),
                            ("has_solution_ragged_last_route", "", ()), ("has_solution_int_last_route", "", ()), ("six_last_profile", "", ()),
                            ("six_batch_hbm_geometry", "", (RAT, 5, 6, 7)), ("six_batch_vc_hbm_plan", ": a vc", (F64, vc3[..., 0], 5, 1, 4, True, 9, 128)),
                            ("six_batch_vc_hbm_plan", ": vc=None", (RAT, None, 5, 1, 4, False, 9)), ("has_solution_batch_plan", ": a vc", (vc3, 5, 1, 4, 9)),
                            ("has_solution_batch_plan", ": vc=None", (None, 5, 1, 4, 9, 64)), ("has_solution_int_plan", "", (vc3, 5, 1, 4, 9))):
        run("six.%s%s" % (name, tag), lambda: getattr(six, name)(*args), [count])
    run("six.mip_hbm_plan", lambda: six.mip_hbm_plan(RAT, vc3, 5, 1, 4, True, False, 9), [dict(out_free=[0, 1, 1], rc=1), count])
    run("six.mip_hbm_plan: vc is no pattern", lambda: six.mip_hbm_plan(F64, vc3[..., 0], 5, 1, 4, False, True, 9, 32), [dict(rc=-3)])
    run("six.has_solution_ragged_plan", lambda: six.has_solution_ragged_plan(vc3, [2, 0], [0, 1]),
        [lambda call: count(call) or call.a["out_route"].__setitem__(slice(None), [0, 3]) or 0])
    run("six.has_solution_ragged_plan: lists of two lengths", lambda: six.has_solution_ragged_plan(vc3, [2, 0], [0]))
    for name in ("mip_last_route", "mip_hbm_last_route", "six_batch_last_route", "six_last_profile"):
        run("six.%s: a return code" % name, getattr(six, name), [dict(rc=-3)])

    # ---- the has_solution fronts: 2 systems under a [2, 3] vc -------------------------------------------------------------------
    vc = pairs(2, 3, start=-2)
    leq, eq = pairs(2, 2, 3), pairs(2, 1, 3, start=30)
    verdict = dict(out_has=[1, -7], out_status=[0, 2, 1, 3])
    fronts = (("has_solution_batch", lambda l, e, **k: six.has_solution_batch(ctx, l, e, vc, False, True, 77, **k)),
              ("has_solution_int_batch", lambda l, e, **k: six.has_solution_int_batch(ctx, l, e, vc, True, **k)))
    for name, fn in fronts:
        run("%s: leq and eq, want_status" % name, lambda: fn(leq, eq, want_status=True), [verdict])
        run("%s: eq=None, integers" % name, lambda: fn(leq[..., 0], None), [dict(out_has=[0, 1])])
        run("%s: leq=None" % name, lambda: fn(None, eq), [dict(out_has=[0, 1])])
        run("%s: both None" % name, lambda: fn(None, None))
        run("%s: another batch size" % name, lambda: fn(leq, eq[:1]))
        run("%s: leq without rows, a return code" % name, lambda: fn(leq[:, :0], eq), [dict(rc=-4)])
    run("has_solution_batch: the defaults, is_int_sol", lambda: six.has_solution_batch(ctx, leq, None, vc, True, False), [dict(out_has=[1, 1])])
    lr, er = [pairs(2, 3), pairs(1, 3, start=9)], [pairs(1, 3, start=40), None]
    fronts = (("has_solution_ragged", lambda l, e, **k: six.has_solution_ragged(ctx, l, e, vc, False, True, 77, **k)),
              ("has_solution_int_ragged", lambda l, e, **k: six.has_solution_int_ragged(ctx, l, e, vc, True, **k)))
    for name, fn in fronts:
        run("%s: eqs=None" % name, lambda: fn(lr, None), [dict(out_has=[1, 0])])
        run("%s: a None system on either side, want_status" % name, lambda: fn([None, lr[1]], er, want_status=True), [verdict])
        run("%s: no equalities anywhere" % name, lambda: fn(lr, [None, np.zeros((0, 3, 2), dtype=np.int32)]), [dict(out_has=[1, 0])])
        run("%s: no inequalities anywhere" % name, lambda: fn([None, None], [er[0], er[0]]), [dict(out_has=[1, 0])])
        run("%s: other columns" % name, lambda: fn([lr[0], pairs(1, 4)], None))
        run("%s: an eqs too few" % name, lambda: fn(lr, er[:1]))
    run("has_solution_ragged: the defaults, is_int_sol", lambda: six.has_solution_ragged(ctx, lr, er, vc, True, False), [dict(out_has=[1, 1])])
    for args in ((2, 1, 2, None, 0, 3, 3, True, 4), (2, 0, 0, 2, 1, 3, 3, False, 4, 5, 55, True), (2, 1, 2, 0, 0, 3, 3, False, 4, 0)):
        run("has_solution_batch_dev", lambda: ctx.has_solution_batch_dev(*args), [{}])

    # ---- the paired batch solvers: 2 problems of 1 row x 3 columns --------------------------------------------------------------
    def solved(kind, nodes=None):
        a = dict(out_status=[0, 3], out_v=[5, 1, 6, 1] if kind == RAT else [5.5, 6.5], out_sol=np.arange(1, 7 if kind == F64 else 13))
        if nodes is not None:
            a["nodes"] = nodes
        return a
    tg, lq1, eq1 = pairs(2, 3, start=50), pairs(2, 1, 3), pairs(2, 1, 3, start=30)
    as_f = lambda a: None if a is None else a[..., 0] * 0.5
    for kind, cast in ((F64, as_f), (RAT, lambda a: a)):
        k = "F64" if kind == F64 else "RAT"
        run("Context.six_batch %s" % k, lambda: ctx.six_batch(kind, True, cast(tg), cast(lq1)), [solved(kind)])
        run("six_batch_hbm %s" % k, lambda: six.six_batch_hbm(ctx, kind, False, cast(tg), cast(lq1), 99), [solved(kind)])
        for name in ("six_batch_vc", "six_batch_vc_hbm"):
            run("%s %s" % (name, k), lambda: getattr(six, name)(ctx, kind, True, cast(tg), cast(vc), cast(lq1), cast(eq1), 99), [solved(kind)])
        if kind == RAT:
            run("six_batch_vc RAT: eq=None", lambda: six.six_batch_vc(ctx, kind, False, tg, vc, lq1), [solved(kind)])
        run("six_batch_vc_hbm %s: leq=None, a return code" % k, lambda: six.six_batch_vc_hbm(ctx, kind, False, cast(tg), cast(vc), None, cast(eq1)), [dict(rc=-4)])
        run("mip_batch_vc %s" % k, lambda: six.mip_batch_vc(ctx, True, False, cast(tg), cast(vc), cast(lq1), cast(eq1), [1, 0, 0], kind=kind), [solved(kind, 12)])
        run("mip_batch_vc_hbm %s" % k, lambda: six.mip_batch_vc_hbm(ctx, False, True, cast(tg), cast(vc), cast(lq1), None, None, kind), [solved(kind, 1 << 40)])
    run("mip_batch_vc: the defaults", lambda: six.mip_batch_vc(ctx, True, True, tg, vc, None, eq1), [solved(RAT, 3)])
    run("mip_batch_vc_hbm: the defaults, ind", lambda: six.mip_batch_vc_hbm(ctx, True, True, tg, vc, lq1, ind=[0, 1, 0]), [solved(RAT, 3)])
    run("six_batch_vc: vc of another shape", lambda: six.six_batch_vc(ctx, RAT, True, tg, vc3, lq1))
    run("six_batch_vc_hbm: leq of another batch size", lambda: six.six_batch_vc_hbm(ctx, RAT, True, tg, vc, lq1[:1]))

    def given(fn, kind):
        out = (np.full(2, 9, dtype=np.int32), six.empty_kind((2,), kind), six.empty_kind((2, 3), kind))
        res = fn(out)
        return res, "the arrays given" if all(r is o for r, o in zip(res, out)) else "other arrays"
    run("six_batch_hbm: out=", lambda: given(lambda out: six.six_batch_hbm(ctx, F64, True, as_f(tg), as_f(lq1), out=out), F64), [dict(out_status=[0, 0])])
    run("six_batch_vc_hbm: out=", lambda: given(lambda out: six.six_batch_vc_hbm(ctx, RAT, True, tg, vc, lq1, out=out), RAT), [dict(out_status=[0, 0])])
    for pivots in ((), (0,), (9, 44)):
        run("six_batch_dev, six_batch_hbm_dev: pivots_ptr %s" % (pivots[:1] or "left out",),
            lambda: (ctx.six_batch_dev(F64, True, 2, 1, 2, 1, 3, 3, 4, 5, *pivots), ctx.six_batch_hbm_dev(RAT, False, 2, 1, 2, 1, 3, 3, 4, 5, *pivots)), [{}, {}])
    for eqp, lqp, tail in ((None, 8, ()), (0, 8, (33,)), (7, None, ()), (7, 0, ())):
        run("six_batch_vc_dev, six_batch_vc_hbm_dev: eq_ptr %s, leq_ptr %s" % (eqp, lqp),
            lambda: (ctx.six_batch_vc_dev(RAT, True, 2, 1, 2, eqp, 1, lqp, 1, 3, 3, 4, 5, *tail),
                     ctx.six_batch_vc_hbm_dev(F64, False, 2, 1, 2, eqp, 1, lqp, 1, 3, 3, 4, 5, *((9,) + tail if tail else ()))), [{}, {}])
    run("six_batch_vc_hbm_dev: pivots_ptr 0, a return code", lambda: ctx.six_batch_vc_hbm_dev(F64, False, 2, 1, 2, 7, 1, 8, 1, 3, 3, 4, 5, 0), [dict(rc=-4)])

    # ---- SIX._solve / MIP._solve: -7 is an answer, any other negative status is raised -------------------------------------------
    t1, l1, e1 = pairs(3, start=50), pairs(1, 3), pairs(2, 3, start=30)
    one = lambda kind: dict(out_v=[7, 2] if kind == RAT else [3.5], out_sol=np.arange(1, 4 if kind == F64 else 7))
    s64, srat = xpoly_amd.SIX(ctx, F64), xpoly_amd.SIX(ctx, RAT)
    srat.set_param(0, 123)
    run("SIX.maxm F64", lambda: s64.maxm(as_f(t1), as_f(vc), as_f(e1), as_f(l1)), [one(F64)])
    run("SIX.minm RAT: set_param, eq=None, status -7", lambda: srat.minm(t1, vc, None, l1), [dict(one(RAT), rc=-7)])
    run("SIX.minm F64: leq without rows, status 2", lambda: s64.minm(as_f(t1), as_f(vc), as_f(e1), []), [dict(one(F64), rc=2)])
    run("SIX.maxm RAT: status -1", lambda: srat.maxm(t1, vc, e1, l1), [dict(rc=-1)])
    m64, mrat = six.MIP(ctx, F64), six.MIP(ctx, RAT)
    run("MIP.maxm RAT: rational_indicator", lambda: mrat.maxm(t1, vc, e1, l1, True, [0, 1, 0]), [one(RAT)])
    run("MIP.minm F64: the defaults, leq=None, status -7", lambda: m64.minm(as_f(t1), as_f(vc), as_f(e1), None), [dict(one(F64), rc=-7)])
    run("MIP.minm RAT: status -3", lambda: mrat.minm(t1, vc, None, l1), [dict(rc=-3)])
    run("MIP.maxm F64: status 4", lambda: m64.maxm(as_f(t1), as_f(vc), [], as_f(l1), is_bin=True), [dict(one(F64), rc=4)])


@pytest.fixture(scope="module")
def trace():
    mp = pytest.MonkeyPatch()
    try:
        return record(mp.setattr)
    finally:
        mp.undo()


def test_the_trace_is_the_recorded_one(trace):
    want = open(GOLDEN).read().splitlines()
    for k, (g, w) in enumerate(zip(trace, want)):
        assert g == w, "line %d" % (k + 1)
    assert len(trace) == len(want)


def test_the_stand_in_is_gone_again(trace):
    from xpoly_amd import _capi
    assert not isinstance(_capi._lib, StandIn)


def test_the_record_holds_what_it_should():
    lines = open(GOLDEN).read().splitlines()
    sc, name = {}, None
    for ln in lines:
        if ln.startswith("== "):
            name = ln[3:]
            sc[name] = []
        else:
            sc[name].append(ln)
    calls = lambda n: [ln for ln in sc[n] if ln.startswith("  call ")]
    for name, body in sc.items():                                   # the calls, then what came out
        assert body[-1][:10] in ("  returns ", "  raises X", "  raises V") and all(ln.startswith("  call ") for ln in body[:-1]), name
    # a view of the stand-in's buffer only where copy=False was asked for AND there are rows; everything else owns its data
    for name, body in sc.items():
        if any("view:" in ln for ln in body if ln.startswith("  returns")):
            assert "copy=False" in name and "no rows" not in name, name
    for name in ("reduce_packed", "fme_packed", "project_packed", "levels_packed", "bounds_packed"):
        assert "view:" in sc[name + " copy=False"][-1] and "view:" not in sc[name + " copy=True"][-1]
        assert "view:" not in sc[name + ": no rows at all under copy=False"][-1]
    # nb == 0: project, levels and bounds answer before any call, reduce and fme make it
    assert [len(calls(n + ": nb == 0")) for n in ("reduce_packed", "fme_packed", "project_packed", "levels_packed", "bounds_packed")] == [1, 1, 0, 0, 0]
    # empty lists go down as one zero, groups without members as NULL
    assert "elim=i[0] (room 4 bytes:0)" in calls("project_ragged: all lists empty")[0]
    assert "mats=NULL rows=NULL cols=NULL offsets=NULL" in calls("hull_ragged: groups but no members")[0]
    # the sizing path: -3 with the offsets filled, then exactly that many cells; a need of 0 makes no second call
    first, second = calls("fme_ragged: a sizing call, then the exact one")
    assert "outs=NULL outs_cap_cells=l:0" in first and first.endswith("-> -3") and "outs_cap_cells=l:7" in second
    assert len(calls("fme_ragged: a sizing call that needs nothing")) == 1
    assert sc["fme_ragged: a sizing call that fills nothing"][-1].startswith("  raises XpgError")
    # -7 is an answer of SIX / MIP, any other negative status is raised
    assert sc["SIX.minm RAT: set_param, eq=None, status -7"][-1].startswith("  returns (int:-7")
    assert sc["SIX.maxm RAT: status -1"][-1].startswith("  raises XpgError") and sc["MIP.minm RAT: status -3"][-1].startswith("  raises XpgError")
    assert "the arrays given" in sc["six_batch_hbm: out="][-1] and "the arrays given" in sc["six_batch_vc_hbm: out="][-1]
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "g15_collectors_trace.txt"))


if __name__ == "__main__":
    saved = []

    def _set(obj, name, value):
        saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)
    try:
        print("\n".join(record(_set)))
    finally:
        for obj, name, value in reversed(saved):
            setattr(obj, name, value)
