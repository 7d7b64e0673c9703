"""GPU parity of the transformed-nest entry points (xpg_lineq_transform_levels_batch_*: det, T^-1, A * T^-1 and every level of
the fme loop in one launch of k_transform_levels_batch) against the composed CPU checker of tests/lineq_transform_cases.py --
rat_det, rat_inv, rat_op cell by cell in operator*'s order, stepped_levels -- with the restatement always and with the real
reference where its build is present, plus an independent check in exact fractions. Bit for bit: nothing is compared with a
tolerance, no case is filtered."""
import os
import subprocess

import numpy as np
import pytest

import lineq_transform_cases as tc
from lineq_transform_cases import XPG_ERR_SHAPE, rows_equal, transformed

pytestmark = pytest.mark.gpu

DEPTHS = [(n, consts) for n in (1, 2, 3, 4) for consts in (1, 2)]


@pytest.fixture(scope="module")
def lq(ctx):
    from xpoly_amd.lineq import Lineq
    return Lineq(ctx)


@pytest.fixture(scope="module")
def checkers(port):
    from oracle.checker import Ref
    return [port] + ([Ref()] if Ref.available() else [])


def _dev_form(ctx):
    """Lineq.transform_levels_packed's arguments and answer through xpg_lineq_transform_levels_batch_rat32_dev: upload, enqueue,
    synchronise, download, the levels cut out of their slots by the counts. The capacities a device caller must state are the
    ones the packed call settles on (the plan view), an explicit cap_out_rows passed on as it is; mode 1 passes no d_out_det."""
    from xpoly_amd.lineq import _stack, transform_levels_dev

    def call(mats, tmats, rhs_idx, mode=0, shared_nest=False, cap_rows=None, cap_out_rows=None):
        a, t = _stack(mats), _stack(tmats)
        nb, n = t.shape[0], rhs_idx
        rows, cols = a.shape[1:3]
        assert a.shape[0] == (1 if shared_nest else nb)
        p = tc.plan_view(nb, rows, cols, n, cap_rows or 0, 0)
        cap, cap_out = p["cap"], cap_out_rows or p["cap_out"]
        sizes = (a.nbytes, t.nbytes, nb * n * max(cap_out, rows) * cols * 8, nb * n * 4, nb * 4, nb * 4, nb * 4, nb * 8, nb * n * n * 8)
        ptrs = [ctx.malloc(sz) for sz in sizes]
        try:
            ctx.upload(ptrs[0], a); ctx.upload(ptrs[1], t)
            ctx.upload(ptrs[8], np.zeros((nb, n, n, 2), dtype=np.int32))            # (left alone for kind 1 and 2)
            outs_at = ptrs[2:7] + [ptrs[7] if mode == 0 else None, ptrs[8]]
            transform_levels_dev(ctx, nb, ptrs[0], shared_nest, ptrs[1], rows, cols, n, mode, cap, cap_out, *outs_at)
            ctx.sync()
            outs = ctx.download(np.zeros((nb, n, cap_out, cols, 2), dtype=np.int32), ptrs[2])
            r = ctx.download(np.zeros((nb, n), dtype=np.int32), ptrs[3])
            ok, steps, kind = (ctx.download(np.zeros(nb, dtype=np.int32), q) for q in ptrs[4:7])
            det = ctx.download(np.zeros((nb, 2), dtype=np.int32), ptrs[7]) if mode == 0 else None
            mult = ctx.download(np.zeros((nb, n, n, 2), dtype=np.int32), ptrs[8])
        finally:
            for q in ptrs:
                ctx.free(q)
        assert (r >= 0).all() and (r <= cap_out).all()
        return ok, steps, kind, det, mult, [[outs[b, k, : r[b, k]] for k in range(n)] for b in range(nb)]
    return call


@pytest.fixture(scope="module", params=["packed", "dev"])
def form(request, ctx, lq):
    """Every case of sections 1 to 4 runs through both entry points: the host arrays' and the device arrays'."""
    return lq.transform_levels_packed if request.param == "packed" else _dev_form(ctx)


def _caps(nb, a, n, cap_rows=0, cap_out_rows=0):
    """The capacities a call settles on (host-only plan view): what the checker is given."""
    p = tc.plan_view(nb, a.shape[0], a.shape[1], n, cap_rows, cap_out_rows)
    return p["cap"], p["cap_out"]


def _wants(lib, pairs, mode=0, cap_rows=0, cap_out_rows=0):
    """[transformed(...)] for [(nest, T)], each distinct pair computed once; the checker must not approximate."""
    memo, out = {}, []
    before = lib.appro_count()
    for a, t in pairs:
        key = (a.tobytes(), t.tobytes())
        if key not in memo:
            cap, cap_out = _caps(len(pairs), a, t.shape[0], cap_rows, cap_out_rows)
            memo[key] = transformed(lib, a, t, mode, cap, cap_out)
        out.append(memo[key])
    assert lib.appro_count() == before
    return out


def _mixed(nb):
    """nb systems of depth 3, every kind of T against a nest with points and one without, so that the verdict kinds of
    neighbours differ: [(nest, T)]."""
    nests = (tc.nest(3), tc.empty_nest(3, 1))
    ts = list(tc.tmats(3).values())
    return [(nests[(b // 2) % 2], ts[b % len(ts)]) for b in range(nb)]


# ---- 1. every kind of T at every depth -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,consts", DEPTHS)
def test_every_kind_of_t_at_every_depth(lq, form, checkers, n, consts):
    a = tc.nest(n, consts)
    kinds = tc.tmats(n)
    ts = np.stack(list(kinds.values()))
    got = form(a, ts, n, shared_nest=True)
    assert lq.transform_last_route()["launches"] == 1
    for lib in checkers:
        want = _wants(lib, [(a, t) for t in ts])
        tc.check(got, want, (n, consts, lib.prefix))
    assert set(got[2].tolist()) == {0, 1, 2}
    for b, t in enumerate(ts):
        if got[2][b] == 0:
            assert got[0][b] == 1 and got[1][b] == n - 1 and len(got[5][b]) == n
            tc.exact_check(a, t, got[4][b], got[5][b][0], 0)
    # one nest per transformation: identical inputs, identical results
    per = form(np.stack([a] * len(ts)), ts, n)
    assert all(np.array_equal(x, y) for x, y in zip(got[:5], per[:5]))
    assert all(rows_equal(x, y) for lb, pb in zip(got[5], per[5]) for x, y in zip(lb, pb))


# ---- 2. verdicts -----------------------------------------------------------------------------------------------------------------
def test_a_nest_without_points_ends_at_the_step_the_transformation_leaves_it(lq, form, port):
    a = tc.empty_nest(3, 1)
    ts = np.stack([tc.tmats(3)[k] for k in ("identity", "dense", "interchange")])
    got = form(a, ts, 3, shared_nest=True)
    tc.check(got, _wants(port, [(a, t) for t in ts]))
    assert got[0].tolist() == [0, 0, 0] and got[1].tolist() == [1, 0, 1] and got[2].tolist() == [0, 0, 0]
    assert all(lv.shape[0] == 0 for b in range(3) for lv in got[5][b])              # level 0 included
    assert np.array_equal(got[4][0], tc.tmats(3)["identity"])                       # the multiplier is there all the same


def test_a_short_cap_rows_is_reported_with_its_step(lq, form, port):
    a = tc.nest(3)
    ts = np.stack([tc.tmats(3)[k] for k in ("identity", "dense", "lower")])
    got = form(a, ts, 3, shared_nest=True, cap_rows=8)
    tc.check(got, _wants(port, [(a, t) for t in ts], cap_rows=8))
    assert got[0].tolist() == [1, -9, 1] and got[1].tolist() == [2, 1, 2]
    assert all(lv.shape[0] == 0 for lv in got[5][1]) and got[5][0][0].shape[0] == 6
    # once more with the need reported: every step fits
    again = form(a, ts, 3, shared_nest=True, cap_rows=9)
    tc.check(again, _wants(port, [(a, t) for t in ts], cap_rows=9))
    assert again[0].tolist() == [1, 1, 1]


def test_a_short_level_slot_is_reported_with_its_level(lq, form, port):
    a = tc.nest(4, 2)
    ts = np.stack([tc.tmats(4)[k] for k in ("identity", "dense", "upper")])
    got = form(a, ts, 4, shared_nest=True, cap_out_rows=10)
    tc.check(got, _wants(port, [(a, t) for t in ts], cap_out_rows=10))
    cap = tc.plan_view(3, 8, 6, 4, 0, 10)["cap"]
    assert got[0].tolist() == [1, -11, 1] and got[1].tolist() == [3, 2, 3] and 10 < 11 <= cap     # the level, not the step
    with pytest.raises(Exception, match="XPG_ERR_SHAPE"):                           # a slot that cannot hold the nest
        form(a, ts, 4, shared_nest=True, cap_out_rows=7)
    assert lq.transform_last_route()["launches"] == 0


def test_a_non_canonical_cell_in_the_nest(lq, form, checkers):
    """A cell 2/2 among the nest's variable columns: the product takes the arithmetic that reduces as the reference's operators
    do, whatever T is, and the constant columns travel bit for bit (a 2/2 there stays 2/2 at level 0)."""
    for n, consts, cell in ((3, 1, (1, 0)), (3, 2, (1, 4)), (2, 1, (3, 1))):
        a = tc.nest(n, consts).copy()
        assert tuple(a[cell]) == (1, 1)
        a[cell] = (2, 2)
        ts = np.stack([tc.tmats(n)[k] for k in ("identity", "dense", "upper", "noncanonical")])
        got = form(a, ts, n, shared_nest=True)
        for lib in checkers:
            tc.check(got, _wants(lib, [(a, t) for t in ts]), (n, cell, lib.prefix))
        assert got[0].tolist() == [1] * 4 and not got[2].any()
        if cell[1] >= n:
            assert all(tuple(got[5][b][0][cell]) == (2, 2) for b in range(4))


# ---- 3. batches ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 3, 65])
def test_batches_with_mixed_verdicts(lq, form, checkers, nb):
    pairs = _mixed(nb)
    got = form(np.stack([a for a, _ in pairs]), np.stack([t for _, t in pairs]), 3)
    for lib in checkers:
        want = _wants(lib, pairs)
        tc.check(got, want, (nb, lib.prefix))
    if nb == 65:
        assert {(w[0], w[2]) for w in want} == {(1, 0), (0, 0), (1, 1), (1, 2)}
        # a neighbour's failure leaves a system alone: good systems sit next to one of each other kind
        beside = {(want[c][0], want[c][2]) for b in range(1, nb - 1) if (want[b][0], want[b][2]) == (1, 0) for c in (b - 1, b + 1)}
        assert beside >= {(0, 0), (1, 1), (1, 2)}, beside


def test_seats_take_a_second_system_above_the_grid(lq, form, port):
    a = tc.nest(3)
    base = list(tc.tmats(3).values())
    nb = 4096 + 300
    ts = np.stack([base[b % len(base)] for b in range(nb)])
    want = _wants(port, [(a, t) for t in base])
    got = form(a, ts, 3, shared_nest=True)
    route = lq.transform_last_route()
    planned = tc.plan(nb, 6, 4, 3)
    assert route == {k: planned[k] for k in tc.ROUTE_KEYS} == {k: tc.plan_view(nb, 6, 4, 3)[k] for k in tc.ROUTE_KEYS}
    seats = route["grid"] * route["groups"]
    assert route["launches"] == 1 and nb > seats == 4096
    # a seat's second system follows one that ended at kind 1 or 2
    assert any(want[b % len(base)][2] != 0 and want[(b + seats) % len(base)][2] == 0 for b in range(nb - seats))
    tc.check(got, [want[b % len(base)] for b in range(nb)])
    per = form(np.ascontiguousarray(np.broadcast_to(a, (nb,) + a.shape)), ts, 3)
    assert all(np.array_equal(x, y) for x, y in zip(got[:5], per[:5]))
    assert all(rows_equal(x, y) for lb, pb in zip(got[5], per[5]) for x, y in zip(lb, pb))


# ---- 4. the multiplier given ---------------------------------------------------------------------------------------------------
def test_mode_1_with_the_checkers_inverse_gives_mode_0s_levels(lq, form, port):
    a = tc.nest(4, 2)
    names = [k for k, t in tc.tmats(4).items() if tc.kind_of(port, t)[0] == 0]
    ts = np.stack([tc.tmats(4)[k] for k in names])
    before = port.appro_count()
    ms = np.stack([port.rat_inv(t)[1] for t in ts])
    assert port.appro_count() == before
    m0 = form(a, ts, 4, shared_nest=True)
    m1 = form(a, ms, 4, mode=1, shared_nest=True)
    assert m1[3] is None and np.array_equal(m1[4], ms) and np.array_equal(m0[4], ms)
    assert np.array_equal(m0[0], m1[0]) and np.array_equal(m0[1], m1[1]) and not m1[2].any()
    assert all(rows_equal(x, y) for lb, pb in zip(m0[5], m1[5]) for x, y in zip(lb, pb))


def test_mode_1_with_an_hnf_multiplier_equals_the_composition(lq, form, port):
    """The reference's second branch (ldtran.cpp:203-257): T not unimodular, Ui from INTMat::hnf, the levels of A * Ui."""
    for n, consts in ((2, 1), (3, 2), (4, 1)):
        a = tc.nest(n, consts)
        t = tc.tmats(n)["diag2"][..., 0].copy()
        t[n - 1, 0] = 1                                                             # so that Ui is not the identity
        st, h, ui = port.int_hnf(t)
        assert np.array_equal(t.astype(np.int64) @ ui, h) and np.abs(ui).max() <= 3
        m = tc.to_rat(ui)
        kinds = form(a, tc.to_rat(t), n, shared_nest=True)
        assert kinds[2].tolist() == [2] and tuple(kinds[3][0]) == (2, 1)
        got = form(a, m, n, mode=1, shared_nest=True)
        tc.check(got, _wants(port, [(a, m)], mode=1), (n,))
        tc.exact_check(a, m, got[4][0], got[5][0][0], 1)


# ---- 5. device form --------------------------------------------------------------------------------------------------------------
def test_the_device_form_equals_the_host_form(ctx, lq):
    from xpoly_amd.lineq import transform_levels_dev
    pairs = _mixed(65)
    nests, ts = np.stack([a for a, _ in pairs]), np.stack([t for _, t in pairs])
    nb, rows, cols, n = 65, 6, 4, 3
    cap, cap_out = _caps(nb, nests[0], n)
    host = lq.transform_levels_packed(nests, ts, n)
    sizes = (nests.nbytes, ts.nbytes, nb * n * cap_out * cols * 8, nb * n * 4, nb * 4, nb * 4, nb * 4, nb * 8, nb * n * n * 8)
    ptrs = [ctx.malloc(s) for s in sizes]
    try:
        ctx.upload(ptrs[0], nests); ctx.upload(ptrs[1], ts)
        ctx.upload(ptrs[8], np.zeros((nb, n, n, 2), dtype=np.int32))                # (left alone for kind 1 and 2)
        for _ in range(2):                                                          # two calls in a row on one context
            transform_levels_dev(ctx, nb, ptrs[0], False, ptrs[1], rows, cols, n, 0, cap, cap_out, *ptrs[2:])
            ctx.sync()
            assert lq.transform_last_route()["launches"] == 1
            outs = ctx.download(np.zeros((nb, n, cap_out, cols, 2), dtype=np.int32), ptrs[2])
            r = ctx.download(np.zeros((nb, n), dtype=np.int32), ptrs[3])
            ok, steps, kind = (ctx.download(np.zeros(nb, dtype=np.int32), p) for p in ptrs[4:7])
            det = ctx.download(np.zeros((nb, 2), dtype=np.int32), ptrs[7])
            mult = ctx.download(np.zeros((nb, n, n, 2), dtype=np.int32), ptrs[8])
            assert (r >= 0).all() and (r <= cap_out).all()
            for x, y in zip((ok, steps, kind, det, mult), host[:5]):
                assert np.array_equal(x, y)
            assert all(rows_equal(outs[b, k, : r[b, k]], host[5][b][k]) for b in range(nb) for k in range(n))
        # the capacities are the caller's: none is defaulted, a level's slot holds the nest
        for c, co in ((0, 0), (5, 5), (16, 17), (16, 0), (16, 5)):
            with pytest.raises(Exception, match="XPG_ERR_SHAPE"):
                transform_levels_dev(ctx, nb, ptrs[0], False, ptrs[1], rows, cols, n, 0, c, co, *ptrs[2:])
            assert lq.transform_last_route()["launches"] == 0
        transform_levels_dev(ctx, 0, ptrs[0], False, ptrs[1], rows, cols, n, 0, cap, cap_out, *ptrs[2:])
        assert lq.transform_last_route()["launches"] == 0
    finally:
        for p in ptrs:
            ctx.free(p)
    none = lq.transform_levels_packed(nests[:0], ts[:0], n)
    assert len(none[0]) == 0 and none[5] == []


def test_a_sizing_call_and_a_buffer_one_row_short(ctx, lq):
    import ctypes as C
    from xpoly_amd._capi import lib, vp
    a = tc.nest(3)
    ts = np.stack(list(tc.tmats(3).values()))
    nb = len(ts)
    off = np.zeros(nb * 3 + 1, dtype=np.int64)
    ok, steps, kind = (np.zeros(nb, dtype=np.int32) for _ in range(3))
    det = np.zeros((nb, 2), dtype=np.int32); mult = np.zeros((nb, 3, 3, 2), dtype=np.int32)
    head = (ctx._h, C.c_int(nb), vp(a), C.c_int(1), vp(ts), C.c_int(6), C.c_int(4), C.c_int(3), C.c_int(0), C.c_int(0), C.c_int(0))
    tail = (None, vp(off), vp(ok), vp(steps), vp(kind), vp(det), vp(mult))
    fn = lib().xpg_lineq_transform_levels_batch_packed_rat32
    assert fn(*head, None, C.c_longlong(0), *tail) == 0 and off[-1] > 0
    total = int(off[-1])
    out = np.zeros((total, 4, 2), dtype=np.int32)
    off[:] = 0; steps[:] = -1; mult[:] = 0
    assert fn(*head, vp(out), C.c_longlong(total - 1), *tail) == XPG_ERR_SHAPE
    assert off[-1] == total and (steps >= 0).all() and mult.any()
    assert fn(*head, vp(out), C.c_longlong(total), *tail) == 0
    want = lq.transform_levels_packed(a, ts, 3, shared_nest=True)
    assert all(rows_equal(out[off[b * 3 + k]: off[b * 3 + k + 1]], want[5][b][k]) for b in range(nb) for k in range(3))
    assert np.array_equal(mult, want[4]) and np.array_equal(det, want[3])


# ---- 6. adapter ------------------------------------------------------------------------------------------------------------------
def _parse(lines):
    """{name: [rows of (num, den)]} of the `<name> <r> <c> n/d ...` lines, in order of appearance per name."""
    out = {}
    for ln in lines:
        p = ln.split()
        r, c = int(p[1]), int(p[2])
        cells = np.array([[int(x) for x in q.split("/")] for q in p[3:]], dtype=np.int32).reshape(r, c, 2)
        out.setdefault(p[0], []).append(cells)
    return out


def _fr(m):
    return [[tc.Fraction(int(c[0]), int(c[1])) for c in row] for row in m]


def test_the_adapter_runs_transform_iter_space_and_the_search(port, tmp_path):
    """tests/cxx/transform_iter_space.cpp in a child process: LoopTran::transformIterSpace on a unimodular and on a nonsingular
    T and a singular one, transform_levels_all on a shared nest of 65 T and on one nest per T; its printed cells against the
    checker's."""
    from test_transform_abi_host import build_iter_space_test
    exe = build_iter_space_test()
    n, a = 3, tc.nest(3)
    ints = [t[..., 0] for k, t in tc.tmats(n).items() if k != "noncanonical"]
    non = tc.tmats(n)["diag2"][..., 0].copy(); non[n - 1, 0] = 1
    ts = [tc.tmats(n)["dense"][..., 0], non, tc.tmats(n)["singular"][..., 0]] + [ints[b % len(ints)] for b in range(62)]
    lines = ["%d %d %d" % (n, a.shape[0], a.shape[1]), " ".join(str(int(x)) for x in a[..., 0].ravel()), str(len(ts))]
    lines += [" ".join(str(int(x)) for x in t.ravel()) for t in ts]
    path = str(tmp_path / "nest.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    out = r.stdout.strip().split("\n")
    at = [i for i, ln in enumerate(out) if ln.startswith(("iter ", "all ", "each "))]
    assert [out[i] for i in at] == ["iter 0 uni 1 status 0", "iter 1 uni 0 status 0", "all rc 0", "each rc 0 same 1"]
    assert out[at[3] + 1:] == ["singular uni 0 status 1 alone 1"]                   # false, and every argument left as it was
    # transformIterSpace, unimodular: one mode 0 call
    w = transformed(port, a, tc.to_rat(ts[0]))
    g = _parse(out[at[0] + 1: at[1]])
    assert g["stride"][0][..., 0].tolist() == [[1] * n] and g["ofst"][0].size == 0 and g["mul"][0].size == 0
    assert np.array_equal(g["idx_map"][0], w[4]) and rows_equal(g["trA"][0], w[5][0])
    assert all(rows_equal(g["limit%d" % j][0], w[5][n - 1 - j]) for j in range(n))          # head .. tail
    # nonsingular: hnf, H^-1, one mode 1 call with Ui, the rest on the host
    st, h, ui = port.int_hnf(non)
    hi = _fr(port.rat_inv(tc.to_rat(h))[1])
    w = transformed(port, a, tc.to_rat(ui), mode=1)
    g = _parse(out[at[1] + 1: at[2]])
    mul = lambda x, y: [[sum(x[i][k] * y[k][j] for k in range(n)) for j in range(n)] for i in range(len(x))]
    diag = [[tc.Fraction(int(h[i, i])) for i in range(n)]]
    assert _fr(g["stride"][0]) == diag and _fr(g["mul"][0]) == diag
    assert _fr(g["idx_map"][0]) == mul(_fr(tc.to_rat(ui)), hi)
    assert mul(_fr(g["idx_map"][0]), _fr(tc.to_rat(non))) == [[tc.Fraction(int(i == j)) for j in range(n)] for i in range(n)]
    assert _fr(g["ofst"][0]) == mul(_fr(tc.to_rat(np.tril(h, -1))), hi)
    assert rows_equal(g["trA"][0], w[5][0]) and all(rows_equal(g["limit%d" % j][0], w[5][n - 1 - j]) for j in range(n))
    # the search: 65 T on the shared nest
    heads = [ln.split() for ln in out[at[2] + 1: at[3]] if ln.startswith("t ")]
    g = _parse([ln for ln in out[at[2] + 1: at[3]] if not ln.startswith("t ")])
    assert len(heads) == 65
    want = _wants(port, [(a, tc.to_rat(t)) for t in ts])
    for b, (hd, w) in enumerate(zip(heads, want)):
        assert (int(hd[3]), int(hd[5]), int(hd[7])) == (w[0], w[1], w[2]) and hd[9] == "%d/%d" % tuple(w[3]), (b, hd, w[:4])
        assert (g["invt"][b].size == 0) if w[2] else np.array_equal(g["invt"][b], w[4]), b
        assert all(rows_equal(g["level%d" % k][b], w[5][k]) for k in range(n)), b
    assert {int(hd[7]) for hd in heads} == {0, 1, 2}
