"""GPU parity of the hull calls (xpg_lineq_hull_batch_ragged_rat32: calcBound on every member of many lists of polyhedra in one
launch, then k_group_reduce, ONE reduce per list, in a second; xpg_lineq_project_union_batch_ragged_rat32: the same behind the
ragged fme chain) against Lineq::ConvexHullUnionAndIntersect composed from the CPU checker's fme and reduce
(tests/lineq_hull_cases.py), against the reference's own build where it is present, and against the composition of the two
existing device calls. Bit-exact: nothing is compared with a tolerance. The facts the cases rest on -- which groups are empty,
which members fail and how, how many rows a group gathers, which home it gets -- are asserted on the checker's answers and the
plan view BEFORE anything is asserted of the device.
  The home of a group is a rule of the shapes alone (its gathered CAPACITY against the LDS rows of the call), so the plan view
states it; test 4 also has a group whose gathered ROWS, as the checker counts them, exceed the LDS rows."""
import ctypes as C

import numpy as np
import pytest

import lineq_bounds_cases as bc
import lineq_hull_cases as hc
import lineq_project_cases as pc
from lineq_hull_cases import XPG_ERR_SHAPE, XPG_ERR_UNSUPPORTED, rows_equal

pytestmark = pytest.mark.gpu

CAP = 512                                                    # cap_rows of the members: no step of the batch needs more


@pytest.fixture(scope="module")
def lq(ctx):
    from xpoly_amd.lineq import Lineq
    return Lineq(ctx)


@pytest.fixture(scope="module")
def batch(port):
    return hc.hull_batch(port)


@pytest.fixture(scope="module")
def wants(port, batch):
    """The composition's answers for both modes at cap 512 / 512, computed once and left unchanged."""
    groups, rhss, _ = batch
    return {flag: hc.want(port, groups, rhss, flag, cap_rows=CAP, cap_out_rows=CAP) for flag in (False, True)}


@pytest.fixture(scope="module")
def pools(port):
    return hc.pools(port)


def _g(names, name):
    return names.index(name)


def test_the_batch_is_the_one_the_cases_rest_on(port, batch, wants, pools):
    """No device: the groups, the checker's answers and the plan view."""
    groups, rhss, names = batch
    assert len(groups) == hc.NG == 40 and {len(g) for g in groups} == {0, 1, 2, 3, 5, 17}
    assert len({g[0].shape[1] for g in groups if g}) == 5 and any(g and r == g[0].shape[1] - 2 for g, r in zip(groups, rhss))
    assert {m.shape[0] for m in groups[_g(names, "mixed rows")]} == {6, 9}            # rows inside a group may differ
    for flag in (False, True):
        w = wants[flag]
        assert all(x[1] == -1 and x[0] in (0, 1) for x in w)                         # every member's calcBound succeeds
        assert [g for g, x in enumerate(w) if x[5] == 0] == [g for g, m in enumerate(groups) if not m]   # the empty groups gather nothing
        assert all(x[0] == 1 and x[4].shape[0] == 0 for g, x in enumerate(w) if not groups[g])
        # the issue's table
        assert (w[_g(names, "overlap")][5], w[_g(names, "overlap")][4].shape[0]) == (9, 4)
        assert w[_g(names, "aba")][5] == 13 and rows_equal(w[_g(names, "aba")][4], w[_g(names, "overlap")][4])
        assert w[_g(names, "disjoint")][5] == 9
        sym = w[_g(names, "symbols")]
        assert sym[0] == 1 and any(not row[:2, 0].any() and row[3, 0] != 0 for row in sym[4])   # a row of symbols only survives
        assert w[_g(names, "rhs cols-2")][0] == 1 and w[_g(names, "repeat")][0] == 1
    assert wants[False][_g(names, "disjoint")][:1] == (1,) and wants[False][_g(names, "disjoint")][4].shape[0] == 4
    dis = wants[True][_g(names, "disjoint")]
    assert dis[0] == 0 and dis[4].shape == (0, 3, 2)
    # ... which reduce leaves with 7 rows before the hull cleans them
    res = np.concatenate([hc.rat([[0, 0, 0]])] + [t for m in groups[_g(names, "disjoint")] for t in bc.chains(port, m, 2)[3] if t.shape[0]])
    ok, left = port.reduce(res, 2, True)
    assert (ok, res.shape[0], left.shape[0]) == (0, 9, 7)
    # both outcomes of reduce occur in both modes, and a union that reduce finds inconsistent keeps its rows
    assert {x[0] for x in wants[False]} == {0, 1} == {x[0] for x in wants[True]}
    assert any(x[0] == 0 and x[4].shape[0] > 0 for x in wants[False]) and all(x[4].shape[0] == 0 for x in wants[True] if x[0] == 0)
    assert max(x[5] for x in wants[False]) == 91
    # the plan: at the default capacities every group with members is at home in LDS
    sizes, rows, cols, rhs = hc.shapes_of(groups, rhss)
    p, homes, gcaps = hc.plan_view(sizes, rows, cols, rhs, None, CAP)
    assert (p, homes, gcaps) == hc.plan(sizes, rows, cols, rhs, None, CAP)
    assert p["cap_hull"] == 1 + 2 * 4 * 17 and p["groups_device"] == 0 and p["groups_lds"] == 35 and homes.count(hc.HOME_NONE) == 5
    good, bad = pools
    assert all(len(x) >= 17 for x in good) and len(bad[5]) >= 2


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_intersect", [False, True])
def test_every_group_equals_the_composition(lq, batch, wants, is_intersect):
    groups, rhss, _ = batch
    got = lq.hull_ragged(groups, rhss, is_intersect, cap_rows=CAP)
    route = lq.hull_ragged_last_route()
    hc.same(got, wants[is_intersect])
    assert route["producer_launches"] == 1 and route["launches"] == 1 and route["grid"] == 40
    assert route["gathered_rows"] == sum(x[5] for x in wants[is_intersect])


def test_every_group_equals_the_real_reference(lq, ref, batch):
    groups, rhss, _ = batch
    for flag in (False, True):
        hc.same(lq.hull_ragged(groups, rhss, flag, cap_rows=CAP), hc.want(ref, groups, rhss, flag, cap_rows=CAP, cap_out_rows=CAP))


# ---- 2. a failing member -------------------------------------------------------------------------------------------------------
def test_a_failing_member_answers_for_its_group_alone(lq, port, batch, wants, pools):
    groups, rhss, _ = batch
    good, bad = pools
    ok5, (b1, b2) = good[5][:4], bad[5][:2]
    v1, v2 = bc.chains(port, b1, 4, CAP, CAP)[:3], bc.chains(port, b2, 4, CAP, CAP)[:3]
    assert v1[0] == 0 and v2[0] == 0
    extra = [[b1] + ok5, ok5[:2] + [b1] + ok5[2:], ok5 + [b1], ok5[:1] + [b2] + ok5[1:3] + [b1] + ok5[3:], [b2]]
    where = [(0, v1), (2, v1), (4, v1), (1, v2), (0, v2)]
    at = 7
    mixed = groups[:at] + extra + groups[at:]
    mrhs = rhss[:at] + [4] * len(extra) + rhss[at:]
    for flag in (False, True):
        w = hc.want(port, extra, [4] * len(extra), flag, cap_rows=CAP, cap_out_rows=CAP)
        assert [(x[1], (x[0], x[2], x[3])) for x in w] == where                      # the checker's facts first
        got = lq.hull_ragged(mixed, mrhs, flag, cap_rows=CAP)
        hc.same(got, wants[flag][:at] + w + wants[flag][at:], "failing")
        for k, (m, v) in enumerate(where):
            g = at + k
            assert (got[1][g], got[0][g], got[2][g], got[3][g]) == (m,) + v and got[4][g].shape == (0, 5, 2)


# ---- 3. the device composition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_intersect", [False, True])
def test_bitwise_equal_to_bounds_ragged_then_reduce_ragged(lq, batch, is_intersect):
    """The two existing calls composed on the host give the same reduce the same rows."""
    groups, rhss, _ = batch
    members = [m for g in groups for m in g]
    mrhs = [r for g, r in zip(groups, rhss) for _ in g]
    bok, _, _, bounds = lq.bounds_ragged(members, rhs_idx=mrhs, cap_rows=CAP)
    assert (bok == 1).all()
    full = [g for g in range(len(groups)) if groups[g]]
    cat, b = [], 0
    for g in range(len(groups)):
        if groups[g]:
            lead = hc.rat([[0] * groups[g][0].shape[1]])
            cat.append(np.concatenate([lead] + [t for i in range(len(groups[g])) for t in bounds[b + i] if t.shape[0]]))
        b += len(groups[g])
    rok, rrows = lq.reduce_ragged(cat, rhs_idx=[rhss[g] for g in full], is_intersect=is_intersect)
    ok, member, _, _, rows = lq.hull_ragged(groups, rhss, is_intersect, cap_rows=CAP)
    assert (member == -1).all()
    for k, g in enumerate(full):
        assert ok[g] == rok[k], g
        keep = rrows[k] if rok[k] or not is_intersect else rrows[k][:0]
        assert rows[g].shape == keep.shape and np.array_equal(rows[g], keep), g


# ---- 4. both homes ---------------------------------------------------------------------------------------------------------------
def test_both_homes_in_one_launch(lq, port, batch, pools):
    groups, rhss, names = batch
    good, _ = pools
    caps = dict(cap_rows=CAP, cap_out_rows=16, cap_hull_rows=1000)
    sizes, rows, cols, rhs = hc.shapes_of(groups, rhss)
    p, homes, gcaps = hc.plan_view(sizes, rows, cols, rhs, None, CAP, 16, 1000)
    assert (p, homes, gcaps) == hc.plan(sizes, rows, cols, rhs, None, CAP, 16, 1000)
    dev = [g for g, h in enumerate(homes) if h == hc.HOME_DEVICE]
    assert [names[g] for g in dev] == ["c3 x17", "c5 x17", "c3 x17"] and p["lds_rows"] == 682 and p["cols"] == 6
    assert all(gcaps[g] == 1000 and 1000 * 5 > 682 * 6 for g in dev) and homes.count(hc.HOME_LDS) == 32
    assert p["slot_bytes"] == 40 * 1000 * 6 * 8
    w = hc.want(port, groups, rhss, False, cap_hull=1000, **{k: caps[k] for k in ("cap_rows", "cap_out_rows")})
    assert all(x[0] >= 0 for x in w)
    got = lq.hull_ragged(groups, rhss, False, **caps)
    route = lq.hull_ragged_last_route()
    assert (route["groups_lds"], route["groups_device"], route["slot_bytes"]) == (32, 3, p["slot_bytes"])
    hc.same(got, w, "both homes")
    # a group whose gathered ROWS exceed the LDS rows, at the default cap_hull_rows: the member count from the plan rule -- the
    # first whose rows, as the checker counts them, need more cells than the LDS matrix area has
    per = [sum(t.shape[0] for t in bc.chains(port, m, 4, CAP, 16)[3]) for m in good[5]]
    n, gathered = 0, 1
    while gathered * 5 <= 682 * 6:
        gathered += per[n % len(per)]; n += 1
    big = [good[5][k % len(good[5])] for k in range(n)]
    small = [groups[_g(names, "overlap")], groups[_g(names, "c1 x3")]]
    trio, trhs = [small[0], big, small[1]], [2, 4, 2]
    sizes, rows, cols, rhs = hc.shapes_of(trio, trhs)
    p, homes, gcaps = hc.plan_view(sizes, rows, cols, rhs, None, CAP, 16, 0)
    assert homes == [hc.HOME_LDS, hc.HOME_DEVICE, hc.HOME_LDS] and p["cap_hull"] == 1 + 8 * n and p["lds_rows"] == 32 * 1024 // (5 * 8)
    w = hc.want(port, trio, trhs, True, cap_rows=CAP, cap_out_rows=16, cap_hull=p["cap_hull"])
    assert w[1][5] == gathered and gathered * 5 > p["lds_rows"] * 5 and w[1][1] == -1
    for flag in (True, False):
        hc.same(lq.hull_ragged(trio, trhs, flag, cap_rows=CAP, cap_out_rows=16),
                w if flag else hc.want(port, trio, trhs, False, cap_rows=CAP, cap_out_rows=16, cap_hull=p["cap_hull"]), "big")
        assert lq.hull_ragged_last_route()["gathered_rows"] == sum(x[5] for x in w)


# ---- 5. capacity -------------------------------------------------------------------------------------------------------------------
def test_capacity_of_the_hull_and_of_a_member(lq, port, batch, wants):
    groups, rhss, names = batch
    w = wants[False]
    over = [g for g, x in enumerate(w) if x[5] > 90]
    assert len(over) == 1 and w[over[0]][5] == 91 and names[over[0]] == "c5 x17"
    got = lq.hull_ragged(groups, rhss, False, cap_rows=CAP, cap_hull_rows=90)
    short = hc.want(port, groups, rhss, False, cap_rows=CAP, cap_out_rows=CAP, cap_hull=90)
    assert [x[:4] for g, x in enumerate(short) if x[0] < 0] == [(-91, -1, -1, 0)]
    hc.same(got, short, "cap_hull 90")
    assert got[0][over[0]] == -91 and got[1][over[0]] == -1 and got[4][over[0]].shape[0] == 0
    assert lq.hull_ragged_last_route()["gathered_rows"] == sum(x[5] for x in w) - 91
    need = int(-got[0].min())
    hc.same(lq.hull_ragged(groups, rhss, False, cap_rows=CAP, cap_hull_rows=need), w, "retry")
    # a member's -need from cap_rows is passed through with its member index
    tight = hc.want(port, groups, rhss, False, cap_rows=64, cap_out_rows=64)
    hit = [(g, x) for g, x in enumerate(tight) if x[0] < 0]
    assert hit and all(x[1] >= 0 and -x[0] > 64 for _, x in hit) and any(x[1] > 0 for _, x in hit)
    got = lq.hull_ragged(groups, rhss, False, cap_rows=64)
    hc.same(got, tight, "cap_rows 64")
    for g, x in hit:
        assert (got[0][g], got[1][g], got[2][g], got[3][g]) == x[:4] and got[4][g].shape[0] == 0


# ---- 6. more groups than the grid ------------------------------------------------------------------------------------------------
def test_workgroups_are_reused_above_the_grid(lq, port, batch):
    groups, rhss, names = batch
    reps = 103
    ng = 40 * reps
    src = [g % 40 for g in range(ng)]
    assert ng > 4096
    second = [(src[j], src[4096 + j]) for j in range(ng - 4096)]                     # workgroup j takes group j, then group 4096 + j
    width = lambda g: groups[g][0].shape[1] if groups[g] else 0
    assert sum(width(a) != width(b) and width(a) and width(b) for a, b in second) >= 10
    caps = dict(cap_rows=CAP, cap_out_rows=16, cap_hull_rows=1000)
    sizes, rows, cols, rhs = hc.shapes_of(groups, rhss)
    homes = hc.plan_view(sizes, rows, cols, rhs, None, CAP, 16, 1000)[1]
    assert any(homes[a] != homes[b] and hc.HOME_NONE not in (homes[a], homes[b]) for a, b in second)   # a seat changes its home, too
    w = hc.want(port, groups, rhss, True, cap_rows=CAP, cap_out_rows=16, cap_hull=1000)
    got = lq.hull_ragged([groups[g] for g in src], [rhss[g] for g in src], True, copy=False, **caps)
    route = lq.hull_ragged_last_route()
    assert route["grid"] == 4096 and route["slot_bytes"] == 4096 * 1000 * 6 * 8 and route["groups_device"] == 3 * reps
    hc.same(got, [w[g] for g in src], "tiled")


# ---- 7. order ----------------------------------------------------------------------------------------------------------------------
def test_order_of_groups_and_of_members(lq, port, batch, wants):
    groups, rhss, names = batch
    perm = np.random.default_rng(11).permutation(40).tolist()
    for order in (perm, list(range(39, -1, -1))):
        got = lq.hull_ragged([groups[g] for g in order], [rhss[g] for g in order], False, cap_rows=CAP)
        hc.same(got, [wants[False][g] for g in order], str(order[:3]))
    # the gather order is part of the contract: a reversed list gives the composition's answer for the reversed list
    rev = [list(reversed(g)) for g in groups]
    for flag in (False, True):
        w = hc.want(port, rev, rhss, flag, cap_rows=CAP, cap_out_rows=CAP)
        assert any(not rows_equal(a[4], b[4]) for a, b in zip(w, wants[flag]))       # ... and it differs somewhere
        hc.same(lq.hull_ragged(rev, rhss, flag, cap_rows=CAP), w, "reversed")


# ---- 8. no groups, the sizing call, the caller's buffer, views ---------------------------------------------------------------------
def _c_call(ctx, groups, rhss, flag=0, cap=0, cap_out=0, cap_hull=0, outs=None, outs_cap=0, goff=None, ng=None, cols=None, rhs=None):
    from xpoly_amd._capi import lib, vp
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    members = [m for g in groups for m in g]
    n = len(groups)
    flat = np.ascontiguousarray(np.concatenate([m.reshape(-1, 2) for m in members]))
    rows = i32([m.shape[0] for m in members]); mcols = i32([m.shape[1] for m in members])
    off = np.zeros(len(members) + 1, dtype=np.int64); off[1:] = np.cumsum(rows.astype(np.int64) * mcols)
    g_off = i32(np.concatenate([[0], np.cumsum([len(g) for g in groups])]) if goff is None else goff)
    mrhs = i32([r for g, r in zip(groups, rhss) for _ in g] if rhs is None else rhs)
    ooff = np.full(n + 1, -5, dtype=np.int64); orows = np.full(n, -7, dtype=np.int32)
    v = [np.full(n, 7, dtype=np.int32) for _ in range(4)]
    code = lib().xpg_lineq_hull_batch_ragged_rat32(
        ctx._h, C.c_int(n if ng is None else ng), vp(g_off), C.c_int(len(members)), vp(flat), vp(rows), vp(mcols if cols is None else i32(cols)), vp(off),
        vp(mrhs), C.c_int(flag), C.c_int(cap), C.c_int(cap_out), C.c_int(cap_hull), vp(outs), C.c_longlong(outs_cap), None, vp(ooff), vp(orows),
        vp(v[0]), vp(v[1]), vp(v[2]), vp(v[3]))
    return code, ooff, orows, v


def test_no_groups_sizing_a_short_buffer_and_views(ctx, lq, batch, wants):
    groups, rhss, _ = batch
    e = lq.hull_ragged([])
    assert all(len(x) == 0 for x in e)
    code, ooff, _, _ = _c_call(ctx, groups[:2], rhss[:2], ng=0, goff=[0])
    assert code == XPG_ERR_SHAPE                                                      # no groups, but members
    only_empty = lq.hull_ragged([[], []])
    assert list(only_empty[0]) == [1, 1] and list(only_empty[1]) == [-1, -1] and lq.hull_ragged_last_route()["launches"] == 0
    a = lq.hull_ragged(groups, rhss, False, cap_rows=CAP)
    v = lq.hull_ragged(groups, rhss, False, cap_rows=CAP, copy=False)
    hc.same(v, wants[False], "views")
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], v[:4])) and all(rows_equal(x, y) for x, y in zip(a[4], v[4]))
    for cap_out in (16, 0):                                                          # slots that come down whole, and slots packed on the device
        code, ooff, orows, ver = _c_call(ctx, groups, rhss, 0, CAP, cap_out)
        assert lq.hull_ragged_last_route()["out_bytes"] <= (512 << 10) if cap_out else lq.hull_ragged_last_route()["out_bytes"] > (512 << 10)
        assert code == 0 and ooff[0] == 0 and (orows >= 0).all() and np.array_equal(ver[0], a[0])
        total = int(ooff[-1])
        assert total == sum(x.shape[0] * x.shape[1] for x in a[4])
        out = np.zeros((total, 2), dtype=np.int32)
        code, ooff2, orows2, ver2 = _c_call(ctx, groups, rhss, 0, CAP, cap_out, outs=out, outs_cap=total - 1)
        assert code == XPG_ERR_SHAPE and lq.hull_ragged_last_route()["launches"] == 1
        assert np.array_equal(ooff2, ooff) and np.array_equal(orows2, orows) and all(np.array_equal(x, y) for x, y in zip(ver, ver2))
        code, ooff3, _, _ = _c_call(ctx, groups, rhss, 0, CAP, cap_out, outs=out, outs_cap=total)
        assert code == 0 and np.array_equal(ooff3, ooff)
        for g in range(40):
            if groups[g]:
                assert rows_equal(out[ooff[g]: ooff[g + 1]].reshape(-1, groups[g][0].shape[1], 2), a[4][g]) and orows[g] == a[4][g].shape[0], g


# ---- 9. errors launch nothing --------------------------------------------------------------------------------------------------------
def test_errors_launch_nothing(ctx, lq, batch, pools):
    groups, rhss, _ = batch
    good, _ = pools
    few, frhs = [good[3][:2], good[5][:3]], [4, 4]                                   # 6 x 5 and 9 x 5: rows differ inside nothing, cols agree

    def call(g=few, r=frhs, **kw):
        code = _c_call(ctx, g, r, **kw)[0]
        assert lq.hull_ragged_last_route()["launches"] == (1 if code == 0 else 0), (kw, code)
        return code

    assert call(cap=CAP) == 0
    assert call([good[3][:1] + good[2][:1], good[5][:3]], [4, 4], rhs=[4, 3, 4, 4, 4]) == XPG_ERR_SHAPE   # mixed cols in a group
    assert call(rhs=[4, 3, 4, 4, 4]) == XPG_ERR_SHAPE                                # mixed rhs_idx in a group
    assert call(rhs=[4, 4, 3, 3, 3], cap=CAP) == 0                                   # groups may differ
    assert call(goff=[0, 3, 2]) == XPG_ERR_SHAPE and call(goff=[1, 2, 5]) == XPG_ERR_SHAPE and call(goff=[0, 2, 4]) == XPG_ERR_SHAPE
    assert call(cap_hull=32768) == XPG_ERR_UNSUPPORTED
    assert call(cap_hull=20000) == XPG_ERR_UNSUPPORTED                               # the scratch of 20000 rows over 160 KB
    assert call(cap=32768) == XPG_ERR_UNSUPPORTED and call(ng=-1) == XPG_ERR_SHAPE


# ---- 10. the projected union ---------------------------------------------------------------------------------------------------------
def test_project_union_is_the_chain_then_one_reduce(lq, port, pools):
    good, bad = pools
    down = lambda nv: list(range(nv - 1, 0, -1))                                     # onto variable 0
    classes = [1, 2, 3, 5]                                                           # nv 2, 3, 4, 4
    groups = [good[c][:n] for c, n in zip(classes, (3, 2, 4, 17))] + [[], good[3][4:7]]
    nvs = [hc.CLASSES[c][1] for c in classes] + [1, 4]
    fails = [m for m in bad[5] if pc.stepped(port, m, 4, down(4), False, CAP, CAP)[0] == 0]
    assert fails
    groups.append(good[5][:2] + fails[:1] + good[5][2:3]); nvs.append(4)
    elims = [[down(nv) for _ in g] for g, nv in zip(groups, nvs)]
    caps = dict(cap_rows=CAP, cap_out_rows=128, cap_hull_rows=1000)
    sizes, rows, cols, rhs = hc.shapes_of(groups, nvs)
    flat = [e for g in elims for e in g]
    p, homes, gcaps = hc.plan_view(sizes, rows, cols, rhs, flat, CAP, 128, 1000)
    assert (p, homes, gcaps) == hc.plan(sizes, rows, cols, rhs, flat, CAP, 128, 1000)
    assert homes == [0, 0, 0, 1, -1, 0, 0] and gcaps[3] == 1000 and 1000 * 5 > p["lds_rows"] * p["cols"]
    for flag in (False, True):
        w = [hc.project_union(port, g, nv, e, flag, False, CAP, 128, 1000) for g, nv, e in zip(groups, nvs, elims)]
        assert w[6][1] == 2 and w[6][0] == 0 and w[6][2] == -1 and all(x[1] == -1 for x in w[:6]) and any(x[4].shape[0] for x in w)
        got = lq.project_union_ragged(groups, nvs, elims, flag, **caps)
        route = lq.hull_ragged_last_route()
        hc.same(got, w, "union %s" % flag)
        assert (route["producer_launches"], route["launches"], route["groups_device"]) == (1, 1, 1)
        assert route["gathered_rows"] == sum(x[5] for x in w)


# ---- 11. the C++ layer -----------------------------------------------------------------------------------------------------------------
def test_the_member_function_and_the_collectors(port, batch, tmp_path):
    """tests/cxx/hull_all.cpp in a child process: Lineq::ConvexHullUnionAndIntersect through a minimal list type and through its
    vector overload, hull_all and project_union_each, compared in there, group for group and bit for bit, with calc_bound_each /
    project_each on all members, a host concatenation and Lineq::reduce. The groups are this file's; at the collector's first
    capacities (the library's defaults) the checker finds a member short of rows, so the answer comes from a retry."""
    import subprocess
    from test_lineq_hull_host import build_collector
    exe = build_collector()
    groups, rhss, names = batch
    first = hc.want(port, groups, rhss, False, cap_rows=4 * 9 + 16, cap_out_rows=4 * 9 + 16)
    assert any(x[0] < 0 and x[1] >= 0 for x in first)                                # one retry at least
    lines = ["%d" % len(groups)]
    for g, r in zip(groups, rhss):
        lines.append("%d %d" % (len(g), r))
        for m in g:
            lines += ["%d %d" % m.shape[:2], " ".join(str(int(x)) for x in np.asarray(m).ravel())]
    path = str(tmp_path / "groups.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert out[0] == "rc 0 0 0" and out[1] == "route 1 1 %d" % len(groups) and "mismatches 0" in out
    per = [ln.split() for ln in out if " ok " in ln]
    assert len(per) == len(groups) and all(p[-1] == "1" for p in per)
    w = hc.want(port, groups, rhss, False, cap_rows=CAP, cap_out_rows=CAP), hc.want(port, groups, rhss, True, cap_rows=CAP, cap_out_rows=CAP)
    assert [(int(p[2]), int(p[3]), int(p[5]), int(p[6])) for p in per] == [(a[0], b[0], a[4].shape[0], b[4].shape[0]) for a, b in zip(*w)]
