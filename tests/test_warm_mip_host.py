"""CPU suite: the host side of the warm-started branch and bound's tests. The launch geometry of xpg_mip_warm_batch_f64
(host-only view xpg_test_warm_batch_geometry, computed by the function the launch calls) against a restatement here; and the
two exact references of tests/warm_mip_ref.py against each other on every case family of tests/warm_mip_cases.py, with the
condition under which a case is kept: exact_bb's deepest path is at most half of the depth_cap its launch gets."""
import ctypes as C
import os

import pytest

import warm_mip_cases as wc
import warm_mip_ref as ref

LDS_MAX = 64 * 1024
XPG_ERR_SHAPE = -3


def plan(rows, cols, is_bin, nb, ws_cap=4 << 30):
    """warm_mip_batch.hip.h, restated: the LDS carve, the depth that shrinks by two down to 4, the workspace strides, chunks."""
    n0, m0 = cols - 1, rows
    depth = n0 + 2 if is_bin else 2 * n0 + 8

    def lds_of(depth):
        mcap = m0 + depth
        wcap = n0 + mcap + 1
        doubles = mcap * wcap + 2 * wcap + mcap + n0 + 8     # T, obj, prow, pcol, c0, red_v
        ints = wcap + mcap + 8                               # bv_row, eq2bv, red_i
        return (doubles * 8 + ints * 4 + 15) // 16 * 16, mcap, wcap
    while lds_of(depth)[0] > LDS_MAX and depth > 4:
        depth -= 2
    lds, mcap, wcap = lds_of(depth)
    snap = mcap * wcap + wcap + 8 + (wcap + mcap + 1) // 2 + 1
    tree = (2 + n0 + depth * snap + 15) // 16 * 16
    chunk = nb
    while chunk * tree * 8 > ws_cap and chunk > 64:
        chunk = (chunk + 1) // 2
    return dict(lds=lds, refused=int(lds > LDS_MAX), depth_cap=depth, mcap=mcap, wcap=wcap, snap_stride=snap, tree_stride=tree,
                chunk=chunk, launches=-(-nb // chunk))


def test_the_geometry_view_equals_its_restatement():
    edge, tall = wc.lds_edge_n0(), wc.refusal_rows()
    shapes = [(r, n0 + 1, is_bin) for r in (1, 2, 5, 26) for n0 in (1, 2, 6, 24, 63, 64, 65, 255, 256, 257, 300) for is_bin in (0, 1)]
    shapes += [(edge + 2, edge + 1, 1), (edge + 3, edge + 2, 1), (edge + 3, edge + 1, 1), (tall, 3, 0), (tall + 1, 3, 0), (tall, 3, 1),
               (2, wc.wide_n0() + 1, 0), (2, wc.wide_n0() + 2, 0), (120, 40, 0), (40, 120, 1)]
    seen = set()
    for rows, cols, is_bin in shapes:
        for nb in (1, 65, 200, 4000, 100001):
            got, want = wc.geometry(rows, cols, is_bin, nb), plan(rows, cols, is_bin, nb)
            assert got == want, (rows, cols, is_bin, nb, got, want)
            full = cols + 1 if is_bin else 2 * cols + 6
            seen.add(("refused", got["refused"]))
            seen.add(("shrunk", got["depth_cap"] < full))
            seen.add(("floor", got["depth_cap"] == 4 and got["depth_cap"] < full and not got["refused"]))
            seen.add(("chunked", got["launches"] > 1))
            seen.add(("short last chunk", got["launches"] > 1 and nb % got["chunk"] != 0))
    for k in ("refused", "shrunk", "floor", "chunked", "short last chunk"):
        assert (k, True) in seen and (k, False) in seen, (k, seen)


def test_the_workspace_bound_of_the_hooks_build_moves_the_chunks():
    """XPG_WARM_BATCH_WS_CAP (hooks build only, host side): the view shows the chunks the launch loop will take, down to the
    floor of 64 trees that the 4 GB bound cannot reach; the product library ignores the switch."""
    import json
    import subprocess
    import sys
    from conftest import HOOKS_SO, ROOT, hooks_env
    assert os.path.exists(HOOKS_SO), "%s is missing: python -m xpoly_amd.build" % HOOKS_SO
    per_tree = plan(4, 3, 0, 1)["tree_stride"] * 8
    code = ("import json, sys; sys.path.insert(0, 'tests')\n"
            "import warm_mip_cases as wc\n"
            "print('G', json.dumps([wc.geometry(4, 3, 0, nb) for nb in (1, 64, 65, 200, 201, 1000)]))\n")
    for cap in (per_tree * 70, per_tree * 10, per_tree * 150):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=hooks_env(XPG_WARM_BATCH_WS_CAP=str(cap)), cwd=ROOT, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        got = json.loads([l for l in r.stdout.splitlines() if l.startswith("G ")][0][2:])
        assert got == [plan(4, 3, 0, nb, cap) for nb in (1, 64, 65, 200, 201, 1000)], (cap, got)
    assert [plan(4, 3, 0, nb, per_tree * 70)["chunk"] for nb in (64, 65, 200, 201, 1000)] == [64, 65, 50, 51, 63]
    assert plan(4, 3, 0, 201, per_tree * 10)["chunk"] == 51 and plan(4, 3, 0, 201, per_tree * 10)["launches"] == 4     # the floor
    os.environ["XPG_WARM_BATCH_WS_CAP"] = str(per_tree * 70)
    try:
        assert wc.geometry(4, 3, 0, 200)["chunk"] == 200                                                               # the product build
    finally:
        del os.environ["XPG_WARM_BATCH_WS_CAP"]


def test_both_sides_of_the_64_kb_boundary():
    edge = wc.lds_edge_n0()
    g = wc.geometry(edge + 2, edge + 1, 1)
    assert g["depth_cap"] == edge + 2 and g["refused"] == 0 and LDS_MAX - 1024 < g["lds"] <= LDS_MAX, g
    assert wc.geometry(edge + 3, edge + 1, 1)["depth_cap"] < edge + 2              # one more row: the depth gives way
    assert wc.geometry(edge + 3, edge + 2, 1)["depth_cap"] < edge + 3              # one more variable too
    tall = wc.refusal_rows()
    g = wc.geometry(tall, 3, 0)
    assert g["depth_cap"] == 4 and g["refused"] == 0 and g["lds"] <= LDS_MAX, g     # the shrinking loop ends at 4 ...
    g = wc.geometry(tall + 1, 3, 0)
    assert g["depth_cap"] == 4 and g["refused"] == 1 and g["lds"] > LDS_MAX, g      # ... and the refusal lies behind it
    n0 = wc.wide_n0()
    g = wc.geometry(2, n0 + 1, 0)
    assert g["depth_cap"] >= 12 and g["wcap"] > 256 and n0 > 257 and wc.geometry(2, n0 + 2, 0)["depth_cap"] < 12, g


def test_the_geometry_view_refuses_bad_arguments():
    from xpoly_amd import _capi
    out = (C.c_longlong * 9)()
    call = lambda rows, cols, nb, o=out, n=9: _capi.lib().xpg_test_warm_batch_geometry(C.c_int(rows), C.c_int(cols), C.c_int(0), C.c_int(nb), o, C.c_int(n))
    assert call(0, 3, 1) == XPG_ERR_SHAPE and call(2, 1, 1) == XPG_ERR_SHAPE and call(2, 3, 0) == XPG_ERR_SHAPE
    assert call(2, 3, 1, None) == XPG_ERR_SHAPE and call(2, 3, 1, out, -1) == XPG_ERR_SHAPE
    out[2] = 77
    assert call(2, 3, 1, out, 2) == 0 and out[2] == 77                               # fills min(n, 9) entries


def all_cases():
    """Every case the GPU tests run, with the senses it runs in."""
    both = (True, False)
    cases = []
    for shape in wc.MIXED_SHAPES:
        cases += [(k, both) for k in wc.memo(wc.mixed, *shape, 8)]
    cases += [(k, both) for k in wc.memo(wc.mixed, *wc.CYCLE_SHAPE, 64)]
    cases += [(k, both) for k in wc.memo(wc.mixed, 2, 2, 0, 8, 4)]
    cases += [(k, both) for k in wc.integral_root(5, 4, 8) + wc.integral_root(2, 4, 2)]
    cases += [(k, both) for k in wc.unbounded(3, 3) + wc.unbounded(2, 4) + wc.root_infeasible(3, 4) + wc.root_infeasible(2, 4)]
    cases += [(wc.deep(wc.DEEP_SMALL_U), both), (wc.TRIVIAL, both), (wc.tall(wc.refusal_rows()), both)]
    cases += [(k, (True,)) for k in wc.memo(wc.wide, wc.wide_n0())]
    cases += [(k, (True,)) for k in wc.memo(wc.lds_edge, wc.lds_edge_n0())]
    return cases


def test_brute_and_exact_bb_agree_on_every_enumerable_case():
    enumerated, statuses = 0, set()
    for k, senses in all_cases():
        for is_max in senses:
            bb, br = wc.solved(k, is_max)
            w = wc.want(k, is_max)
            if br is None:
                assert w.by == "exact_bb"
                continue
            assert (br.status, br.optimum) == (bb.status, bb.optimum) == (w.status, w.optimum), (k.name, is_max, br[:2], bb)
            if br.status == ref.SUCC:
                assert tuple(bb.point) in br.points, (k.name, is_max)
            enumerated += 1
            statuses.add(br.status)
    assert enumerated >= 200 and statuses == {ref.SUCC, ref.NO_SOL}, (enumerated, statuses)


def test_no_retained_case_walks_deeper_than_half_its_depth_cap():
    deepest = 0
    for k, senses in all_cases():
        cap = wc.depth_cap(k)
        for is_max in senses:
            w = wc.want(k, is_max)
            assert 2 * w.deepest <= cap, (k.name, is_max, w.deepest, cap)
            deepest = max(deepest, w.deepest)
    assert deepest >= 5                                                      # and the families do branch
    cap = wc.depth_cap(wc.deep(wc.DEEP_LARGE_U))
    assert cap == 12
    for is_max in (True, False):
        small, large = wc.want(wc.deep(wc.DEEP_SMALL_U), is_max), wc.want(wc.deep(wc.DEEP_LARGE_U), is_max)
        assert small.status == large.status == ref.NO_SOL and small.root == large.root == "optimal"
        assert 2 * small.deepest <= cap and large.deepest > 2 * cap, (small, large)


def test_the_families_are_what_they_say():
    for k in wc.unbounded(3, 3) + wc.unbounded(2, 4):
        assert k.c[0] > 0 and all(row[0] <= 0 for row in k.A)
        w = wc.want(k, True)
        assert (w.status, w.root, w.by) == (ref.UNBOUND, "unbounded", "exact_bb"), k.name
    assert any(bi < 0 for bi in wc.unbounded(3, 3)[1].b)                     # the variant whose root needs phase one
    for k in (wc.root_infeasible(3, 4)[0], wc.root_infeasible(2, 4)[0]):
        assert all(wc.want(k, s).root == "infeasible" and wc.want(k, s).status == ref.NO_SOL for s in (True, False))
    for k in (wc.root_infeasible(3, 4)[1], wc.root_infeasible(2, 4)[1]):
        assert all(wc.want(k, s).root == "optimal" and wc.want(k, s).status == ref.NO_SOL for s in (True, False))
    for k in wc.integral_root(5, 4, 8) + wc.integral_root(2, 4, 2):
        for is_max in (True, False):
            bb = ref.exact_bb(k.c, k.A, k.b, is_max)
            assert bb.status == ref.SUCC and bb.nodes == 1 and bb.deepest == 0, (k.name, bb)
    mixed = [k for k, _ in all_cases() if k.family == "mixed"]
    flat = lambda k: [a for row in k.A for a in row]
    assert all(max(abs(a) for a in flat(k)) <= 5 and max(abs(v) for v in k.c) <= 6 for k in mixed)
    assert any(a < 0 for k in mixed for a in flat(k)) and any(v < 0 for k in mixed for v in k.c) and any(v == 0 for k in mixed for v in k.c)
    assert any(bi == 0 for k in mixed for bi in k.b) and any(bi < 0 for k in mixed for bi in k.b)
    assert any(bi.denominator == 2 for k in mixed for bi in k.b if not isinstance(bi, int))
    assert any(len(set(map(tuple, k.A))) < len(k.A) for k in mixed) and any(len(set(zip(*k.A))) < len(k.c) for k in mixed)
    many = [len(ref.brute(k.c, k.A, k.b, k.is_bin, True).points) for k in wc.memo(wc.mixed, *wc.CYCLE_SHAPE, 64)]
    assert max(many) >= 4                                                     # many equal optima


def test_wide_is_brute_over_its_active_variables():
    """On a miniature of 12 variables, where exact_bb over all twelve is cheap, and on the cases the GPU runs."""
    active = [0, 3, 4, 7, 8, 11]
    for k in wc.wide(12, range(12), active):
        bb, br = ref.exact_bb(k.c, k.A, k.b, True), wc.wide_want(k, active)
        assert (bb.status, bb.optimum) == (br.status, br.optimum) == (ref.SUCC, br.optimum), (k.name, bb, br[:2])
    n0 = wc.wide_n0()
    assert wc.wide_active(n0) == [0, 63, 64, 255, 256, n0 - 1]
    for k in wc.memo(wc.wide, n0):
        others = [j for j in range(n0) if j not in wc.wide_active(n0)]
        assert all(k.c[j] > 0 for j in wc.wide_active(n0)) and all(k.c[j] <= 0 and k.A[0][j] >= 0 and k.A[1][j] >= 0 for j in others)
        br, w = wc.wide_want(k, wc.wide_active(n0)), wc.want(k, True)
        assert (w.status, w.optimum) == (br.status, br.optimum), (k.name, w, br[:2])
