"""CPU suite: the launch rules of the two HBM-resident Rational loops (lp_host.hip.h r32_loop_plan, through the host-only
xpg_test_r32_loop_plan) against their Python mirror, and the case table of tests/r32_loop_cases.py: which geometries it
reaches, and -- from the checker's answers alone -- that its LPs do what the GPU tests of test_gpu_r32_loop_geometry.py rest
on: pivots that leave on second-round rows and on the lower row of identical pairs, phase one, end states inside the budget,
the `weird` hand-off of the n/0 variants, no float32 rescue in the set replayed in fractions.Fraction. No device needed."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import r32_loop_cases as RC                              # noqa: E402


@pytest.fixture(scope="module")
def facts(port):
    return {c["name"]: RC.facts(port, c) for c in RC.CASES}


def test_plan_mirror_equals_the_library():
    edges = {1, 2, 3, 4200}
    for k in range(64, 4200, 64):                        # every multiple of 64 (so of 256) and both neighbours
        edges.update((k - 1, k, k + 1))
    widths = set(range(200, 601, 50)) | {255, 256, 257, 511, 512, 513, 599, 600, 603}
    n = 0
    for forced in (RC.NONE, RC.FUSED, RC.PIPE):
        for m in sorted(edges):
            ws = set(widths)
            for cells in (RC.FUSED_FROM, RC.FUSED_UPTO):  # both size thresholds, from either side, at this height
                ws.update(w for w in (cells // m - 1, cells // m, cells // m + 1, cells // m + 2) if w > 0)
            for W in sorted(ws):
                assert RC.lib_plan(m, W, forced) == RC.plan(m, W, forced), (m, W, forced)
                n += 1
    assert n > 10000
    from xpoly_amd._capi import lib
    o = (C.c_int32 * 11)()
    for bad in ((0, 5, 0), (5, 0, 0), (5, 5, 3), (5, 5, -1)):
        assert lib().xpg_test_r32_loop_plan(*bad, o, 11) == -3
    assert lib().xpg_test_r32_loop_plan(5, 5, 0, None, 11) == -3
    o[5] = 77
    assert lib().xpg_test_r32_loop_plan(100, 300, 0, o, 5) == 0 and o[5] == 77      # n fields and no more


def test_size_rule_switches_loops_at_both_thresholds():
    for m, W, fused in RC.SIZE_RULE:
        assert RC.lib_plan(m, W)["fused"] == fused, (m, W, m * W)
        assert RC.lib_plan(m, W, RC.FUSED)["fused"] == 1 and RC.lib_plan(m, W, RC.PIPE)["fused"] == 0
    cells = sorted(m * W for m, W, _ in RC.SIZE_RULE)
    assert RC.FUSED_FROM in cells and RC.FUSED_UPTO in cells
    assert any(c < RC.FUSED_FROM for c in cells) and min(c for c in cells if c > RC.FUSED_UPTO) <= RC.FUSED_UPTO + 2000


def test_case_table_reaches_every_geometry_it_claims():
    fused = [RC.plan(c["m"], c["nv"] + c["m"] + 1, RC.FUSED) for c in RC.CASES if "fused" in c["loops"]]
    pipe = [RC.plan(c["m"], c["nv"] + c["m"] + 1, RC.PIPE) for c in RC.CASES if "pipe" in c["loops"]]
    assert {p["fN"] for p in fused} == {1, 2, 3, 4, 5, 15, 16}
    assert {p["pN"] for p in pipe} == {1, 2, 4, 5, 9, 16}
    assert {p["frows"] for p in fused} == {1, 2, 3}
    assert {p["prows"] for p in pipe} == {1, 2}
    assert {p["fNP"] for p in fused} == {1, 2, 3, 4, 5, 9} and {p["pNP"] for p in pipe} == {1, 2, 3, 4, 5, 9, 17}
    # the grid's max(m, N + NP) branch with more than one stager
    assert any(c["m"] < p["fN"] + p["fNP"] == p["fgx"] and p["fNP"] == 3
               for c, p in ((c, RC.plan(c["m"], c["nv"] + c["m"] + 1, RC.FUSED)) for c in RC.CASES if "fused" in c["loops"]))
    # the edges the issue names: one row in the second pick workgroup, the step from 15 to 16, W on either side of 256 and 512
    shapes = {(c["m"], c["nv"] + c["m"] + 1) for c in RC.CASES}
    assert {64, 65, 960, 961, 1024, 1025, 1088, 1100, 2049, 256, 257, 4100} <= {m for m, _ in shapes}
    assert {255, 256, 257, 512, 513} <= {W for _, W in shapes}
    # the default route: both loops, both sides of both thresholds stay in the host-only list
    default = [RC.plan(c["m"], c["nv"] + c["m"] + 1)["fused"] for c in RC.CASES]
    assert 0 in default and 1 in default
    by = {c["name"]: RC.plan(c["m"], c["nv"] + c["m"] + 1) for c in RC.CASES}
    assert by["craft-1100x8"]["fused"] == 1 and by["craft-2049x8"]["fused"] == 1 and by["craft-4100x3-p"]["fused"] == 0
    for c in RC.CASES:
        assert 1 in c["Ks"] and any(k % 2 for k in c["Ks"]) and any(k % 2 == 0 for k in c["Ks"])
    assert max(RC.BY_NAME["craft-4100x3-p"]["Ks"]) <= 4


def test_facts_of_every_case_are_the_recorded_ones(facts):
    assert set(facts) == set(RC.EXPECT)
    for name, f in facts.items():
        assert f == RC.EXPECT[name], name


def test_cases_do_what_the_gpu_tests_rest_on(facts):
    for c in RC.CASES:
        f = facts[c["name"]]
        assert f["status"] != -7, c["name"]                # the reference defines every case: none is skipped at run time
        if c["exact"]:
            assert f["appro"] == 0 and not f["phase_one"], c["name"]      # the Fraction replay holds: no float32 rescue
        if "upper" in f:
            assert f["upper"] == [], c["name"]             # the lower row of two identical rows wins (lpsol.h:604-611)
        if "second" in f and f["second"]:
            assert min(f["second"]) <= max(c["Ks"]) and any(k >= min(f["second"]) for k in c["Ks"])
    tall = [c["name"] for c in RC.CASES if c["kind"] == "craft" and c["m"] > RC.stride(c["m"], c["lanes"])]
    assert sorted(tall) == sorted(["craft-1025x8", "craft-1088x8", "craft-1100x8", "craft-2049x8", "craft-4100x3-p"])
    for name in tall:                                      # several rows per pick lane: a second-round row or a tie inside a lane
        assert facts[name]["second"] or facts[name]["lane_lo"], name
    for name in ("craft-1088x8", "craft-1100x8", "craft-2049x8", "craft-4100x3-p", "kk-1100x8"):
        assert facts[name]["second"] and facts[name]["lane_lo"], name
    for name in ("craft-65x6", "craft-961x7", "craft-257x8-p", "craft-1025x8-p"):
        assert facts[name]["alone"], name                  # the last pick workgroup's only row leaves
    assert sum(1 for f in facts.values() if f.get("wg_lo")) >= 8
    assert {n for n, f in facts.items() if f["phase_one"]} == {"rand1-1100x12", "rand2-1100x12", "rand2-65x8", "rand1-961x8"}
    assert {n for n, f in facts.items() if f["status"] == 0} == {"craft-961x7", "wide-33x222"}
    assert all(facts[n]["status"] == 2 for n in facts if facts[n]["phase_one"])
    for n in ("n0-130x40", "n0-300x40", "n0-1100x8"):
        assert facts[n]["weird"] and not facts[n]["phase_one"], n
    for n in ("wide-40x471", "wide-40x472", "wide-2x600"):     # entering and leaving columns on either side of a block edge
        assert len(facts[n]["enter_blocks"]) == 2 and len(facts[n]["leave_blocks"]) == 2, n


def test_fraction_replay_follows_the_checker(port):
    """The replay is fed the checker's trace here (the GPU's in the GPU suite): the columns it follows must be the checker's,
    cell for cell as values, and every step must take the lowest row of the minimum ratio with the constant column >= 0."""
    from fractions import Fraction
    for name in ("craft-65x6", "craft-1100x8", "wide-40x472", "craft-257x8-p"):
        c = RC.BY_NAME[name]
        leq, tg, _ = RC.build(c)
        K = max(c["Ks"])
        res = RC.two_stage_trace(port, leq, tg, K)
        cols = RC.replay_cols(c["m"], c["nv"], res["trace"])
        col, obj, rows = RC.replay(leq, tg, res["trace"], cols)
        assert rows == RC.leaving_rows(c["m"], c["nv"], res["trace"])
        for j in cols:
            assert [Fraction(int(n), int(d)) for n, d in res["tab"][:, j]] == col[j], (name, j)
            assert Fraction(int(res["tgtf"][j, 0]), int(res["tgtf"][j, 1])) == obj[j], (name, j)
