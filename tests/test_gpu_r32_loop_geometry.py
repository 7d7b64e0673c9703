"""The two HBM-resident Rational simplex loops -- one launch per pivot (csrc/lp_fused_r32.hip.h) and two launches
(csrc/lp_pipe_r32.hip.h) -- at every launch geometry of r32_loop_plan (lp_host.hip.h): the LPs of tests/r32_loop_cases.py, whose
pivots leave on second-round rows of a pick lane, on the lower of two identical rows of one lane and of two pick workgroups, on
the last workgroup's only row; stager counts 1 .. 9 with entering, leaving and constant columns on either side of a block edge;
the grid's N + NP > m branch; phase one with ties; cells not in lowest terms and n/0 cells at several workgroups. Every
(case, K) is compared bit for bit with the checker (status, tableau, objective row, basis maps, pivot trace, maxv / sol at an
end state), with the real reference where it is built, across the forced loops, two spacings of the generic point and the
default route, and -- the exact set -- with K pivots of lpsol.h:1471-1510 replayed in fractions.Fraction
(tests/test_r32_loop_host.py asserts, without a GPU, that the cases do what is claimed here). One child process per
environment: XPG_R32_LOOP is read once per process."""
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import r32_loop_cases as RC                              # noqa: E402

ENVS = {
    "fused": ("fused", dict(XPG_R32_LOOP="fused")),
    "pipe": ("pipe", dict(XPG_R32_LOOP="pipe")),
    "fused-g1": ("fused", dict(XPG_R32_LOOP="fused", XPG_R32_GENERIC_EVERY="1")),
    "fused-g3": ("fused", dict(XPG_R32_LOOP="fused", XPG_R32_GENERIC_EVERY="3")),
    "default": (None, {}),
}
_runs, _want = {}, {}


def run(name):
    """The records of one worker run, {(case, K): record}; one child process per environment, made once."""
    if name not in _runs:
        from conftest import hooks_env
        loop, over = ENVS[name]
        env = hooks_env()                                # (XPG_R32_GENERIC_EVERY is a hook-only switch: the -DXPG_TEST_HOOKS build)
        for k in ("XPG_R32_LOOP", "XPG_R32_GENERIC_EVERY"):
            env.pop(k, None)
        env.update(over, R32_LOOP_CASES=loop or "")
        r = subprocess.run([sys.executable, os.path.join(HERE, "r32_loop_worker.py")], cwd=ROOT, env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        recs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        _runs[name] = {(x["name"], x["K"]): x for x in recs}
        assert len(_runs[name]) == len(recs) == sum(len(c["Ks"]) for c in RC.CASES if RC.runs_in(c, loop)), name
    return _runs[name]


def want(port, case, K):
    """The checker's record of (case, K), made once."""
    key = (case["name"], K)
    if key not in _want:
        leq, tg, _ = RC.build(case)
        res = RC.two_stage_trace(port, leq, tg, K)
        cols = RC.replay_cols(case["m"], case["nv"], res["trace"]) if case["exact"] else None
        _want[key] = RC.record(res, case, K, cols)
    return _want[key]


def state(rec):
    return {k: v for k, v in rec.items() if k != "ran"}


def check_against_checker(port, name):
    loop = ENVS[name][0]
    got = run(name)
    n = 0
    for case in RC.CASES:
        if not RC.runs_in(case, loop):
            continue
        for K in case["Ks"]:
            g, w = got[(case["name"], K)], want(port, case, K)
            for k in w:                                  # field by field, so that a failure names the array
                assert g.get(k) == w[k], (name, case["name"], K, k)
            assert state(g) == w, (name, case["name"], K)
            if loop:
                assert g["ran"] == loop, (name, case["name"], K, g["ran"])
            n += 1
    assert n == len(got)
    # what the comparison rests on did take place: end states, tableaux read back after odd and even pivot counts
    assert any(r["status"] == 0 and "sol" in r for r in got.values())
    assert {len(r["trace"]) // 2 % 2 for r in got.values() if r["status"] == 4} == {0, 1}


def test_forced_fused_loop_matches_checker(port):
    check_against_checker(port, "fused")


def test_forced_two_launch_loop_matches_checker(port):
    check_against_checker(port, "pipe")
    assert ("craft-4100x3-p", 4) in run("pipe")          # the second row of a pick lane of the two-launch loop: 4100 rows


def test_generic_point_before_every_and_every_third_launch_gives_the_same_records(port):
    base = run("fused")
    for name in ("fused-g1", "fused-g3"):
        other = run(name)
        assert other.keys() == base.keys()
        for key in base:
            assert other[key] == base[key], (name, key)


def test_default_route_takes_the_planned_loop_and_gives_the_same_records(port):
    got = run("default")
    for case in RC.CASES:
        for K in case["Ks"]:
            g = got[(case["name"], K)]
            phase_one = RC.EXPECT[case["name"]]["phase_one"]
            W = case["nv"] + case["m"] + (2 if phase_one and g["status"] == 2 else 1)     # phase one: the artificial variable's column
            assert g["ran"] == ("fused" if RC.plan(case["m"], W)["fused"] else "pipe"), (case["name"], K, g["ran"])
            for name in case["loops"]:                   # all environments: identical records
                assert state(run(name)[(case["name"], K)]) == state(g), (name, case["name"], K)
            assert state(g) == want(port, case, K), (case["name"], K)
    ran = {(c["name"], got[(c["name"], max(c["Ks"]))]["ran"]) for c in RC.CASES}
    assert ("craft-1100x8", "fused") in ran and ("craft-2049x8", "fused") in ran and ("craft-4100x3-p", "pipe") in ran and ("craft-1024x8", "fused") in ran
    assert ("craft-64x6", "pipe") in ran


@pytest.mark.parametrize("part", range(3))
def test_matches_the_real_reference(ref, part):
    """The same records from the real reference (it keeps no pivot trace): every case at its largest budget -- the state after
    K pivots holds every earlier one -- from the forced runs; a third of the table per test."""
    n = 0
    for case in RC.CASES[part::3]:
        leq, tg, _ = RC.build(case)
        K = max(case["Ks"])
        g = run("fused" if "fused" in case["loops"] else "pipe")[(case["name"], K)]
        res = ref.two_stage(RC.RAT, leq, tg, K)
        res["trace"] = np.asarray(g["trace"])
        w = RC.record(res, case, K, g.get("cols"))
        for k in w:
            assert g.get(k) == w[k], (case["name"], K, k)
        n += 1
    assert n >= len(RC.CASES) // 3


def test_exact_set_against_fraction_replay():
    """K pivots of SIX::pivot (lpsol.h:1471-1510) in fractions.Fraction, driven by the GPU's own pivot trace, on the constant
    column, every entering column and 16 sampled ones, and the objective row: the GPU's cells must be those values (the set
    has no float32 rescue: tests/test_r32_loop_host.py); at every step the row left is the lowest row of the minimum
    ratio and the constant column stays >= 0."""
    n = 0
    for case in RC.CASES:
        if not case["exact"]:
            continue
        leq, tg, _ = RC.build(case)
        for name in case["loops"]:
            g = run(name)[(case["name"], max(case["Ks"]))]
            trace = np.asarray(g["trace"]).reshape(-1, 2)
            assert len(trace) == RC.EXPECT[case["name"]]["pivots"]
            cols = g["cols"]
            assert cols == RC.replay_cols(case["m"], case["nv"], trace)
            col, obj, _ = RC.replay(leq, tg, trace, cols)
            tab = np.asarray(g["tabcols"], dtype=np.int64).reshape(case["m"], len(cols), 2)
            ob = np.asarray(g["objcols"], dtype=np.int64).reshape(len(cols), 2)
            assert (tab[..., 1] > 0).all() and (ob[..., 1] > 0).all()
            for k, j in enumerate(cols):
                assert [Fraction(int(a), int(b)) for a, b in tab[:, k]] == col[j], (name, case["name"], j)
                assert Fraction(int(ob[k, 0]), int(ob[k, 1])) == obj[j], (name, case["name"], j)
            n += 1
            if name == "fused" and "pipe" in case["loops"]:   # the other loop's record is this one (identical records): replayed once
                assert state(run("pipe")[(case["name"], max(case["Ks"]))]) == state(g)
                break
    assert n == sum(1 for c in RC.CASES if c["exact"])


@pytest.mark.parametrize("name", ["craft-1100x8", "craft-2049x8"])
def test_tall_default_route_in_chunks_equals_one_shot(ctx, name):
    """Several rows per pick lane on the route the size rule takes by itself: chunks of 1, 2, 3, ... launches (every call
    starts with a generic point and ends on either side of the ping-pong tableau) leave the state one call leaves."""
    import xpoly_amd
    case = RC.BY_NAME[name]
    leq, tg, _ = RC.build(case)
    a = xpoly_amd.DeviceLP(ctx, RC.RAT, leq, tg); a.begin()
    for k in (1, 2, 3, 1):
        assert a.iterate(k) == xpoly_amd.six.XPG_RUNNING
        assert a.r32_loop_ran() == "fused"
        assert a.read()["tab"].shape[0] == case["m"]      # a read between the calls must not disturb the loop
    b = xpoly_amd.DeviceLP(ctx, RC.RAT, leq, tg); b.begin()
    assert b.iterate(7) == xpoly_amd.six.XPG_RUNNING
    ra, rb = a.read(), b.read()
    assert a.pivots_done() == b.pivots_done() == 7
    assert np.array_equal(a.trace(), b.trace())
    assert RC.EXPECT[name]["second"] and min(RC.EXPECT[name]["second"]) <= 7
    for k in ("tab", "tgtf", "nvset", "bvset", "bv2eq", "eq2bv"):
        assert np.array_equal(ra[k], rb[k]), k
    a.close(); b.close()
