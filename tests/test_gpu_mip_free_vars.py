"""MIP trees with FREE variables walked on the device: a vc that is a sign pattern (diagonal -1 = x >= 0, 0 = free; what
Lineq::initVarConstraint builds, src/com/linsys.cpp:803-819) no longer sends the tree walk to the host controller --
k_mip_tree splits v = v' - v'' in front of every node LP as SIX::normalize does (src/com/lpsol.h:1365-1392).

Checkers (tests/free_var_cases.py): the CPU restatement in non-strict mode -- the real reference is undefined with a free
variable -- and the unchanged host controller, reached in a child process started with XPG_MIP_DEVICE=0. Every comparison
is exact: status, the optimum's bits, the solution's bits, and against the host controller the node count.
xpg_mip_last_route tells the two routes apart, whose answers are the same."""
import os
import subprocess
import sys

import numpy as np
import pytest

import free_var_cases as fc
from free_var_cases import F64, RAT
from tools import gen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch_answers(ctx, probs, kind, is_max, nfree):
    """mip_batch_vc over the problems, one call per free set; (status, v, sol) per problem. Every call must have taken
    the device route."""
    from xpoly_amd.six import mip_batch_vc, mip_last_route
    out = [None] * len(probs)
    for free, idx in fc.groups_by_free_set(probs):
        tg, vc, leq = fc.batch_arrays(probs, idx, kind)
        st, v, sol, nodes = mip_batch_vc(ctx, is_max, False, tg, vc, leq, kind=kind)
        r = mip_last_route()
        assert r == dict(device_trees=len(idx), host_trees=0, free_vars=nfree), (free, r)
        assert nodes >= len(idx)
        for k, i in enumerate(idx):
            out[i] = (st[k], v[k], sol[k])
    return out


@pytest.mark.parametrize("kind", [RAT, F64])
@pytest.mark.parametrize("shape", fc.SHAPES)
def test_integer_programs_with_free_variables_match_the_oracle(ctx, port, shape, kind):
    """256 programs per shape, maxm and minm: the oracle decides all 512 (no -7), so nothing is skipped."""
    probs = fc.shape_problems(shape)
    seen, negative, compared = set(), 0, 0
    for is_max in (True, False):
        want = fc.oracle_answers(port, shape, kind, is_max)
        got = _batch_answers(ctx, probs, kind, is_max, shape[2])
        for i in range(len(probs)):
            assert want[i][0] != -7, (shape, kind, is_max, i)
            assert fc.same_answer(*got[i], want[i]), (shape, kind, is_max, i, got[i], want[i])
            seen.add(int(want[i][0]))
            if want[i][0] == 0:
                s = np.asarray(want[i][2])
                negative += bool(((s[..., 0] if kind == RAT else s)[:-1] < 0).any())
            compared += 1
    assert compared == 2 * fc.PER_SHAPE
    assert seen == {0, 1, 2}, seen
    assert negative > 0.25 * compared, negative                   # the free variables do go below zero


def test_host_controller_gives_the_same_batches_and_node_counts(ctx):
    """The same batches in a child process with XPG_MIP_DEVICE=0 (read once per process): sha256 over status + v + sol and
    the node count are equal; here every tree takes the device, there none."""
    mine = fc.batch_digests(ctx)
    for line, r, nb in mine:
        assert r["device_trees"] == nb and r["host_trees"] == 0, (line, r)
    code = ("import sys; sys.path.insert(0, 'tests')\n"
            "import xpoly_amd, free_var_cases as fc\n"
            "ctx = xpoly_amd.Context(0)\n"
            "for line, r, nb in fc.batch_digests(ctx):\n"
            "    assert r['device_trees'] == 0 and r['host_trees'] == nb and r['free_vars'] == 0, (line, r)\n"
            "    print('D', line)\n")
    env = dict(os.environ, XPG_MIP_DEVICE="0", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    theirs = [l[2:] for l in r.stdout.splitlines() if l.startswith("D ")]
    assert len(theirs) == len(mine) and len(mine) >= 4 * 2 * 2
    for (line, _, _), other in zip(mine, theirs):
        assert line == other


@pytest.mark.parametrize("shape", fc.SHAPES)
def test_single_calls_take_the_device_and_agree_with_batch_and_oracle(ctx, port, shape):
    """MIP.maxm / minm (both kinds) and has_solution(int; unique and not) on the first 32 problems of the shape."""
    from xpoly_amd.six import MIP, has_solution, mip_last_route
    count = 32
    probs = fc.shape_problems(shape)
    for kind in (RAT, F64):
        mip = MIP(ctx, kind)
        for is_max in (True, False):
            want = fc.oracle_answers(port, shape, kind, is_max)
            batch = _batch_answers(ctx, probs, kind, is_max, shape[2])
            for i in range(count):
                tg, vc, leq = fc.batch_arrays(probs, [i], kind)
                got = (mip.maxm if is_max else mip.minm)(tg[0], vc, None, leq[0])
                r = mip_last_route()
                assert r["host_trees"] == 0 and r["device_trees"] >= 1 and r["free_vars"] == shape[2], (shape, kind, i, r)
                assert fc.same_answer(*got, want[i]), (shape, kind, is_max, i, got, want[i])
                assert fc.same_answer(*got, batch[i]), (shape, kind, is_max, i)
    with fc.non_strict(port):
        for i in range(count):
            tg, vc, leq = fc.batch_arrays(probs, [i], RAT)
            for unique in (True, False):
                want = port.has_solution(leq[0], None, vc, shape[1], True, unique)
                assert want != -7, (shape, i, unique)
                got = has_solution(ctx, leq[0], None, vc, shape[1], True, unique)
                r = mip_last_route()
                assert r["host_trees"] == 0 and 1 <= r["device_trees"] <= 2, (shape, i, unique, r)
                assert got == want, (shape, i, unique, got, want)


@pytest.mark.parametrize("kind", [RAT, F64])
def test_equalities_at_the_root_and_01_branching_with_free_variables(ctx, port, kind):
    """tests/mip_eq_cases.py's programs with one or two variables made free, through MIP. The reference is undefined on part
    of them (convertEq2Ineq reads the equality at the inequality's row index): the oracle leaves out 17-18 %; at most 25 % may
    be skipped. These shapes are tiny, so (nearly) every compared call must have walked its tree on the device."""
    from xpoly_amd.six import MIP, mip_last_route
    mip = MIP(ctx, kind)
    compared, on_device, seen = 0, 0, {}
    for it, (p, is_bin) in enumerate(fc.free_var_eq_problems(kind)):
        for is_max in (True, False):
            with fc.non_strict(port):
                want = port.mip_solve(kind, is_max, is_bin, p["tgtf"], p["vc"], p["eq"], p["leq"], p.get("ind"))
            if want[0] == -7:
                continue
            got = (mip.maxm if is_max else mip.minm)(p["tgtf"], p["vc"], p["eq"], p["leq"], is_bin, p.get("ind"))
            r = mip_last_route()
            assert fc.same_answer(*got, want), (it, is_max, is_bin, got, want)
            assert r["device_trees"] + r["host_trees"] == 1, r
            on_device += r["device_trees"]
            compared += 1
            seen[int(want[0])] = seen.get(int(want[0]), 0) + 1
    print("kind %d: compared %d of 480, statuses %s, on the device %d (%.1f %%)" % (kind, compared, seen, on_device, 100.0 * on_device / compared))
    assert compared >= 360, compared
    assert 0 in seen and len(seen) >= 3, seen
    assert on_device > 0.8 * compared, (on_device, compared)


def test_a_general_vc_still_works_and_goes_to_the_host_controller(ctx, port):
    """A diagonal of -2 and a nonzero constant are not sign patterns: mip_batch_vc hands them to the host controller with
    the caller's vc, and the answers are the oracle's."""
    from xpoly_amd.six import mip_batch_vc, mip_last_route
    nb = 64
    probs = fc.shape_problems((3, 4, 1), nb)
    tg = gen.to_rat(np.stack([p["tgtf"] for p in probs])); leq = gen.to_rat(np.stack([p["leq"] for p in probs]))
    for vc0 in fc.general_vcs(4):
        vc = gen.to_rat(vc0)
        seen = set()
        for is_max in (True, False):
            st, v, sol, nodes = mip_batch_vc(ctx, is_max, False, tg, vc, leq)
            r = mip_last_route()
            assert r == dict(device_trees=0, host_trees=nb, free_vars=0), r
            with fc.non_strict(port):
                for b in range(nb):
                    want = port.mip_solve(RAT, is_max, False, tg[b], vc, None, leq[b])
                    assert want[0] != -7, b
                    assert fc.same_answer(st[b], v[b], sol[b], want), (is_max, b, st[b], want)
                    seen.add(int(want[0]))
        assert seen == {0, 1, 2}, seen


def test_dependence_polyhedra_with_symbols_as_variables_at_batch_size(ctx, port):
    """4096 parametrised polyhedra per shape in one call: move2var, reduce and both walks stay on the device, the symbols
    (and the caller's free variables) split per node. The oracle decides every one of the first 1024 of each shape."""
    from xpoly_amd.six import dep_is_empty_batch, dep_is_empty_batch_symbols_as_vars, mip_last_route
    check = 1024
    for (nv, ns, rows), mats in fc.dep_systems():
        assert mats.shape[0] == 4096
        for vc0 in ((None,) if (nv, ns) != (3, 2) else (None, gen.to_rat(gen.vc_nonneg(nv, False, free=(1,))))):
            got, nodes = dep_is_empty_batch_symbols_as_vars(ctx, mats, nv, vc=vc0)
            r = mip_last_route()
            assert r["host_trees"] == 0 and r["device_trees"] >= 1 and r["free_vars"] == ns + (0 if vc0 is None else 1), r
            parity, _ = dep_is_empty_batch(ctx, mats, rhs_idx=nv, vc=vc0)
            wide = fc.dep_wide_vc(nv, ns, vc0)
            seen = {}
            with fc.non_strict(port):
                for b in range(check):
                    by_reduce, want = fc.dep_oracle(port, mats[b], nv, ns, wide)
                    assert want != -7, (nv, ns, b)
                    assert got[b] == want, (nv, ns, b, got[b], want)
                    assert parity[b] == (want if by_reduce is not None else -7), (nv, ns, b)   # parity mode: unchanged
                    seen[(by_reduce, want)] = seen.get((by_reduce, want), 0) + 1
            assert (None, 0) in seen and (None, 1) in seen, seen
            assert set(np.unique(got[check:])) <= {0, 1}
    # no symbols, a caller's vc that frees variable 1: the all-on-device branch takes it too
    (nv, ns, rows), mats = fc.dep_systems(512)[0]
    pattern = gen.to_rat(gen.vc_nonneg(nv + ns, False, free=(1,)))
    got, _ = dep_is_empty_batch(ctx, mats, vc=pattern)
    r = mip_last_route()
    assert r["host_trees"] == 0 and r["device_trees"] >= 1 and r["free_vars"] == 1, r
    verdicts = set()
    with fc.non_strict(port):
        for b in range(512):
            _, want = fc.dep_oracle(port, mats[b], nv + ns, 0, pattern)
            assert want != -7, b
            assert got[b] == want, (b, got[b], want)
            verdicts.add(want)
    assert verdicts == {0, 1}


def test_node_lps_too_wide_for_lds_go_to_the_host_controller(ctx, port):
    """fp64, 20 variables of which 16 are free, 50 inequalities: the node LPs fit the walk's 64 KB without the twins and
    not with them, so the batch is the host controller's -- same answers as the oracle."""
    import ctypes as C
    from xpoly_amd._capi import lib
    from xpoly_amd.six import mip_batch_vc, mip_last_route
    tg, vc, leq = fc.wide_lp_f64()
    nb, rows, cols = leq.shape
    assert (rows, cols) == (50, 21)
    fits = lambda extra: lib().xpg_test_mip_fits(C.c_int(F64), C.c_int(rows), C.c_int(0), C.c_int(cols), C.c_int(0), C.c_int(extra))
    assert fits(0) == 1 and fits(16) == 0
    seen = set()
    for is_max in (True, False):
        st, v, sol, nodes = mip_batch_vc(ctx, is_max, False, tg, vc, leq, kind=F64)
        r = mip_last_route()
        assert r == dict(device_trees=0, host_trees=nb, free_vars=0), r
        with fc.non_strict(port):
            for b in range(nb):
                want = port.mip_solve(F64, is_max, False, tg[b], vc, None, leq[b])
                assert want[0] != -7, b
                assert fc.same_answer(st[b], v[b], sol[b], want), (is_max, b, st[b], want)
                seen.add(int(want[0]))
    assert 0 in seen and len(seen) >= 2, seen
