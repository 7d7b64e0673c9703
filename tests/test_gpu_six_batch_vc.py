"""Batches of LPs with equalities and free variables in one launch (xpg_six_batch_vc_*): SIX::normalize
(src/com/lpsol.h:1290-1394, convertEq2Ineq :1197-1278), the LDS-resident solve and calcFinalSolution (:1851-1899) on the
device for the whole batch.

Checkers (tests/six_eq_cases.py): the CPU restatement -- non-strict where a variable is free, the real reference being
undefined there -- and the unchanged single-problem route SIX.maxm / minm, which reshapes on the host. Every comparison is
exact: status, the optimum's bits, the solution's bits. six_batch_last_route tells the device route from the per-problem
fallback, whose answers are the same."""
import os
import subprocess
import sys

import numpy as np
import pytest

import free_var_cases as fc
import six_eq_cases as sc
from conftest import hooks_env, needs_hooks
from free_var_cases import F64, RAT
from tools import gen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch(ctx, shape, kind, is_max, count=sc.PER_SHAPE, vc=None, max_iter=0xFFFFFFFF):
    from xpoly_amd.six import six_batch_vc
    tg, vc0, eq, leq = sc.shape_arrays(shape, kind, count)
    return six_batch_vc(ctx, kind, is_max, tg, vc0 if vc is None else vc, leq, eq, max_iter=max_iter)


def _singles(ctx, kind, is_max, tg, vc, eq, leq, max_iter=0xFFFFFFFF):
    """SIX.maxm / minm one problem at a time: the host-reshaping route."""
    from xpoly_amd.six import SIX
    six = SIX(ctx, kind)
    six.set_param(0, max_iter)
    solve = six.maxm if is_max else six.minm
    return [solve(tg[i], vc, None if eq is None else eq[i], None if leq is None else leq[i]) for i in range(tg.shape[0])]


@pytest.mark.parametrize("kind", [RAT, F64])
def test_batches_match_the_oracle(ctx, port, kind):
    """Every shape x direction is one batch call of 256 LPs (64 for the shape with 66 equalities, minm only). A problem is
    skipped only where the oracle itself returns -7, at most 4 of the 512 per shape (the generator's measured maximum is 1)."""
    from xpoly_amd.six import six_batch_last_route
    seen, negative = set(), 0
    for shape in sc.SHAPES + (sc.WIDE_EQ,):
        skipped, nb = 0, sc.cases_of(shape)
        for is_max in sc.directions(shape):
            want = sc.oracle_answers(port, shape, kind, is_max)
            st, v, sol = _batch(ctx, shape, kind, is_max, nb)
            r = six_batch_last_route()
            assert r == dict(device=nb, fallback=0, free=shape[3]), (shape, is_max, r)
            for i in range(nb):
                if want[i][0] == -7:
                    skipped += 1
                    continue
                assert fc.same_answer(st[i], v[i], sol[i], want[i]), (shape, kind, is_max, i, st[i], v[i], sol[i], want[i])
                seen.add(int(want[i][0]))
                if want[i][0] == 0 and shape[3] > 0:
                    s = np.asarray(want[i][2])
                    negative += bool(((s[..., 0] if kind == RAT else s)[:-1] < 0).any())
        print("shape %s kind %d: skipped %d of %d" % (shape, kind, skipped, nb * len(sc.directions(shape))))
        assert skipped <= 4, (shape, kind, skipped)
    assert seen == {0, 1, 2, 3}, seen
    assert negative >= 40, negative                              # the free variables do go below zero


@pytest.mark.parametrize("kind", [RAT, F64])
def test_batch_equals_single_calls_bit_for_bit(ctx, kind):
    """The first 64 problems of every shape, and of four more: no inequalities at all (leq = None); more inequality rows
    than columns, where the reference's leading-value index (lpsol.h:1232) leaves the row for some LPs -- those alone end -7,
    in the batch as in their single calls; and two sizes at which the batch runs 128 and 256 threads per LP (a single call
    picks its threads by the rows its own normal form has); and the shape with 66 equalities, minm only. Statuses of -7 are
    compared like any other."""
    count = 64
    statuses = {}
    for shape in sc.SHAPES + sc.EXTRA_SHAPES + (sc.WIDE_EQ,):
        tg, vc, eq, leq = sc.shape_arrays(shape, kind, count)
        assert (leq is None) == (shape[0] == 0)
        for is_max in sc.directions(shape):
            st, v, sol = _batch(ctx, shape, kind, is_max, count)
            one = _singles(ctx, kind, is_max, tg, vc, eq, leq)
            for i in range(count):
                assert fc.same_answer(st[i], v[i], sol[i], one[i]), (shape, kind, is_max, i, st[i], v[i], sol[i], one[i])
                if st[i] != 0:
                    assert not sol[i].any(), (shape, i)                  # written on status 0 only
                statuses.setdefault(shape, set()).add(int(st[i]))
    assert -7 in statuses[(9, 2, 4, 0)] and len(statuses[(9, 2, 4, 0)]) >= 2, statuses      # some LPs of the batch, not all
    assert 0 in statuses[(0, 2, 4, 1)], statuses


def test_a_general_vc_and_a_shape_beyond_64_kb_fall_back_per_problem(ctx):
    from xpoly_amd.six import six_batch_last_route
    shape, count = (5, 2, 5, 1), 16
    for kind in (RAT, F64):
        tg, _, eq, leq = sc.shape_arrays(shape, kind, count)
        for vc0 in fc.general_vcs(5):
            vc = gen.to_rat(vc0) if kind == RAT else np.ascontiguousarray(vc0, dtype=np.float64)
            for is_max in (True, False):
                st, v, sol = _batch(ctx, shape, kind, is_max, count, vc=vc)
                assert six_batch_last_route() == dict(device=0, fallback=count, free=0)
                one = _singles(ctx, kind, is_max, tg, vc, eq, leq)
                for i in range(count):
                    assert fc.same_answer(st[i], v[i], sol[i], one[i]), (kind, is_max, i, st[i], one[i])
    # fp64, the first square shape the plan view refuses for maxm
    from xpoly_amd.six import six_batch_vc
    nv = sc.largest_square(True) + 1
    rc, out = sc.plan_view(gen.vc_nonneg(nv, False), F64, nv, 1, True)
    assert rc == 0 and out[0] == 0
    tg, vc, eq, leq = sc.dense_square(nv)
    st, v, sol = six_batch_vc(ctx, F64, True, tg, vc, leq, eq, max_iter=64)
    assert six_batch_last_route() == dict(device=0, fallback=4, free=0)
    one = _singles(ctx, F64, True, tg, vc, eq, leq, max_iter=64)
    for i in range(4):
        assert fc.same_answer(st[i], v[i], sol[i], one[i]), (i, st[i], one[i])


def _cycled(shape, kind, nb):
    tg, vc, eq, leq = sc.shape_arrays(shape, kind)
    idx = np.arange(nb) % sc.PER_SHAPE
    return tg[idx], vc, eq[idx], leq[idx]


@pytest.mark.parametrize("kind", [RAT, F64])
def test_launch_geometry(ctx, kind):
    """nb = 1, 3 and 257 (one more LP than the cases hold, cycled): LP i is problem i mod 256 of the 256-LP call."""
    from xpoly_amd.six import six_batch_vc, six_batch_last_route
    shape = (5, 2, 5, 1)
    for is_max in (True, False):
        st0, v0, sol0 = _batch(ctx, shape, kind, is_max)
        for nb in (1, 3, 257):
            tg, vc, eq, leq = _cycled(shape, kind, nb)
            st, v, sol = six_batch_vc(ctx, kind, is_max, tg, vc, leq, eq)
            assert six_batch_last_route() == dict(device=nb, fallback=0, free=1)
            idx = np.arange(nb) % sc.PER_SHAPE
            assert np.array_equal(st, st0[idx]) and v.tobytes() == v0[idx].tobytes() and sol.tobytes() == sol0[idx].tobytes(), (is_max, nb)


def grid_digest(ctx):
    """sha256 over status + v + sol of 37 LPs of (5,2,5,1), per kind and direction."""
    import hashlib
    from xpoly_amd.six import six_batch_vc
    out = []
    for kind in (RAT, F64):
        for is_max in (True, False):
            tg, vc, eq, leq = _cycled((5, 2, 5, 1), kind, 37)
            st, v, sol = six_batch_vc(ctx, kind, is_max, tg, vc, leq, eq)
            out.append("%d %d %s" % (kind, is_max, hashlib.sha256(st.tobytes() + v.tobytes() + sol.tobytes()).hexdigest()))
    return out


@needs_hooks
def test_a_capped_grid_walks_the_batch_in_strides(ctx):
    """XPG_SIX_VC_GRID=2 (hooks build; read once per process, hence the child): two workgroups take 37 LPs in turn, each LP
    through the same scratch slot and LDS block as the one before -- the answers are those of the uncapped launch."""
    mine = grid_digest(ctx)
    code = ("import sys; sys.path.insert(0, 'tests')\n"
            "import xpoly_amd, test_gpu_six_batch_vc as t\n"
            "ctx = xpoly_amd.Context(0)\n"
            "for line in t.grid_digest(ctx):\n"
            "    print('D', line)\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=hooks_env(XPG_SIX_VC_GRID="2"), cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    theirs = [l[2:] for l in r.stdout.splitlines() if l.startswith("D ")]
    assert theirs == mine and len(mine) == 4


DEV_SCRIPT = r"""
import sys
import numpy as np
import torch                                   # torch's HIP runtime first, then the library's (the order bench.py uses)
torch.zeros(1, device="cuda")
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import xpoly_amd
from xpoly_amd.six import six_batch_vc, six_batch_last_route
import six_eq_cases as sc
ctx = xpoly_amd.Context(0)
shape = (3, 3, 6, 2)
for kind in (1, 0):
    tg, vc, eq, leq = sc.shape_arrays(shape, kind)
    nb, cols = tg.shape[0], tg.shape[1]
    for is_max in (True, False):
        st0, v0, sol0 = six_batch_vc(ctx, kind, is_max, tg, vc, leq, eq)
        d = [torch.from_numpy(np.array(a)).cuda() for a in (tg, vc, eq, leq)]     # (copies: the cases are read-only)
        for trimmed in (False, True):
            if trimmed:
                ctx.trim()
            st = torch.full((nb,), 99, dtype=torch.int32, device="cuda")
            v = torch.zeros_like(torch.from_numpy(v0)).cuda(); sol = torch.zeros_like(torch.from_numpy(sol0)).cuda()
            torch.cuda.synchronize()
            ctx.six_batch_vc_dev(kind, is_max, nb, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), eq.shape[1], d[3].data_ptr(),
                                 leq.shape[1], cols, st.data_ptr(), v.data_ptr(), sol.data_ptr())
            ctx.sync()
            assert six_batch_last_route() == dict(device=nb, fallback=0, free=-1)
            assert st.cpu().numpy().tobytes() == st0.tobytes(), (kind, is_max, trimmed)
            assert v.cpu().numpy().tobytes() == v0.tobytes(), (kind, is_max, trimmed)
            assert sol.cpu().numpy().tobytes() == sol0.tobytes(), (kind, is_max, trimmed)
            assert (st0 == 0).any() and (st0 != 0).any()
print("DEV OK")
"""


def test_device_arrays_give_the_host_call_bytes_also_after_a_trim():
    """torch device tensors for every array of (3,3,6,2), vc included; the call only enqueues, ctx.sync() follows. Status,
    optimum and solution are the host-array call's bytes (rows of failed LPs stay as they were: zero on both sides), and
    again after xpg_trim has returned the scratch slots. In a process of its own: torch's HIP runtime comes up first."""
    r = subprocess.run([sys.executable, "-c", DEV_SCRIPT, ROOT], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and "DEV OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
