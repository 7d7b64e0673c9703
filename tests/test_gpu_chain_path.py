"""The chain launch's path inside one wave (lp_chain.hip.h): the 64-bit wave minimum as two 32-bit minima and 1 / pivot
computed by the lane that publishes the record, on ties and near-ties between pick workers, under forced aborts of the roll
call and at the smallest grids. Every solve is compared with the pipelined loop, which shares none of that code, bit for bit."""
import numpy as np
import pytest

from conftest import needs_hooks

from tools import gen

pytestmark = pytest.mark.gpu
F64 = 0
STATE = ("tab", "tgtf", "nvset", "bvset", "bv2eq", "eq2bv")


def same_state(got, want, what):
    for k in STATE:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and (np.array_equal(a.view(np.uint64), b.view(np.uint64))
                                       if a.dtype == np.float64 else np.array_equal(a, b)), (what, k)


def solve(mode, leq, tg, Ks, monkeypatch):
    """{K: (status, state, chain runs, chain aborts)} of TwoStageMethod(max_iter = K) through the loop `mode`."""
    import xpoly_amd
    monkeypatch.setenv("XPG_LOOP", mode)
    c = xpoly_amd.Context(0)
    out = {}
    for K in Ks:
        lp = xpoly_amd.DeviceLP(c, F64, leq, tg)
        st = lp.two_stage(K)
        got = lp.read()
        aborts, _ = lp.chain_aborts()
        out[K] = (st, got, lp.chain_runs, aborts)
        lp.close()
    c.close()
    return out


def blocked_equals_pipelined(leq, tg, Ks, monkeypatch, what):
    want = solve("pipe", leq, tg, Ks, monkeypatch)
    got = solve("block", leq, tg, Ks, monkeypatch)
    for K in Ks:
        assert got[K][0] == want[K][0], (what, K, got[K][0], want[K][0])
        same_state(got[K][1], want[K][1], (what, K))
    return got


def tied_lp():
    """191 x 192 (W = 384: three pick workers, six prep workers): gen.hard_lp_f64(64, 192) three times over. Rows 64..127 are
    rows 0..63 again, rows 128..190 are rows 0..62 times 2 (an exact scaling: the same ratios), and the right-hand side of
    row 64 + 17 is one ulp up."""
    a, tg = gen.hard_lp_f64(64, 192)
    leq = np.concatenate([a, a, 2.0 * a[:63]], axis=0)
    leq[64 + 17, -1] = np.nextafter(leq[64 + 17, -1], np.inf)
    return np.ascontiguousarray(leq), tg


def test_ties_and_near_ties_between_pick_workers(monkeypatch):
    """Equal ratios in different pick workers (the lowest row must win) and keys that differ in the low word only, at
    K = 40 and 400 against the pipelined loop. Checked on the CPU with the oracle (its states after k = 0 .. 399 pivots of
    this LP, the ratio b_i / a_i,nv of every row with a_i,nv > 0 in the column that enters next): 112 of the 400 stages have
    the least ratio in rows of more than one pick worker -- 19 of the stages 1 .. 31, which the first chain launch runs, and
    25 of the first 40 --, and five stages (8, 156, 167, 229, 256) have another candidate whose key shares the minimum's high
    word and differs in the low one: at stage 8 rows 17 and 145 hold the least ratio and row 81, whose right-hand side is
    the ulp up, the next key."""
    leq, tg = tied_lp()
    got = blocked_equals_pipelined(leq, tg, (40, 400), monkeypatch, "ties")
    assert got[400][2] > 0, got[400][2:]                  # the chain launches really ran


@needs_hooks
@pytest.mark.parametrize("k", [3, -3])
def test_forced_aborts_of_the_roll_call_and_of_the_placement_check(monkeypatch, k):
    """The roll call failing on every third launch (3) and the placement check on every third
    one-XCD launch (-3): a 511 x 512 LP at K = 1200 equals the pipelined loop's, and launches both ran and aborted."""
    leq, tg = gen.hard_lp_f64(511, 512)
    monkeypatch.setenv("XPG_CHAIN_TEST_ABORT", str(k))
    got = blocked_equals_pipelined(leq, tg, (1200,), monkeypatch, ("abort", k))
    runs, aborts = got[1200][2:]
    assert runs > 0 and aborts > 0, (k, runs, aborts)


@pytest.mark.parametrize("shape", [(63, 64), (64, 4031)])
def test_smallest_grids(monkeypatch, shape):
    """63 x 64 (W = 128: one pick worker, two prep workers) and 64 x 4031 (W = 4096, a leading dimension that is a multiple
    of 512) at K = 200: the smallest grids, one pick worker whose record is the only one every prep worker combines."""
    m, n = shape
    leq, tg = gen.hard_lp_f64(m, n)
    got = blocked_equals_pipelined(leq, tg, (200,), monkeypatch, shape)
    assert got[200][2] > 0, got[200][2:]
