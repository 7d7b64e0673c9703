"""GPU parity of the fused calcBound entry points (xpg_lineq_bounds_batch_*: every elimination chain of every system in ONE
launch of k_calc_bound_batch, the chains' shared prefixes walked once) against the CPU checker's fme applied chain by chain and
step after step (tests/lineq_bounds_cases.py chains), against the reference's own build where it is present, and against the
chained-launch route the library keeps (Lineq.calcBound_packed). Bit-exact: nothing is compared with a tolerance."""
import json
import os
import subprocess

import numpy as np
import pytest

import lineq_bounds_cases as bc
from lineq_bounds_cases import XPG_ERR_SHAPE, XPG_ERR_UNSUPPORTED, rows_equal
from tools import gen

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(3, 1, 256), (4, 2, 256), (5, 3, 256), (6, 4, 256), (9, 4, 512)]
# gen.random_system(default_rng([4242, 9, 1037]), 9, 4): chains 0 and 1 run, chain 2 needs 651 rows at its last step -- the lowest
# failing chain is above 0 (found on the CPU among 3000 candidates per shape; none at (6, 4), none inconsistent)
ABOVE_ZERO = (9, 4, [4242, 9, 1037], 512, (-651, 2, 2))


@pytest.fixture(scope="module")
def lq(ctx):
    from xpoly_amd.lineq import Lineq
    return Lineq(ctx)


def _batch(rows, nv, nb=48):
    rng = np.random.default_rng(rows * 100 + nv)
    return np.stack([gen.random_system(rng, rows, nv) for _ in range(nb)])


@pytest.fixture(scope="module")
def wants(port):
    """The chain checker's answers for the five batches, computed once: {(rows, nv): [(ok, chain, steps, bounds)]}."""
    return {(rows, nv): [bc.chains(port, m, nv, cap, cap) for m in _batch(rows, nv)] for rows, nv, cap in SHAPES}


def _same(got, want, what=""):
    ok, chain, steps, bounds = got
    for b, (wok, wchain, wsteps, wb) in enumerate(want):
        assert (ok[b], chain[b], steps[b]) == (wok, wchain, wsteps), (what, b, ok[b], chain[b], steps[b], wok, wchain, wsteps)
        assert len(bounds[b]) == len(wb) and all(rows_equal(g, w) for g, w in zip(bounds[b], wb)), (what, b)


# ---- 1. parity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,nv,cap", SHAPES)
def test_bounds_match_the_chain_checker(lq, wants, rows, nv, cap):
    got = lq.bounds_packed(_batch(rows, nv), nv, cap_rows=cap)
    route = lq.bounds_last_route()
    assert route["launches"] == 1 and route["steps"] == (nv - 1) * (nv + 2) // 2
    _same(got, wants[(rows, nv)])
    assert set(got[0].tolist()) == ({1} if nv == 1 else {0, 1})
    assert all(c == -1 and s == 0 for o, c, s in zip(*got[:3]) if o == 1)


@pytest.mark.parametrize("rows,nv,cap", SHAPES)
def test_bounds_match_the_real_reference(lq, ref, rows, nv, cap):
    """The same batches against the reference's own Lineq::fme, chain by chain, where its build is present."""
    mats = _batch(rows, nv)
    _same(lq.bounds_packed(mats, nv, cap_rows=cap), [bc.chains(ref, m, nv, cap, cap) for m in mats])


def test_a_first_failure_above_chain_zero(lq, port):
    rows, nv, seed, cap, verdict = ABOVE_ZERO
    one = gen.random_system(np.random.default_rng(seed), rows, nv)
    want = bc.chains(port, one, nv, cap, cap)
    assert want[:3] == verdict
    mats = np.stack([one] + list(_batch(rows, nv, 7)))
    _same(lq.bounds_packed(mats, nv, cap_rows=cap), [want] + [bc.chains(port, m, nv, cap, cap) for m in mats[1:]])


# ---- 2. against the chained-launch route -----------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,nv,cap", SHAPES)
def test_bounds_equal_the_chained_launch_route(lq, rows, nv, cap):
    mats = _batch(rows, nv)
    ok, chain, steps, bounds = lq.bounds_packed(mats, nv, cap_rows=cap)
    pok, pb = lq.calcBound_packed(mats, nv, cap_rows=cap)
    assert (pok >= 0).all() and np.array_equal(ok, pok)
    for b in range(len(mats)):
        assert all(rows_equal(bounds[b][j], pb[b][j]) for j in range(nv)), b


def test_golden_cases_and_the_authors_example(lq):
    ex = gen.to_rat(np.array([[-1, 0, -1], [1, 0, 4], [-1, -1, -5], [1, 1, 12]], dtype=np.int32))
    ok, chain, steps, bounds = lq.bounds_packed(ex, 2)
    assert (ok[0], chain[0], steps[0]) == (1, -1, 0)
    b1 = sorted((int(r[0][0]), int(r[2][0])) for r in bounds[0][0])
    b2 = sorted((int(r[1][0]), int(r[2][0])) for r in bounds[0][1])
    assert b1 == [(-1, -1), (1, 4)] and b2 == [(-1, -1), (1, 11)]                    # 1 <= i1 <= 4 and 1 <= i2 <= 11
    g = json.load(open(os.path.join(GOLD, "g5_lineq.json")))
    assert g["calc_bound"]
    for c in g["calc_bound"]:                                                        # outputs of the real reference
        mat = np.array(c["mat"]["data"], dtype=np.int32).reshape(tuple(c["mat"]["shape"]))
        ok, chain, steps, bounds = lq.bounds_packed(mat, c["rhs"], cap_rows=256)
        assert ok[0] == c["ok"]
        if c["ok"]:
            for j, w in enumerate(c["limits"]):
                assert rows_equal(bounds[0][j], np.array(w["data"], dtype=np.int32).reshape(tuple(w["shape"])))


# ---- 3. capacity -----------------------------------------------------------------------------------------------------------
def test_capacity_is_reported_per_chain_and_step_and_the_rest_is_packed(lq, port, wants):
    rows, nv = 9, 4
    mats = _batch(rows, nv)
    short = [bc.chains(port, m, nv, 256, 256) for m in mats]
    assert any(w[0] < 0 for w in short) and any(w[0] == 1 for w in short)
    got = lq.bounds_packed(mats, nv, cap_rows=256)
    _same(got, short, "cap 256")
    for b, w in enumerate(short):
        if w[0] < 0:
            assert -got[0][b] == bc.chain(port, mats[b], nv, w[1])[3][w[2]] > 256    # the need of that chain's step
    # once more with the largest need reported: test 1's answers
    _same(lq.bounds_packed(mats, nv, cap_rows=int(-got[0].min())), wants[(rows, nv)], "need")
    # result slots one row under the tallest result: -rows, that result's j, the length of its chain's list
    full = wants[(rows, nv)]
    tall = max(x.shape[0] for w in full if w[0] == 1 for x in w[3])
    assert tall > 1
    cap_out = tall - 1
    got3 = lq.bounds_packed(mats, nv, cap_rows=512, cap_out_rows=cap_out)
    hit = 0
    for b, w in enumerate(full):
        over = [j for j, x in enumerate(w[3]) if x.shape[0] > cap_out] if w[0] == 1 else []
        if over:
            hit += 1
            assert (got3[0][b], got3[1][b], got3[2][b]) == (-w[3][over[0]].shape[0], over[0], nv - 1), b
            assert all(x.shape[0] == 0 for x in got3[3][b]), b
        else:
            _same(tuple(x[b: b + 1] for x in got3), [w], "cap_out")
    assert hit > 0
    _same(got3, [bc.chains(port, m, nv, 512, cap_out) for m in mats], "cap_out, checker")


# ---- 4. both homes of a step's result ---------------------------------------------------------------------------------------
def test_both_homes_of_a_steps_result(lq, port, wants):
    rows, nv, cap = 9, 4, 512
    mats = _batch(rows, nv)
    cap_lds = bc.plan_view(48, rows, nv + 1, nv, cap)["cap_lds"]
    assert cap_lds < cap
    needs, prefix = [], []
    for m in mats:
        n, p = bc.step_needs(port, m, nv)
        needs += list(n.values()); prefix += p
    assert any(n <= cap_lds for n in needs) and any(cap_lds < n <= cap for n in needs), (cap_lds, sorted(needs))
    assert any(cap_lds < n <= cap for n in prefix), (cap_lds, sorted(prefix))        # a prefix built directly in the hold slot
    got = lq.bounds_packed(mats, nv, cap_rows=cap)
    assert lq.bounds_last_route()["cap_lds"] == cap_lds
    _same(got, wants[(rows, nv)])


# ---- 5. seat reuse ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,nv,cap,nb", [(6, 4, 256, 4096 + 300), (9, 4, 512, 4096 + 296)])
def test_seats_are_reused_above_the_grid(lq, wants, rows, nv, cap, nb):
    base = _batch(rows, nv)
    mats = np.ascontiguousarray(np.tile(base, (nb // 48 + 1, 1, 1, 1))[:nb])
    ok, chain, steps, bounds = lq.bounds_packed(mats, nv, cap_rows=cap, copy=False)
    route = lq.bounds_last_route()
    assert route["launches"] == 1 and route["grid"] * route["groups"] == 4096 < nb
    assert route["seat_bytes"] == bc.plan(nb, rows, nv + 1, nv, cap)["seat_bytes"] == 4096 * 3 * cap * (nv + 1) * 8
    want = wants[(rows, nv)]
    reps = nb // 48 + 1
    assert np.array_equal(ok, np.tile([w[0] for w in want], reps)[:nb]) and np.array_equal(chain, np.tile([w[1] for w in want], reps)[:nb])
    assert np.array_equal(steps, np.tile([w[2] for w in want], reps)[:nb])
    for b in range(nb):
        wb = want[b % 48][3]
        assert all(rows_equal(bounds[b][j], wb[j]) for j in range(nv)), b


# ---- 6. the device form, views, the large-output path -----------------------------------------------------------------------
def _dev_call(ctx, mats, nv, cap, cap_out):
    from xpoly_amd.lineq import bounds_dev
    nb, rows, cols = mats.shape[:3]
    d_m = ctx.malloc(max(mats.nbytes, 8)); d_o = ctx.malloc(max(nb * nv * cap_out * cols * 8, 8))
    d_r = ctx.malloc(max(nb * nv * 4, 8))
    d_k, d_c, d_s = ctx.malloc(max(nb * 4, 8)), ctx.malloc(max(nb * 4, 8)), ctx.malloc(max(nb * 4, 8))
    try:
        if nb:
            ctx.upload(d_m, mats)
        bounds_dev(ctx, nb, d_m, rows, cols, nv, cap, cap_out, d_o, d_r, d_k, d_c, d_s)
        ctx.sync()
        if not nb:
            z = np.zeros(0, dtype=np.int32)
            return z, z, z, []
        outs = ctx.download(np.zeros((nb, nv, cap_out, cols, 2), dtype=np.int32), d_o)
        r = ctx.download(np.zeros((nb, nv), dtype=np.int32), d_r)
        k, c, s = (ctx.download(np.zeros(nb, dtype=np.int32), p) for p in (d_k, d_c, d_s))
    finally:
        for p in (d_m, d_o, d_r, d_k, d_c, d_s):
            ctx.free(p)
    return k, c, s, [[outs[b, j, : r[b, j]] for j in range(nv)] for b in range(nb)]


def test_the_device_form_equals_the_host_form(ctx, lq, wants):
    rows, nv = 9, 4
    mats = _batch(rows, nv)
    host = lq.bounds_packed(mats, nv, cap_rows=512, cap_out_rows=40)
    _same(host, wants[(rows, nv)])
    for _ in range(2):                              # two calls in a row on one context
        dev = _dev_call(ctx, mats, nv, 512, 40)
        assert lq.bounds_last_route()["launches"] == 1
        assert all(np.array_equal(h, d) for h, d in zip(host[:3], dev[:3]))
        assert all(rows_equal(host[3][b][j], dev[3][b][j]) for b in range(48) for j in range(nv))
    # no systems: nothing launched, nothing written
    dev = _dev_call(ctx, mats[:0], nv, 512, 40)
    assert len(dev[0]) == 0 and lq.bounds_last_route()["launches"] == 0
    ok0, chain0, steps0, b0 = lq.bounds_packed(mats[:0], nv)
    assert len(ok0) == 0 and b0 == [] and lq.bounds_last_route()["launches"] == 0


def test_views_and_the_large_output_path(lq, wants):
    rows, nv = 6, 4
    mats = _batch(rows, nv)
    ok, chain, steps, bounds = lq.bounds_packed(mats, nv, cap_rows=64)
    _same((ok, chain, steps, bounds), wants[(rows, nv)])                             # (no step of the batch needs more than 26 rows)
    vok, vchain, vsteps, vb = lq.bounds_packed(mats, nv, cap_rows=64, copy=False)     # read before the next packed call
    assert np.array_equal(ok, vok) and all(rows_equal(bounds[b][j], vb[b][j]) for b in range(48) for j in range(nv))
    # 8 x 48 x 4 slots of 64 rows are over what comes down with the counts: scan and pack on the device, the same rows
    assert 48 * nv * 64 * (nv + 1) * 8 <= (512 << 10) < 8 * 48 * nv * 64 * (nv + 1) * 8
    big = np.ascontiguousarray(np.tile(mats, (8, 1, 1, 1)))
    bok, bchain, bsteps, bb = lq.bounds_packed(big, nv, cap_rows=64, copy=False)
    assert np.array_equal(bok, np.tile(ok, 8)) and np.array_equal(bchain, np.tile(chain, 8)) and np.array_equal(bsteps, np.tile(steps, 8))
    assert all(rows_equal(bb[b][j], bounds[b % 48][j]) for b in range(len(big)) for j in range(nv))


# ---- 7. edges ---------------------------------------------------------------------------------------------------------------
def test_edges(lq, port):
    # one variable: no step at all, the input's rows as they are -- a duplicated row included
    one = gen.to_rat(np.array([[1, 4], [-1, -1], [1, 4], [2, 9]], dtype=np.int32))
    ok, chain, steps, bounds = lq.bounds_packed(np.stack([one, one[::-1]]), 1)
    assert ok.tolist() == [1, 1] and chain.tolist() == [-1, -1] and steps.tolist() == [0, 0]
    assert np.array_equal(bounds[0][0], one) and np.array_equal(bounds[1][0], one[::-1])
    assert lq.bounds_last_route()["steps"] == 0
    # systems of zero rows only: every row is constant-true and goes, every result is empty
    zeros = gen.to_rat(np.zeros((3, 6, 5), dtype=np.int32))
    zok, zchain, zsteps, zb = lq.bounds_packed(zeros, 4)
    assert zok.tolist() == [1, 1, 1] and zchain.tolist() == [-1] * 3 and zsteps.tolist() == [0] * 3
    assert all(x.shape[0] == 0 for row in zb for x in row)
    # a constant row below zero: the first step of chain 0 -- a prefix step -- finds it
    bad = gen.to_rat(np.array([[1, 1, 0, 5], [0, 0, 0, -1], [-1, 0, 1, 3], [0, -1, -1, 2]], dtype=np.int32))
    assert bc.chains(port, bad, 3)[:3] == (0, 0, 0)
    good = gen.to_rat(np.array([[1, 1, 0, 5], [0, 0, 0, 1], [-1, 0, 1, 3], [0, -1, -1, 2]], dtype=np.int32))
    got = lq.bounds_packed(np.stack([bad, good, bad]), 3)
    _same(got, [bc.chains(port, m, 3) for m in (bad, good, bad)])
    assert got[0].tolist() == [0, 1, 0] and got[1].tolist() == [0, -1, 0] and got[2].tolist() == [0, 0, 0]


# ---- 8. argument errors -----------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(ctx, lq):
    import ctypes as C
    from xpoly_amd._capi import lib, vp, XpgError
    from xpoly_amd.lineq import bounds_dev
    mats = _batch(6, 4, 4)
    off = np.zeros(17, dtype=np.int64); ok = np.zeros(4, dtype=np.int32); ch = np.zeros(4, dtype=np.int32); st = np.zeros(4, dtype=np.int32)

    def call(rhs, cap=0, out=None, out_cap=0):
        rc = lib().xpg_lineq_bounds_batch_packed_rat32(ctx._h, C.c_int(4), vp(mats), C.c_int(6), C.c_int(5), C.c_int(rhs), C.c_int(cap), C.c_int(0),
                                                       vp(out), C.c_longlong(out_cap), None, vp(off), vp(ok), vp(ch), vp(st))
        launched = rc == 0 or (rc == XPG_ERR_SHAPE and out is not None)             # (a buffer too small is found after the launch)
        assert lq.bounds_last_route()["launches"] == (1 if launched else 0)
        return rc

    assert call(4) == 0
    assert call(0) == XPG_ERR_SHAPE and call(5) == XPG_ERR_SHAPE                    # rhs_idx outside [1, cols)
    assert call(4, cap=32768) == XPG_ERR_UNSUPPORTED                                # cap > 32767
    assert call(4, cap=4000) == XPG_ERR_UNSUPPORTED                                 # the layout of cap rows over 160 KB
    # the device form takes the caller's capacities as they are
    d = ctx.malloc(4 * 4 * 64 * 5 * 8)
    try:
        for cap, cap_out in ((0, 0), (5, 5), (64, 65)):                             # no cap_rows, cap_rows < rows, cap_out_rows > cap_rows
            with pytest.raises(XpgError, match="XPG_ERR_SHAPE"):
                bounds_dev(ctx, 4, d, 6, 5, 4, cap, cap_out, d, d, d, d, d)
            assert lq.bounds_last_route()["launches"] == 0
    finally:
        ctx.free(d)
    # a sizing call fills the offsets; a buffer one row short is refused with them (and the verdicts) filled
    assert call(4, cap=64) == 0 and off[16] > 0
    total = int(off[16])
    out = np.zeros((total, 5, 2), dtype=np.int32)
    want_ok = ok.copy()
    off[:] = 0; ok[:] = 7
    assert call(4, cap=64, out=out, out_cap=total - 1) == XPG_ERR_SHAPE
    assert off[16] == total and np.array_equal(ok, want_ok)
    assert call(4, cap=64, out=out, out_cap=total) == 0
    _, _, _, res = lq.bounds_packed(mats, 4, cap_rows=64)
    assert all(rows_equal(out[off[b * 4 + j]: off[b * 4 + j + 1]], res[b][j]) for b in range(4) for j in range(4))


# ---- the collector ------------------------------------------------------------------------------------------------------------
def test_the_collector_bounds_three_shape_classes(port, tmp_path):
    """tests/cxx/calc_bound_all.cpp in a child process: systems of three shapes, interleaved, through xpoly_amd::calc_bound_all,
    each checked in there against Lineq::calcBound of the adapter on the single system. A step of the 9 x 5 class needs more
    rows than the first capacity tried (4 rows + 16): the collector calls again with the need reported."""
    from test_lineq_bounds_host import build_collector
    exe = build_collector()
    classes = ((4, 2), (6, 4), (9, 4))
    rngs = [np.random.default_rng(rows * 100 + nv) for rows, nv in classes]
    systems = []
    for k in range(8):
        for (rows, nv), rng in zip(classes, rngs):
            m = rng.integers(-3, 4, size=(rows, nv + 1)) * (rng.random((rows, nv + 1)) < 0.7)
            m[:, nv] = rng.integers(-2, 9, size=rows)
            systems.append((m.astype(np.int32), nv))
    needs = [n for m, nv in systems if m.shape[0] == 9 for n in bc.step_needs(port, gen.to_rat(m), nv)[0].values()]
    assert max(needs) > 4 * 9 + 16                             # over the first capacity of the 9-row class: a second call
    lines = ["%d" % len(systems)]
    for m, nv in systems:
        lines += ["%d %d %d" % (m.shape[0], m.shape[1], nv), " ".join(str(int(x)) for x in m.ravel())]
    path = str(tmp_path / "systems.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert out[0] == "rc 0" and "mismatches 0" in out
    verdicts = {ln.split()[2] for ln in out if " ok " in ln}
    assert len([ln for ln in out if " ok " in ln]) == len(systems) and verdicts == {"0", "1"}, verdicts
