"""GPU parity of the projection entry points (xpg_lineq_project_batch_*: a list of variables eliminated in ONE launch of
k_fme_chain_batch) against the CPU checker's fme applied step after step (tests/lineq_project_cases.py stepped), and against
the product's own single-step Lineq.fme chained in Python -- k_fme_batch, which runs the same step (w_fme_step) once per launch.
Bit-exact: nothing is compared with a tolerance."""
import os
import subprocess

import numpy as np
import pytest

import lineq_project_cases as pc
from lineq_project_cases import XPG_ERR_SHAPE, XPG_ERR_UNSUPPORTED, rows_equal
from tools import gen

pytestmark = pytest.mark.gpu

PARITY = [(4, 2, [1]), (6, 4, [3, 2]), (9, 4, [3, 2, 1])]


@pytest.fixture(scope="module")
def lq(ctx):
    from xpoly_amd.lineq import Lineq
    return Lineq(ctx)


def _batch(rows, nv, nb, seed=None):
    rng = np.random.default_rng(rows * 100 + nv if seed is None else seed)
    return np.stack([gen.random_system(rng, rows, nv) for _ in range(nb)])


def _chained(lq, mats, nv, elim, dark=False):
    """The product's single-step fme, step after step: (ok[nb], steps[nb], [rows]). Each step is one ragged call over the
    systems still alive and not empty; an empty system stays empty (fme of an empty system is true and empty)."""
    nb = len(mats)
    cur = [np.asarray(m) for m in mats]
    ok = np.ones(nb, dtype=np.int32); steps = np.full(nb, len(elim), dtype=np.int32)
    for k, u in enumerate(elim):
        alive = [b for b in range(nb) if ok[b] == 1 and cur[b].shape[0] > 0]
        if not alive:
            break
        sok, res = lq.fme_ragged([cur[b] for b in alive], [u] * len(alive), [nv] * len(alive), dark)
        for b, o, r in zip(alive, sok, res):
            if o:
                cur[b] = r
            else:
                ok[b] = 0; steps[b] = k; cur[b] = r[:0]
    return ok, steps, [cur[b] if ok[b] == 1 else cur[b][:0] for b in range(nb)]


@pytest.fixture(scope="module")
def wants(port):
    """The stepped checker's answers for the parity batches, computed once: {(rows, nv, dark): [(ok, steps, rows, needs)]}."""
    out = {}
    for rows, nv, elim in PARITY:
        mats = _batch(rows, nv, 48)
        for dark in (False, True):
            out[(rows, nv, dark)] = [pc.stepped(port, mats[b], nv, elim, dark, cap_rows=256) for b in range(48)]
    return out


@pytest.mark.parametrize("rows,nv,elim", PARITY)
def test_projection_matches_the_stepped_checker(lq, wants, rows, nv, elim):
    mats = _batch(rows, nv, 48)
    verdicts, stops = set(), set()
    for dark in (False, True):
        ok, steps, res = lq.project_packed(mats, nv, elim, dark, cap_rows=256)
        assert lq.project_last_route()["launches"] == 1
        for b, (wok, wsteps, wrows, _) in enumerate(wants[(rows, nv, dark)]):
            assert (ok[b], steps[b]) == (wok, wsteps), (dark, b, ok[b], steps[b], wok, wsteps)
            assert rows_equal(res[b], wrows), (dark, b)
            verdicts.add(int(ok[b])); stops.add(int(steps[b]))
    assert verdicts == {0, 1}, verdicts
    if len(elim) > 1:
        assert len(stops) > 1, stops
    else:
        assert stops == {0, 1}, stops               # one step: it either says inconsistent (0) or completes (1)


@pytest.mark.parametrize("rows,nv,elim", PARITY)
def test_projection_matches_the_real_reference(lq, ref, rows, nv, elim):
    """The same batches against the reference's own Lineq::fme, step after step, where its build is present."""
    mats = _batch(rows, nv, 48)
    for dark in (False, True):
        ok, steps, res = lq.project_packed(mats, nv, elim, dark, cap_rows=256)
        for b in range(48):
            wok, wsteps, wrows, _ = pc.stepped(ref, mats[b], nv, elim, dark, cap_rows=256)
            assert (ok[b], steps[b]) == (wok, wsteps) and rows_equal(res[b], wrows), (dark, b)


def test_chains_stop_at_every_step_index(lq, wants):
    """The kernel's own steps: inconsistent at step 0, 1 and 2, and chains that run to the end, in one batch."""
    mats = _batch(9, 4, 48)
    for dark in (False, True):
        ok, steps, _ = lq.project_packed(mats, 4, [3, 2, 1], dark, cap_rows=256)
        assert {int(s) for s in steps} == {0, 1, 2, 3}, steps
        assert {int(s) for s, o in zip(steps, ok) if o == 0} == {0, 1, 2} and {int(s) for s, o in zip(steps, ok) if o == 1} == {3}
        assert steps.tolist() == [w[1] for w in wants[(9, 4, dark)]]


@pytest.mark.parametrize("rows,nv,elim", PARITY)
def test_one_statement_of_the_step(lq, rows, nv, elim):
    """A chain in one launch against the step on its own: the same batches through single-step fme calls (k_fme_batch) chained
    in Python."""
    mats = _batch(rows, nv, 48)
    for dark in (False, True):
        ok, steps, res = lq.project_packed(mats, nv, elim, dark, cap_rows=256)
        cok, csteps, cres = _chained(lq, mats, nv, elim, dark)
        assert np.array_equal(ok, cok) and np.array_equal(steps, csteps), (dark, ok, cok, steps, csteps)
        assert all(rows_equal(res[b], cres[b]) for b in range(48)), dark


def test_a_single_step_equals_fme_packed(lq):
    mats = _batch(9, 4, 48)
    for dark in (False, True):
        fok, foff, frows = lq.fme_packed(mats, 4, 3, dark, cap_rows=256)
        for elim in ([3], [3, 3]):                  # a repeated index finds no row with u and copies
            ok, steps, res = lq.project_packed(mats, 4, elim, dark, cap_rows=256)
            assert np.array_equal(ok, fok), (elim, dark)
            for b in range(48):
                want = frows[foff[b]: foff[b + 1]] if fok[b] else frows[:0]
                assert rows_equal(res[b], want), (elim, dark, b)
                assert steps[b] == (len(elim) if fok[b] else 0), (elim, dark, b, steps[b])


# ---- both homes of a step's result, and capacity ---------------------------------------------------------------------------
HOMES = (12, 6, [5, 4], 8)


@pytest.fixture(scope="module")
def homes(port):
    rows, nv, elim, nb = HOMES
    mats = _batch(rows, nv, nb)
    return mats, [pc.stepped(port, mats[b], nv, elim) for b in range(nb)]


def _homes_cap(needs):
    """A cap_rows that holds every step of the batch and whose LDS result area does not: above the 12 KB layout."""
    cap = max(128, max(needs))
    p = pc.plan_view(HOMES[3], HOMES[0], HOMES[1] + 1, cap)
    assert p["cap_lds"] < cap, p
    return cap, p["cap_lds"]


def test_both_homes_of_a_steps_result(lq, homes):
    rows, nv, elim, nb = HOMES
    mats, want = homes
    needs = [n for w in want for n in w[3] if n is not None]
    cap, cap_lds = _homes_cap(needs)
    assert any(n <= cap_lds for n in needs) and any(n > cap_lds for n in needs), (cap_lds, sorted(needs))
    ok, steps, res = lq.project_packed(mats, nv, elim, cap_rows=cap)
    assert lq.project_last_route()["cap_lds"] == cap_lds
    for b, (wok, wsteps, wrows, _) in enumerate(want):
        assert (ok[b], steps[b]) == (wok, wsteps), (b, ok[b], steps[b], wok, wsteps)
        assert rows_equal(res[b], wrows), b


def test_capacity_is_reported_per_step_and_the_rest_is_packed(lq, port, homes):
    rows, nv, elim, nb = HOMES
    mats, want = homes
    needs = [n for w in want for n in w[3] if n is not None]
    cap = max(needs) - 1
    assert cap >= rows
    short = [pc.stepped(port, mats[b], nv, elim, cap_rows=cap) for b in range(nb)]
    assert any(w[0] < 0 for w in short) and any(w[0] == 1 for w in short)
    ok, steps, res = lq.project_packed(mats, nv, elim, cap_rows=cap)
    for b, (wok, wsteps, wrows, wneeds) in enumerate(short):
        assert (ok[b], steps[b]) == (wok, wsteps), (b, ok[b], steps[b], wok, wsteps)
        assert rows_equal(res[b], wrows), b
        if wok < 0:
            assert -ok[b] == wneeds[wsteps] > cap
    # once more with the largest need reported: every step fits
    ok2, steps2, res2 = lq.project_packed(mats, nv, elim, cap_rows=int(-ok.min()))
    for b, (wok, wsteps, wrows, _) in enumerate(want):
        assert (ok2[b], steps2[b]) == (wok, wsteps) and rows_equal(res2[b], wrows), b
    # final slots smaller than a final result: -rows with steps == n_elim, the others packed
    final = [w[2].shape[0] for w in want if w[0] == 1]
    assert max(final) > 1
    cap_out = max(final) - 1
    ok3, steps3, res3 = lq.project_packed(mats, nv, elim, cap_rows=max(needs), cap_out_rows=cap_out)
    for b, (wok, wsteps, wrows, _) in enumerate(want):
        if wok == 1 and wrows.shape[0] > cap_out:
            assert ok3[b] == -wrows.shape[0] and steps3[b] == len(elim) and res3[b].shape[0] == 0, b
        else:
            assert (ok3[b], steps3[b]) == (wok, wsteps) and rows_equal(res3[b], wrows), b


def test_seats_are_reused_above_the_grid(lq):
    rows, nv, elim = 6, 4, [3, 2]
    base = _batch(rows, nv, 64)
    cok, csteps, cres = _chained(lq, base, nv, elim)
    seat_bytes = []
    for nb in (4096 + 300, 4096 + 1000):
        mats = np.ascontiguousarray(np.tile(base, (nb // 64 + 1, 1, 1, 1))[:nb])
        ok, steps, res = lq.project_packed(mats, nv, elim, cap_rows=256)
        route = lq.project_last_route()
        assert route["launches"] == 1 and nb > route["grid"] * route["groups"] == 4096 * route["groups"]
        seat_bytes.append(route["seat_bytes"])
        assert np.array_equal(ok, np.tile(cok, nb // 64 + 1)[:nb]) and np.array_equal(steps, np.tile(csteps, nb // 64 + 1)[:nb])
        assert all(rows_equal(res[b], cres[b % 64]) for b in range(nb))
    assert seat_bytes[0] == seat_bytes[1] == pc.plan(5000, rows, nv + 1, 256)["seat_bytes"]


def test_device_slots_of_a_seat_are_reused(lq, homes):
    """The 12 x 7 batch whose steps land in the seats' device slots as well as in LDS, tiled above the grid: a seat takes a
    second system and builds its steps in the slots the first one left."""
    rows, nv, elim, nb0 = HOMES
    mats, want = homes
    needs = [n for w in want for n in w[3] if n is not None]
    cap, cap_lds = _homes_cap(needs)
    assert sum(n > cap_lds for n in needs) >= nb0                                     # device slots are the common case here
    nb = 4096 + 8 * 37
    big = np.ascontiguousarray(np.tile(mats, (nb // nb0, 1, 1, 1)))
    ok, steps, res = lq.project_packed(big, nv, elim, cap_rows=cap)
    route = lq.project_last_route()
    assert route["launches"] == 1 and route["grid"] * route["groups"] == 4096 < nb and route["cap_lds"] == cap_lds
    assert route["seat_bytes"] == 4096 * 2 * cap * (nv + 1) * 8
    for b in range(nb):
        wok, wsteps, wrows, _ = want[b % nb0]
        assert (ok[b], steps[b]) == (wok, wsteps) and rows_equal(res[b], wrows), b


def _dev_call(ctx, mats, nv, elim, cap, cap_out, dark=False):
    from xpoly_amd.lineq import project_dev
    nb, rows, cols = mats.shape[:3]
    d_m = ctx.malloc(max(mats.nbytes, 8)); d_o = ctx.malloc(max(nb * cap_out * cols * 8, 8))
    d_r, d_k, d_s = ctx.malloc(max(nb * 4, 8)), ctx.malloc(max(nb * 4, 8)), ctx.malloc(max(nb * 4, 8))
    try:
        if nb:
            ctx.upload(d_m, mats)
        project_dev(ctx, nb, d_m, rows, cols, nv, elim, dark, cap, cap_out, d_o, d_r, d_k, d_s)
        ctx.sync()
        outs = ctx.download(np.zeros((nb, cap_out, cols, 2), dtype=np.int32), d_o) if nb else np.zeros((0, cap_out, cols, 2), dtype=np.int32)
        r, k, s = (ctx.download(np.zeros(nb, dtype=np.int32), p) if nb else np.zeros(0, dtype=np.int32) for p in (d_r, d_k, d_s))
    finally:
        for p in (d_m, d_o, d_r, d_k, d_s):
            ctx.free(p)
    return k, s, [outs[b, : r[b]] for b in range(nb)]


def test_the_device_form_equals_the_host_form(ctx, lq):
    rows, nv, elim = 9, 4, [3, 2, 1]
    mats = _batch(rows, nv, 48)
    ok, steps, res = lq.project_packed(mats, nv, elim, cap_rows=256, cap_out_rows=40)
    for _ in range(2):                              # two calls in a row on one context
        dok, dsteps, dres = _dev_call(ctx, mats, nv, elim, 256, 40)
        assert lq.project_last_route()["launches"] == 1
        assert np.array_equal(ok, dok) and np.array_equal(steps, dsteps)
        assert all(rows_equal(res[b], dres[b]) for b in range(48))
    # no systems: nothing launched, nothing written
    dok, dsteps, dres = _dev_call(ctx, mats[:0], nv, elim, 256, 40)
    assert len(dok) == 0 and lq.project_last_route()["launches"] == 0
    ok0, steps0, res0 = lq.project_packed(mats[:0], nv, elim)
    assert len(ok0) == 0 and res0 == []


def test_views_and_empty_systems(lq):
    rows, nv, elim = 6, 4, [3, 2]
    mats = _batch(rows, nv, 48)
    ok, steps, res = lq.project_packed(mats, nv, elim, cap_rows=64)
    vok, vsteps, vres = lq.project_packed(mats, nv, elim, cap_rows=64, copy=False)        # read before the next packed call
    assert np.array_equal(ok, vok) and all(rows_equal(res[b], vres[b]) for b in range(48))
    # the large-output path (scan and pack on the device) gives the same rows as the small one
    big = np.ascontiguousarray(np.tile(mats, (8, 1, 1, 1)))
    bok, bsteps, bres = lq.project_packed(big, nv, elim, cap_rows=64, copy=False)
    assert np.array_equal(bok, np.tile(ok, 8)) and all(rows_equal(bres[b], res[b % 48]) for b in range(len(big)))
    # systems of zero rows only: every row is constant-true and goes, the empty intermediate is carried to the end
    zeros = gen.to_rat(np.zeros((3, rows, nv + 1), dtype=np.int32))
    zok, zsteps, zres = lq.project_packed(zeros, nv, elim)
    assert zok.tolist() == [1, 1, 1] and zsteps.tolist() == [2, 2, 2] and all(r.shape[0] == 0 for r in zres)


def test_shape_errors_launch_nothing(ctx, lq):
    import ctypes as C
    from xpoly_amd._capi import lib, vp
    mats = _batch(6, 4, 4)
    off = np.zeros(5, dtype=np.int64); ok = np.zeros(4, dtype=np.int32); steps = np.zeros(4, dtype=np.int32)

    def call(rhs, elim, cap=0):
        el = np.asarray(elim, dtype=np.int32)
        rc = lib().xpg_lineq_project_batch_packed_rat32(ctx._h, C.c_int(4), vp(mats), C.c_int(6), C.c_int(5), C.c_int(rhs), vp(el),
                                                        C.c_int(len(el)), C.c_int(0), C.c_int(cap), C.c_int(0), None, C.c_longlong(0), None,
                                                        vp(off), vp(ok), vp(steps))
        assert lq.project_last_route()["launches"] == (1 if rc == 0 else 0)
        return rc

    assert call(4, [3, 2]) == 0
    assert call(4, np.zeros(0, dtype=np.int32)) == XPG_ERR_SHAPE                    # n_elim <= 0
    assert call(4, [4]) == XPG_ERR_SHAPE and call(4, [3, -1]) == XPG_ERR_SHAPE      # an index outside [0, rhs_idx)
    assert call(0, [0]) == XPG_ERR_SHAPE and call(5, [3]) == XPG_ERR_SHAPE          # rhs_idx outside [1, cols)
    assert call(4, [3], cap=32768) == XPG_ERR_UNSUPPORTED                           # cap > 32767
    assert call(4, [3], cap=4000) == XPG_ERR_UNSUPPORTED                            # the layout of cap rows over 160 KB
    assert call(4, [3] * (pc.CHAIN_MAX + 1)) == XPG_ERR_UNSUPPORTED and call(4, [3] * pc.CHAIN_MAX) == 0
    # the device form takes the caller's capacities as they are: none is defaulted or clamped behind d_outs' row stride
    from xpoly_amd._capi import XpgError
    from xpoly_amd.lineq import project_dev
    d = ctx.malloc(4 * 64 * 5 * 8)
    try:
        for cap, cap_out in ((0, 0), (5, 5), (64, 65)):                             # no cap_rows, cap_rows < rows, cap_out_rows > cap_rows
            with pytest.raises(XpgError, match="XPG_ERR_SHAPE"):
                project_dev(ctx, 4, d, 6, 5, 4, [3, 2], False, cap, cap_out, d, d, d, d)
            assert lq.project_last_route()["launches"] == 0
    finally:
        ctx.free(d)
    # a sizing call fills the offsets; a buffer one row short is refused with them filled
    assert call(4, [3, 2], cap=64) == 0 and off[4] > 0
    total = int(off[4])
    out = np.zeros((total, 5, 2), dtype=np.int32)
    el = np.array([3, 2], dtype=np.int32)
    args = (ctx._h, C.c_int(4), vp(mats), C.c_int(6), C.c_int(5), C.c_int(4), vp(el), C.c_int(2), C.c_int(0), C.c_int(64), C.c_int(0))
    off[:] = 0
    assert lib().xpg_lineq_project_batch_packed_rat32(*args, vp(out), C.c_longlong(total - 1), None, vp(off), vp(ok), vp(steps)) == XPG_ERR_SHAPE
    assert off[4] == total
    assert lib().xpg_lineq_project_batch_packed_rat32(*args, vp(out), C.c_longlong(total), None, vp(off), vp(ok), vp(steps)) == 0
    _, _, res = lq.project_packed(mats, 4, [3, 2], cap_rows=64)
    assert all(rows_equal(out[off[b]: off[b + 1]], res[b]) for b in range(4))


def test_the_collector_projects_three_shape_classes(port, tmp_path):
    """tests/cxx/project_all.cpp in a child process: systems of three shapes, interleaved, through xpoly_amd::project_all, each
    checked in there against Lineq::fme of the adapter, variable after variable. The 12 x 7 class needs more rows than the
    first capacity tried: the collector calls again with the need reported."""
    from test_lineq_project_host import build_collector
    exe = build_collector()
    nv, elim = 6, [5, 4]
    rng = np.random.default_rng(77)
    systems = []
    for k in range(8):
        for rows in (5, 8, 12):
            m = rng.integers(-3, 4, size=(rows, nv + 1)) * (rng.random((rows, nv + 1)) < 0.7)
            m[:, nv] = rng.integers(-2, 9, size=rows)
            systems.append(m.astype(np.int32))
    needs = [n for m in systems for n in pc.stepped(port, gen.to_rat(m), nv, elim)[3] if n is not None]
    assert max(needs) > 12 * 12 // 4 + 12 + 1                  # over the default capacity of the 12-row class: a second call
    lines = ["%d %d %d" % (nv, len(elim), len(systems)), " ".join(map(str, elim))]
    for m in systems:
        lines += ["%d %d" % m.shape, " ".join(str(int(x)) for x in m.ravel())]
    path = str(tmp_path / "systems.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert out[0] == "rc 0" and "mismatches 0" in out
    verdicts = {ln.split()[2] for ln in out if " ok " in ln}
    assert len([ln for ln in out if " ok " in ln]) == len(systems) and verdicts == {"0", "1"}, verdicts
