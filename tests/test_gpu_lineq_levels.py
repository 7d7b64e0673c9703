"""GPU parity of the levels entry points (xpg_lineq_levels_batch_*: a projection that keeps the rows after EVERY step, one
launch of k_fme_levels_batch) against the CPU checker's fme applied step after step with every intermediate recorded
(tests/lineq_levels_cases.py stepped_levels), against the real reference where its build is present, and against the
product's own projection and single-step fme. The batches are tests/test_gpu_lineq_project.py's. Bit-exact: nothing is
compared with a tolerance."""
import subprocess

import numpy as np
import pytest

import lineq_levels_cases as lc
import lineq_project_cases as pc
from lineq_levels_cases import XPG_ERR_SHAPE, XPG_ERR_UNSUPPORTED, rows_equal, stepped_levels
from tools import gen

pytestmark = pytest.mark.gpu

PARITY = [(4, 2, [1]), (6, 4, [3, 2]), (9, 4, [3, 2, 1])]
HOMES = (12, 6, [5, 4], 8)


@pytest.fixture(scope="module")
def lq(ctx):
    from xpoly_amd.lineq import Lineq
    return Lineq(ctx)


def _batch(rows, nv, nb, seed=None):
    rng = np.random.default_rng(rows * 100 + nv if seed is None else seed)
    return np.stack([gen.random_system(rng, rows, nv) for _ in range(nb)])


def _cap_out(nb, rows, nv, n_elim, cap_rows, cap_out_rows=0):
    """The cap_out_rows a call settles on (host-only plan view)."""
    return lc.plan_view(nb, rows, nv + 1, n_elim, cap_rows, cap_out_rows)["cap_out"]


def _check(got, want, tag=()):
    """(ok, steps, levels) of a call against [(ok, steps, levels, ...)] of the checker, system by system, level by level."""
    ok, steps, levels = got
    assert len(ok) == len(want)
    for b, w in enumerate(want):
        assert (ok[b], steps[b]) == (w[0], w[1]), tag + (b, ok[b], steps[b], w[0], w[1])
        assert len(levels[b]) == len(w[2])
        for k, wl in enumerate(w[2]):
            assert rows_equal(levels[b][k], wl), tag + (b, k)
        if w[0] <= 0:                                    # a failed system: 0 rows at EVERY level, those before its step too
            assert all(lv.shape[0] == 0 for lv in levels[b]), tag + (b,)


@pytest.fixture(scope="module")
def wants(port):
    """The stepped checker's answers for the parity batches, computed once: {(rows, nv, dark): [(ok, steps, levels, needs, sizes)]}."""
    out = {}
    for rows, nv, elim in PARITY:
        mats = _batch(rows, nv, 48)
        cap_out = _cap_out(48, rows, nv, len(elim), 256)
        for dark in (False, True):
            out[(rows, nv, dark)] = [stepped_levels(port, mats[b], nv, elim, dark, cap_rows=256, cap_out_rows=cap_out) for b in range(48)]
    return out


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,nv,elim", PARITY)
def test_every_level_matches_the_stepped_checker(lq, wants, rows, nv, elim):
    mats = _batch(rows, nv, 48)
    verdicts, stops = set(), set()
    for dark in (False, True):
        got = lq.levels_packed(mats, nv, elim, dark, cap_rows=256)
        assert lq.levels_last_route()["launches"] == 1
        _check(got, wants[(rows, nv, dark)], (dark,))
        verdicts |= {int(v) for v in got[0]}; stops |= {int(s) for s in got[1]}
        # a system that failed after its first step HAD rows at the levels before: they are gone all the same
        if rows == 9:
            assert any(w[0] == 0 and w[1] > 0 and w[4] and w[4][0] > 0 for w in wants[(rows, nv, dark)])
    assert verdicts == {0, 1}, verdicts
    if rows == 9:
        assert stops == {0, 1, 2, 3}, stops


@pytest.mark.parametrize("rows,nv,elim", PARITY)
def test_every_level_matches_the_real_reference(lq, ref, rows, nv, elim):
    """The same batches against the reference's own Lineq::fme, step after step, where its build is present."""
    mats = _batch(rows, nv, 48)
    cap_out = _cap_out(48, rows, nv, len(elim), 256)
    for dark in (False, True):
        got = lq.levels_packed(mats, nv, elim, dark, cap_rows=256)
        assert lq.levels_last_route()["launches"] == 1
        _check(got, [stepped_levels(ref, mats[b], nv, elim, dark, cap_rows=256, cap_out_rows=cap_out) for b in range(48)], (dark,))


# ---- 2. the last level is the projection ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,nv,elim", PARITY)
def test_the_last_level_is_the_projection(lq, rows, nv, elim):
    mats = _batch(rows, nv, 48)
    for dark in (False, True):
        pok, psteps, pres = lq.project_packed(mats, nv, elim, dark, cap_rows=256)
        ok, steps, levels = lq.levels_packed(mats, nv, elim, dark, cap_rows=256, cap_out_rows=256)
        assert np.array_equal(ok, pok) and np.array_equal(steps, psteps), (dark, ok, pok, steps, psteps)
        assert all(rows_equal(levels[b][-1], pres[b]) for b in range(48)), dark


def test_a_single_step_equals_fme_packed_and_a_repeated_index_copies(lq):
    mats = _batch(9, 4, 48)
    for dark in (False, True):
        fok, foff, frows = lq.fme_packed(mats, 4, 3, dark, cap_rows=256)
        for elim in ([3], [3, 3]):                  # a repeated index finds no row with u and copies
            ok, steps, levels = lq.levels_packed(mats, 4, elim, dark, cap_rows=256, cap_out_rows=256)
            assert np.array_equal(ok, fok), (elim, dark)
            for b in range(48):
                want = frows[foff[b]: foff[b + 1]] if fok[b] else frows[:0]
                assert all(rows_equal(lv, want) for lv in levels[b]), (elim, dark, b)
                assert steps[b] == (len(elim) if fok[b] else 0), (elim, dark, b, steps[b])


# ---- 3. both homes of a level --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def homes(port):
    rows, nv, elim, nb = HOMES
    mats = _batch(rows, nv, nb)
    return mats, [stepped_levels(port, mats[b], nv, elim) for b in range(nb)]


def _homes_cap(needs):
    """A cap_rows that holds every step of the batch and whose LDS result area does not: above the 12 KB layout."""
    cap = max(128, max(needs))
    p = lc.plan_view(HOMES[3], HOMES[0], HOMES[1] + 1, len(HOMES[2]), cap, cap)
    assert p["cap_lds"] < cap, p
    return cap, p["cap_lds"]


def test_levels_are_stored_from_lds_and_from_a_device_side(lq, homes):
    rows, nv, elim, nb = HOMES
    mats, want = homes
    needs = [n for w in want for n in w[3] if n is not None]
    cap, cap_lds = _homes_cap(needs)
    # the steps whose level is STORED: those of the systems that end well, with rows
    stored = [w[3][k] for w in want if w[0] == 1 for k in range(len(w[4])) if w[4][k] > 0]
    assert any(n <= cap_lds for n in stored) and any(n > cap_lds for n in stored), (cap_lds, sorted(stored))
    got = lq.levels_packed(mats, nv, elim, cap_rows=cap, cap_out_rows=cap)
    assert lq.levels_last_route()["cap_lds"] == cap_lds
    _check(got, want)


# ---- 4. capacities ---------------------------------------------------------------------------------------------------------------
def test_a_short_cap_rows_is_reported_with_its_step_and_the_rest_is_packed(lq, port, homes):
    rows, nv, elim, nb = HOMES
    mats, want = homes
    needs = [n for w in want for n in w[3] if n is not None]
    cap = max(needs) - 1
    assert cap >= rows
    short = [stepped_levels(port, mats[b], nv, elim, cap_rows=cap) for b in range(nb)]
    assert any(w[0] < 0 for w in short) and any(w[0] == 1 for w in short)
    got = lq.levels_packed(mats, nv, elim, cap_rows=cap, cap_out_rows=cap)
    _check(got, short)
    for b, w in enumerate(short):
        if w[0] < 0:
            assert -got[0][b] == w[3][w[1]] > cap
    # once more with the largest need reported: every step fits
    need = int(-got[0].min())
    _check(lq.levels_packed(mats, nv, elim, cap_rows=need, cap_out_rows=need), want)


def test_a_short_level_slot_is_reported_at_an_intermediate_step(lq, port, homes):
    rows, nv, elim, nb = HOMES
    mats, want = homes
    needs = [n for w in want for n in w[3] if n is not None]
    cap = max(needs)
    step = 0                                        # an intermediate step, not the last one (chosen here, on the CPU)
    assert step < len(elim) - 1
    sizes = [w[4][step] for w in want if len(w[4]) > step]
    cap_out = max(sizes) - 1
    assert cap_out >= 1
    short = [stepped_levels(port, mats[b], nv, elim, cap_rows=cap, cap_out_rows=cap_out) for b in range(nb)]
    hit = [b for b, w in enumerate(short) if w[0] < 0 and w[1] == step]
    assert hit and any(w[0] == 1 and any(lv.shape[0] for lv in w[2]) for w in short)
    got = lq.levels_packed(mats, nv, elim, cap_rows=cap, cap_out_rows=cap_out)
    _check(got, short)
    for b in hit:                                   # -rows, with cap_out_rows < rows <= cap_rows: the level, not the step
        assert cap_out < -got[0][b] <= cap and -got[0][b] == want[b][4][step] and got[1][b] == step


# ---- 5. seat and slot reuse ------------------------------------------------------------------------------------------------------
def test_seats_and_level_slots_above_the_grid(lq, port):
    rows, nv, elim = 6, 4, [3, 2]
    base = _batch(rows, nv, 64)
    nb = 4096 + 300
    cap_out = _cap_out(nb, rows, nv, len(elim), 256)
    want = [stepped_levels(port, base[b], nv, elim, cap_rows=256, cap_out_rows=cap_out) for b in range(64)]
    assert {w[0] for w in want} == {0, 1}
    mats = np.ascontiguousarray(np.tile(base, (nb // 64 + 1, 1, 1, 1))[:nb])
    ok, steps, levels = lq.levels_packed(mats, nv, elim, cap_rows=256)
    route = lq.levels_last_route()
    planned = lc.plan(nb, rows, nv + 1, len(elim), 256)
    assert route == {k: planned[k] for k in lc.PLAN_KEYS[:7]}, (route, planned)
    assert route["launches"] == 1 and nb > route["grid"] * route["groups"] == 4096 * route["groups"]
    assert route["level_bytes"] == nb * len(elim) * cap_out * (nv + 1) * 8
    # the seats do not follow nb; the level slots do
    other = lc.plan_view(4096 + 1000, rows, nv + 1, len(elim), 256)                   # the library's own plan of a larger batch
    assert other["seat_bytes"] == route["seat_bytes"] and other["level_bytes"] > route["level_bytes"]
    for b in range(nb):
        w = want[b % 64]
        assert (ok[b], steps[b]) == (w[0], w[1]), b
        assert all(rows_equal(levels[b][k], w[2][k]) for k in range(len(elim))), b


def test_empty_intermediates(lq):
    rows, nv, elim = 6, 4, [3, 2]
    zeros = gen.to_rat(np.zeros((3, rows, nv + 1), dtype=np.int32))
    ok, steps, levels = lq.levels_packed(zeros, nv, elim)
    assert ok.tolist() == [1, 1, 1] and steps.tolist() == [2, 2, 2]
    assert all(lv.shape[0] == 0 for b in range(3) for lv in levels[b])
    # views: read before the next packed call
    mats = _batch(rows, nv, 48)
    a = lq.levels_packed(mats, nv, elim, cap_rows=64)
    v = lq.levels_packed(mats, nv, elim, cap_rows=64, copy=False)
    assert np.array_equal(a[0], v[0]) and all(rows_equal(a[2][b][k], v[2][b][k]) for b in range(48) for k in range(2))


# ---- 6. device form --------------------------------------------------------------------------------------------------------------
def _dev_call(ctx, mats, nv, elim, cap, cap_out, dark=False):
    from xpoly_amd.lineq import levels_dev
    nb, rows, cols = mats.shape[:3]
    n = len(elim)
    d_m = ctx.malloc(max(mats.nbytes, 8)); d_o = ctx.malloc(max(nb * n * cap_out * cols * 8, 8))
    d_r, d_k, d_s = ctx.malloc(max(nb * n * 4, 8)), ctx.malloc(max(nb * 4, 8)), ctx.malloc(max(nb * 4, 8))
    try:
        if nb:
            ctx.upload(d_m, mats)
        levels_dev(ctx, nb, d_m, rows, cols, nv, elim, dark, cap, cap_out, d_o, d_r, d_k, d_s)
        ctx.sync()
        if nb:
            outs = ctx.download(np.zeros((nb, n, cap_out, cols, 2), dtype=np.int32), d_o)
            r = ctx.download(np.zeros((nb, n), dtype=np.int32), d_r)
            k, s = (ctx.download(np.zeros(nb, dtype=np.int32), p) for p in (d_k, d_s))
        else:
            outs = np.zeros((0, n, cap_out, cols, 2), dtype=np.int32); r = np.zeros((0, n), dtype=np.int32)
            k = s = np.zeros(0, dtype=np.int32)
    finally:
        for p in (d_m, d_o, d_r, d_k, d_s):
            ctx.free(p)
    assert (r >= 0).all() and (r <= cap_out).all()
    return k, s, [[outs[b, j, : r[b, j]] for j in range(n)] for b in range(nb)]


def test_the_device_form_equals_the_host_form(ctx, lq):
    rows, nv, elim = 9, 4, [3, 2, 1]
    mats = _batch(rows, nv, 48)
    ok, steps, levels = lq.levels_packed(mats, nv, elim, cap_rows=256, cap_out_rows=40)
    for _ in range(2):                              # two calls in a row on one context
        dok, dsteps, dlev = _dev_call(ctx, mats, nv, elim, 256, 40)
        assert lq.levels_last_route()["launches"] == 1
        assert np.array_equal(ok, dok) and np.array_equal(steps, dsteps)
        assert all(rows_equal(levels[b][k], dlev[b][k]) for b in range(48) for k in range(3))
    # no systems: nothing launched, nothing written
    dok, dsteps, dlev = _dev_call(ctx, mats[:0], nv, elim, 256, 40)
    assert len(dok) == 0 and lq.levels_last_route()["launches"] == 0
    ok0, steps0, lev0 = lq.levels_packed(mats[:0], nv, elim)
    assert len(ok0) == 0 and lev0 == []


def test_shape_errors_launch_nothing(ctx, lq):
    import ctypes as C
    from xpoly_amd._capi import XpgError, lib, vp
    from xpoly_amd.lineq import levels_dev
    mats = _batch(6, 4, 4)
    off = np.zeros(4 * 64 + 1, dtype=np.int64); ok = np.zeros(4, dtype=np.int32); steps = np.zeros(4, dtype=np.int32)

    def call(rhs, elim, cap=0):
        el = np.asarray(elim, dtype=np.int32)
        rc = lib().xpg_lineq_levels_batch_packed_rat32(ctx._h, C.c_int(4), vp(mats), C.c_int(6), C.c_int(5), C.c_int(rhs), vp(el),
                                                       C.c_int(len(el)), C.c_int(0), C.c_int(cap), C.c_int(0), None, C.c_longlong(0), None,
                                                       vp(off), vp(ok), vp(steps))
        assert lq.levels_last_route()["launches"] == (1 if rc == 0 else 0)
        return rc

    assert call(4, [3, 2]) == 0
    assert call(4, np.zeros(0, dtype=np.int32)) == XPG_ERR_SHAPE                    # n_elim <= 0
    assert call(4, [4]) == XPG_ERR_SHAPE and call(4, [3, -1]) == XPG_ERR_SHAPE      # an index outside [0, rhs_idx)
    assert call(0, [0]) == XPG_ERR_SHAPE and call(5, [3]) == XPG_ERR_SHAPE          # rhs_idx outside [1, cols)
    assert call(4, [3], cap=32768) == XPG_ERR_UNSUPPORTED                           # cap > 32767
    assert call(4, [3], cap=4000) == XPG_ERR_UNSUPPORTED                            # the layout of cap rows over 160 KB
    assert call(4, [3] * (pc.CHAIN_MAX + 1)) == XPG_ERR_UNSUPPORTED and call(4, [3] * pc.CHAIN_MAX) == 0
    # the device form takes the caller's capacities as they are: none is defaulted or clamped behind d_outs' row stride
    d = ctx.malloc(4 * 2 * 64 * 5 * 8)
    try:
        for cap, cap_out in ((0, 0), (5, 5), (64, 65), (64, 0)):    # no cap_rows, cap_rows < rows, cap_out_rows > cap_rows, no cap_out_rows
            with pytest.raises(XpgError, match="XPG_ERR_SHAPE"):
                levels_dev(ctx, 4, d, 6, 5, 4, [3, 2], False, cap, cap_out, d, d, d, d)
            assert lq.levels_last_route()["launches"] == 0
    finally:
        ctx.free(d)
    # a sizing call fills the offsets; a buffer one row short is refused with them and the verdicts filled
    assert call(4, [3, 2], cap=64) == 0 and off[8] > 0
    total = int(off[8])
    out = np.zeros((total, 5, 2), dtype=np.int32)
    el = np.array([3, 2], dtype=np.int32)
    args = (ctx._h, C.c_int(4), vp(mats), C.c_int(6), C.c_int(5), C.c_int(4), vp(el), C.c_int(2), C.c_int(0), C.c_int(64), C.c_int(0))
    off[:] = 0; steps[:] = -1
    assert lib().xpg_lineq_levels_batch_packed_rat32(*args, vp(out), C.c_longlong(total - 1), None, vp(off), vp(ok), vp(steps)) == XPG_ERR_SHAPE
    assert off[8] == total and (steps >= 0).all()
    assert lib().xpg_lineq_levels_batch_packed_rat32(*args, vp(out), C.c_longlong(total), None, vp(off), vp(ok), vp(steps)) == 0
    _, _, levels = lq.levels_packed(mats, 4, [3, 2], cap_rows=64)
    assert all(rows_equal(out[off[b * 2 + k]: off[b * 2 + k + 1]], levels[b][k]) for b in range(4) for k in range(2))


# ---- 7. adapter ------------------------------------------------------------------------------------------------------------------
def test_the_adapter_keeps_the_levels_of_three_nest_depths(port, tmp_path):
    """tests/cxx/levels_all.cpp in a child process: nests of depth 3, 4 and 6, each with systems of three shape classes
    interleaved, through xpoly_amd::levels_all and through Lineq::fmeLevels on a list type, every entry compared in there with
    the adapter's own Lineq::fme run as the reference's loop runs it. One class -- 9 rows at depth 3, found here on the CPU --
    has a step that needs more rows than the first capacity tried, so the adapter calls again with the need reported; the
    systems of depth 4 and 6 are drawn until they fit the defaults."""
    from test_lineq_levels_host import build_adapter_test
    exe = build_adapter_test()
    rng = np.random.default_rng(77)
    groups, retry = [], set()
    for nv, row_classes, per in ((3, (4, 6, 9), 4), (4, (5, 8, 10), 4), (6, (5, 8, 12), 6)):
        elim = list(range(nv - 1, 0, -1))
        systems = []
        for k in range(per):
            for rows in row_classes:
                # deep nests can need tens of thousands of rows, and a new need at every step is more calls than the adapter
                # makes: at depth 4 and 6 a system that does not fit the default capacities is drawn again, so that the
                # retries are those of depth 3
                cap = rows * rows // 4 + rows + 1
                while True:
                    m = rng.integers(-3, 4, size=(rows, nv + 1)) * (rng.random((rows, nv + 1)) < 0.7)
                    m[:, nv] = rng.integers(-2, 9, size=rows)
                    if nv == 3 or stepped_levels(port, gen.to_rat(m), nv, elim, cap_rows=cap, cap_out_rows=min(cap, 4 * rows + 16))[0] >= 0:
                        break
                systems.append(m.astype(np.int32))
        for m in systems:
            rows = m.shape[0]
            cap = rows * rows // 4 + rows + 1
            w = stepped_levels(port, gen.to_rat(m), nv, elim)
            if any(n is not None and n > cap for n in w[3]) or any(s > min(cap, 4 * rows + 16) for s in w[4]):
                retry.add((nv, rows))
        groups.append((nv, systems))
    assert retry == {(3, 9)}, retry                 # that class alone is over a default capacity: a second call for it
    lines = ["%d" % len(groups)]
    for nv, systems in groups:
        lines.append("%d %d" % (nv, len(systems)))
        for m in systems:
            lines += ["%d %d" % m.shape, " ".join(str(int(x)) for x in m.ravel())]
    path = str(tmp_path / "nests.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert [ln for ln in out if ln.startswith("group")] == ["group %d rc 0" % g for g in range(3)] and "mismatches 0" in out
    per_system = [ln.split() for ln in out if " ok " in ln]
    assert len(per_system) == sum(len(s) for _, s in groups)
    assert all(p[5] == "1" and p[7] == "1" for p in per_system) and {p[3] for p in per_system} == {"0", "1"}
