"""CPU suite: a batch whose shapes all agree gets, through the ragged plan views (xpg_test_lineq_ragged_plan with both `levels`
values, xpg_test_lineq_bounds_ragged_plan), exactly the figures -- and exactly the return code -- of the uniform views
(xpg_test_lineq_project_plan / _levels_plan / _bounds_plan), at the edges of the capacity and envelope rule:
  cap_rows      0, rows - 1, rows, 32767, 32768
  cap_out_rows  0, 1, cap - 1, cap, cap + 1 (cap: what the kind's rule settles on for that cap_rows; values an `int` cannot hold
                are not calls the ABI has)
  shapes        the last rows x cols on the near side and the first on the far side of fme_lds's 12 KB layout switch (cols 9) and
                of the 160 KB refusal (cols 13), found through tests/lineq_project_cases.py's restatement of fme_lds
  rows          32767, 32768, 46341 and 92682 (rows x rows no longer an int), with every cap_rows and cap_out_rows 0 and 1: the
                whole grid there would pass the thousand calls this file keeps under
Where a uniform plan had more than one system per workgroup the ragged views would have to refuse (their kernels' seat is the
workgroup); the row-elimination kernels take the whole wave, so no shape here has one."""
import lineq_bounds_cases as bc
import lineq_bounds_ragged_cases as brc
import lineq_levels_cases as lc
import lineq_project_cases as pc
import lineq_ragged_cases as rc_
from lineq_project_cases import XPG_ERR_UNSUPPORTED

NB = 3
ELIM = [1, 0]
SHARED = ("launches", "grid", "groups", "sys_lds", "cap_lds", "seat_bytes", "cap", "cap_out")
INT_MAX = 2 ** 31 - 1
CALLS = [0]


def _lib():
    from xpoly_amd import build, _capi
    build.build()
    return _capi.lib()


def _last_within(cols, limit, full):
    """The most rows r for which a cap = r layout of `cols` columns stays within `limit` bytes (full: the all-in-LDS layout)."""
    def lds(r):
        if full:
            capx = r
            return r * cols * 8 * 2 + pc.lineq_lds_bytes(capx, cols) - capx * cols * 8 + 16
        return pc.fme_lds(r, r, cols)[1]
    r = 1
    while lds(r + 1) <= limit:
        r += 1
    return r


def _edge_shapes():
    r12, r160 = _last_within(9, 12 * 1024, True), _last_within(13, 160 * 1024, False)
    assert pc.fme_lds(r12, r12, 9)[0] == r12 and pc.fme_lds(r12 + 1, r12 + 1, 9)[0] < r12 + 1          # the switch lies between them
    assert pc.fme_lds(r160, r160, 13)[1] <= 160 * 1024 < pc.fme_lds(r160 + 1, r160 + 1, 13)[1]
    return [(r12, 9), (r12 + 1, 9), (r160, 13), (r160 + 1, 13)]


def _cap(rows, cap_rows, fme_kind):
    cap = (rows * rows // 4 + rows + 1 if fme_kind else 4 * rows + 16) if cap_rows <= 0 else cap_rows
    return max(cap, rows)


def _agree(u, g, extra, what):
    """u: the uniform view's answer, g: the ragged view's; extra: the ragged view's own figures where both are plans."""
    CALLS[0] += 2
    if not isinstance(u, dict):
        assert g == u, (what, u, g)
        return
    if u["groups"] > 1:
        assert g == XPG_ERR_UNSUPPORTED, (what, u, g)
        return
    assert isinstance(g, dict), (what, u, g)
    assert all(g[k] == u[k] for k in SHARED), (what, u, g)
    for k, v in extra(u).items():
        assert g[k] == v, (what, k, v, u, g)


def _one(rows, cols, cap_rows, cap_outs_of):
    rhs = cols - 1
    rr, cc, el = [rows] * NB, [cols] * NB, [ELIM] * NB
    env = dict(cols=cols, rows=rows)
    for cap_out in cap_outs_of(_cap(rows, cap_rows, True)):
        what = (rows, cols, cap_rows, cap_out)
        _agree(pc.plan_view(NB, rows, cols, cap_rows, cap_out), rc_.plan_view(rr, cc, None, el, False, cap_rows, cap_out),
               lambda u: dict(env, out_bytes=NB * u["cap_out"] * cols * 8), ("project",) + what)
        _agree(lc.plan_view(NB, rows, cols, len(ELIM), cap_rows, cap_out), rc_.plan_view(rr, cc, None, el, True, cap_rows, cap_out),
               lambda u: dict(env, out_bytes=u["level_bytes"]), ("levels",) + what)
    for cap_out in cap_outs_of(_cap(rows, cap_rows, False)):
        what = (rows, cols, cap_rows, cap_out)
        _agree(bc.plan_view(NB, rows, cols, rhs, cap_rows, cap_out), brc.plan_view(rr, cc, None, cap_rows, cap_out),
               lambda u: dict(env, steps=NB * u["steps"], out_bytes=NB * rhs * u["cap_out"] * cols * 8), ("bounds",) + what)


def test_uniform_and_ragged_plans_agree_at_the_capacity_edges():
    _lib()
    CALLS[0] = 0
    some_plan, some_refusal = [0], [0]
    for rows, cols in _edge_shapes():
        for cap_rows in (0, rows - 1, rows, 32767, 32768):
            _one(rows, cols, cap_rows, lambda cap: sorted({v for v in (0, 1, cap - 1, cap, cap + 1) if 0 <= v <= INT_MAX}))
            some_plan[0] += isinstance(pc.plan_view(NB, rows, cols, cap_rows), dict)
            some_refusal[0] += pc.plan_view(NB, rows, cols, cap_rows) == XPG_ERR_UNSUPPORTED
    assert some_plan[0] >= 3 and some_refusal[0] >= 3          # both sides of the refusal were met
    assert CALLS[0] <= 600, CALLS[0]                           # (with the 40 above, the 240 + 40 below: 920 in this file)


def test_rows_whose_square_is_no_int_are_refused_alike():
    _lib()
    CALLS[0] = 0
    for rows in (32767, 32768, 46341, 92682):
        for cap_rows in (0, rows - 1, rows, 32767, 32768):
            _one(rows, 3, cap_rows, lambda cap: (0, 1))
            assert pc.plan_view(NB, rows, 3, cap_rows) == XPG_ERR_UNSUPPORTED
            assert bc.plan_view(NB, rows, 3, 2, cap_rows) == XPG_ERR_UNSUPPORTED
    assert CALLS[0] <= 240, CALLS[0]
