"""GPU: the route records of the row-elimination families are independent. One handle calls, in this order, the packed
projection, the packed levels, the ragged projection, the ragged levels, the fused calcBound, the ragged calcBound, the hull
and the projected union, three systems each at shapes no two families share; afterwards every xpg_lineq_*_last_route still
shows its own family's last call -- figure for figure what the family's plan view says of that call's shapes -- the hull calls
have left the ragged and ragged-calcBound records alone although they launch those families' kernels, and a call refused
before its launch (an elimination list with an index >= rhs_idx) zeroes its own family's record and no other. What the calls
compute is the other GPU tests' matter (bit for bit); here only the verdicts' shapes are looked at."""
import numpy as np
import pytest

import lineq_bounds_cases as bc
import lineq_bounds_ragged_cases as brc
import lineq_hull_cases as hc
import lineq_levels_cases as lc
import lineq_project_cases as pc
import lineq_ragged_cases as rc_

pytestmark = pytest.mark.gpu


def _sys(rows, nv, n=1, seed=0):
    return list(rc_.class_batch(rows, nv, n, seed=1000 + 10 * rows + nv + seed))


def _head(plan, keys):
    assert isinstance(plan, dict), plan
    return {k: plan[k] for k in keys}


def _shape(mats):
    return [m.shape[0] for m in mats], [m.shape[1] for m in mats]


def test_every_family_keeps_its_own_record(ctx):
    from xpoly_amd.lineq import Lineq
    from xpoly_amd.six import XpgError
    lq = Lineq(ctx)
    readers = dict(project=Lineq.project_last_route, levels=Lineq.levels_last_route, ragged=Lineq.ragged_last_route,
                   bounds=Lineq.bounds_last_route, bounds_ragged=Lineq.bounds_ragged_last_route, hull=Lineq.hull_ragged_last_route)
    want = {}
    # 1. packed projection: 3 systems of 4 x 3
    a = np.stack(_sys(4, 2, 3))
    ok, _, _ = lq.project_packed(a, 2, [1])
    assert len(ok) == 3
    want["project"] = _head(pc.plan_view(3, 4, 3), pc.PLAN_KEYS[:6])
    assert readers["project"]() == want["project"]
    # 2. packed levels: 3 systems of 5 x 4, two levels
    a = np.stack(_sys(5, 3, 3))
    ok, _, _ = lq.levels_packed(a, 3, [2, 1])
    assert len(ok) == 3
    want["levels"] = _head(lc.plan_view(3, 5, 4, 2), lc.PLAN_KEYS[:7])
    # 3. ragged projection: 4 x 3, 5 x 4, 6 x 5
    mats, elims = _sys(4, 2) + _sys(5, 3) + _sys(6, 4), [[1], [2, 1], [3, 2]]
    ok, _, _ = lq.project_ragged(mats, None, elims)
    assert len(ok) == 3
    rows, cols = _shape(mats)
    ragged_project = _head(rc_.plan_view(rows, cols, None, elims, False), rc_.ROUTE_KEYS)
    assert readers["ragged"]() == ragged_project
    # 4. ragged levels (the same record): 5 x 4, 6 x 5, 8 x 5
    mats, elims = _sys(5, 3, seed=1) + _sys(6, 4, seed=1) + _sys(8, 4), [[2, 1], [3, 2], [3, 2, 1]]
    ok, _, _ = lq.levels_ragged(mats, None, elims)
    assert len(ok) == 3
    rows, cols = _shape(mats)
    want["ragged"] = _head(rc_.plan_view(rows, cols, None, elims, True), rc_.ROUTE_KEYS)
    assert want["ragged"] != ragged_project
    # 5. fused calcBound: 3 systems of 6 x 4
    a = np.stack(_sys(6, 3, 3))
    ok = lq.bounds_packed(a, 3)[0]
    assert len(ok) == 3
    want["bounds"] = _head(bc.plan_view(3, 6, 4, 3), bc.PLAN_KEYS[:7])
    # 6. ragged calcBound: 4 x 3, 6 x 5, 5 x 4
    mats = _sys(4, 2, seed=2) + _sys(6, 4, seed=2) + _sys(5, 3, seed=2)
    ok = lq.bounds_ragged(mats)[0]
    assert len(ok) == 3
    rows, cols = _shape(mats)
    want["bounds_ragged"] = _head(brc.plan_view(rows, cols), brc.ROUTE_KEYS)
    # the six records differ pairwise so far (the hull's is still empty), so none can stand in for another
    before_hull = {k: readers[k]() for k in ("ragged", "bounds_ragged")}
    assert before_hull == {k: want[k] for k in before_hull}
    # 7. hull: two groups, 4 x 3 twice and 5 x 4 (k_calc_bound_ragged produces)
    groups = [_sys(4, 2, 2, seed=3), _sys(5, 3, seed=3)]
    ok = lq.hull_ragged(groups)[0]
    assert len(ok) == 2
    sizes, rows, cols, _ = hc.shapes_of(groups)
    hull = _head(hc.plan_view(sizes, rows, cols)[0], hc.ROUTE_KEYS)
    got = readers["hull"]()
    assert {k: got[k] for k in hc.ROUTE_KEYS} == hull
    assert {k: readers[k]() for k in before_hull} == before_hull
    # 8. projected union (the same record): one group of three 6 x 5 (k_fme_chain_ragged produces)
    groups, elims = [_sys(6, 4, 3, seed=4)], [[[3], [3], [3]]]
    ok = lq.project_union_ragged(groups, None, elims)[0]
    assert len(ok) == 1
    sizes, rows, cols, _ = hc.shapes_of(groups)
    want["hull"] = _head(hc.plan_view(sizes, rows, cols, None, elims[0])[0], hc.ROUTE_KEYS)
    assert want["hull"] != hull
    assert {k: readers[k]() for k in before_hull} == before_hull

    def records():
        got = {k: readers[k]() for k in readers}
        got["hull"] = {k: got["hull"][k] for k in hc.ROUTE_KEYS}
        return got

    # after the whole sequence every record is still its own call's plan
    assert records() == want
    figures = [tuple(v.values()) for v in want.values()]
    assert all(figures[i][:6] != figures[j][:6] for i in range(len(figures)) for j in range(i)), want
    # a call refused before launch zeroes its own family's record and no other
    bad3 = np.stack(_sys(4, 2, 3))
    refused = (
        ("project", lambda: lq.project_packed(bad3, 2, [2])),
        ("levels", lambda: lq.levels_packed(bad3, 2, [1, 2])),
        ("ragged", lambda: lq.project_ragged(list(bad3), None, [[1], [2], [1]])),
        ("hull", lambda: lq.project_union_ragged([list(bad3)], None, [[[1], [1], [2]]])),
    )
    for family, call in refused:
        with pytest.raises(XpgError):
            call()
        want[family] = dict.fromkeys(want[family], 0)
        assert records() == want, family
    with pytest.raises(XpgError):
        lq.levels_ragged(list(bad3), None, [[1], [1], [1, 2]])
    assert records() == want
