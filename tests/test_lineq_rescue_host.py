"""No device: the inputs of tests/test_gpu_lineq_rescue.py ARE in the regime where the Rational approximates, the restatement
(oracle/oracle.cpp) equals the real reference on them bit for bit -- against tests/golden/g17_lineq_rescue.json always, against
the reference's build where it is present -- and no expected answer is trivial. The thresholds are conditions on the inputs:
where a changed generator misses one, the inputs change, not the threshold."""
import json
import os
import zlib
from fractions import Fraction

import numpy as np
import pytest

import lineq_bounds_cases as bc
import lineq_levels_cases as lc
import lineq_project_cases as pc
import lineq_rescue_cases as rq
import lineq_transform_cases as tc
from lineq_rescue_cases import rows_equal


def _int_det(m):
    """The determinant of an integer matrix in Python integers, by the first row."""
    if len(m) == 1:
        return m[0][0]
    return sum((-1) ** j * m[0][j] * _int_det([r[:j] + r[j + 1:] for r in m[1:]]) for j in range(len(m)))


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_lineq_rescue.json")


@pytest.fixture(scope="module")
def chains(port):
    """{family: ([lineq_project_cases.stepped], [rescues])} at no capacity, computed once."""
    return {f: rq.want_project(port, rq.family(f), rq.depth(f)) for f in rq.FAMILIES}


@pytest.fixture(scope="module")
def gold():
    return json.load(open(GOLD))


# ---- the cases are in the regime --------------------------------------------------------------------------------------------------
def test_the_tiled_families_make_the_rational_approximate(chains):
    for f in rq.TILED:
        _, rescues = chains[f]
        hit = sum(r > 0 for r in rescues)
        assert 2 * hit >= len(rescues), (f, rescues)                                 # at least half
        if rq.FAMILIES[f][1] == rq.W:
            assert hit == len(rescues), (f, rescues)                                 # at (30 000, 70 000) all of them
    for f in ("d4_empty", "d4_prediv"):                                              # the other families: at least half too
        assert 2 * sum(r > 0 for r in chains[f][1]) >= rq.PER, (f, chains[f][1])


def test_the_late_family_starts_to_rescue_inside_the_chain(port):
    firsts = [rq.first_rescue_step(port, m, 5) for m in rq.family("d5_late")]
    assert any(k is not None and k >= 2 for k in firsts), firsts
    # and the large range at its first step, so both ends of a chain meet a rescue
    assert any(rq.first_rescue_step(port, m, 3) == 0 for m in rq.family("d3_w"))


def test_the_predivided_family_enters_with_denominators(port):
    mats = rq.family("d4_prediv")
    assert (mats[..., 1] > 1).all() and (mats[..., 1] >= rq.W[0]).any()
    lead = [next(c for c in row if c[0] != 0) for m in mats for row in m]
    assert all(abs(int(c[0])) == int(c[1]) for c in lead)                            # s/|s|: not canonical


def test_the_skew_product_is_in_the_regime(port):
    for n in (2, 3, 4):
        a = rq.transform_nests(n, 1)[0]
        for name, t in rq.skews(n).items():
            kind, det, m = tc.kind_of(port, t)
            assert kind == 0 and det in ((1, 1), (-1, 1)), (n, name, kind, det)
            assert int(np.abs(m[..., 0]).max()) == rq.SKEW                           # the inverse is exact and carries the skew
            _, rescues = rq.counted(port, tc.product, port, a, m, n)
            assert rescues > 0, (n, name)
        _, rescues = rq.counted(port, tc.product, port, a, rq.tmats(n)["identity"], n)
        assert rescues == 0


def test_the_determinant_of_one_transformation_approximates(port):
    for n in (2, 3, 4):
        (kind, det, m), rescues = rq.counted(port, tc.kind_of, port, rq.det_rescued(n))
        assert rescues > 0 and kind in (1, 2) and m is None, (n, kind, det, rescues)
        assert det[1] == 0 or Fraction(det[0], det[1]) != _int_det(rq.det_rescued(n)[..., 0].tolist()), (n, det)   # not the determinant


# ---- no answer is trivial ----------------------------------------------------------------------------------------------------------
def test_no_answer_is_trivial(port, chains):
    for f, (want, _) in chains.items():
        n = rq.depth(f)
        if f == "d4_empty":
            assert all((w[0], w[1]) == (0, n - 2) for w in want), f                  # variable 1 goes at the last step
            assert all(sum(rq.rescues_by_step(port, m, n)[: n - 2]) > 0 for m in rq.family(f)), f   # ... after steps that rescued
            continue
        assert all((w[0], w[1]) == (1, n - 1) and w[2].shape[0] >= 2 for w in want), f


def test_the_default_capacities_hold_every_chain(port, chains):
    """The list depth-1 .. 1 never needs more than 11 rows, and every call of the small families at its defaults is the all-LDS
    layout's; calcBound's chains, which eliminate in other orders, stay within 4 * rows + 16."""
    most = 0
    for f in rq.SMALL:
        mats, n = rq.family(f), rq.depth(f)
        rows, cols = mats.shape[1:3]
        needs = [x for w in chains[f][0] for x in w[3] if x is not None]
        most = max(most, max(needs))
        assert max(needs) <= pc.plan(rq.PER, rows, cols)["cap"], f
        p = pc.plan(rq.PER, rows, cols)
        assert p["cap_lds"] == p["cap"], (f, p)
        sizes = [s for m in mats for s in lc.stepped_levels(port, m, n, rq.elim_of(n))[4]]
        assert max(sizes) <= lc.plan(rq.PER, rows, cols, n - 1)["cap_out"], f
        b = bc.plan(rq.PER, rows, cols, n)
        assert b["cap_lds"] == b["cap"], (f, b)
        assert max(x for m in mats for x in bc.step_needs(port, m, n)[0].values()) <= b["cap"], f
    assert most == 11


def test_the_wide_family_needs_the_device_slots(port, chains):
    """d5_wide at WIDE_CAP: past the 12 KB layout, and steps of rescued systems on both sides of cap_lds."""
    rows, cols = rq.family("d5_wide", 1).shape[1:3]
    p = pc.plan(rq.WIDE_NB, rows, cols, rq.WIDE_CAP)
    assert p["cap_lds"] < p["cap"] == rq.WIDE_CAP and p["sys_lds"] > 12 * 1024, p
    want, rescues = chains["d5_wide"]
    needs = [x for w in want[: rq.WIDE_NB] for x in w[3]]
    assert all(r > 0 for r in rescues[: rq.WIDE_NB]) and max(needs) <= rq.WIDE_CAP
    assert any(x <= p["cap_lds"] for x in needs) and sum(x > p["cap_lds"] for x in needs) >= rq.WIDE_NB, (p["cap_lds"], sorted(needs))
    assert all(w[3][0] == 17 for w in want)                                          # 8 rows without i4, 3 x 3 pairs
    b = bc.plan(rq.WIDE_NB, rows, cols, 5, rq.WIDE_CAP)
    bneeds, prefix = [], []
    for m in rq.family("d5_wide", rq.WIDE_NB):
        x, y = bc.step_needs(port, m, 5)
        bneeds += list(x.values()); prefix += y
    assert b["cap_lds"] < b["cap"] == rq.WIDE_CAP and max(bneeds) <= rq.WIDE_CAP
    assert any(x <= b["cap_lds"] for x in bneeds) and sum(x > b["cap_lds"] for x in bneeds) >= rq.WIDE_NB
    assert any(x > b["cap_lds"] for x in prefix)                                     # a prefix built directly in the hold slot


def test_the_mixed_list_and_the_groups(port):
    mats, nvs, elims, names = rq.mixed_list()
    assert len(mats) == 21 and names.count("exact") == 3 and {m.shape for m in mats} >= {(6, 4, 2), (8, 6, 2), (10, 7, 2), (9, 5, 2)}
    for m, nv, el, name in zip(mats, nvs, elims, names):
        _, r = rq.counted(port, pc.stepped, port, m, nv, el)
        assert (r == 0) if name == "exact" else (r > 0 or name.endswith("_k")), (name, r)
    groups, rhss, gnames = rq.groups()
    assert [len(g) for g in groups] == [1, 2, 5, 3]
    for flag in (False, True):
        hulls, hr = rq.want_hulls(port, flag)
        unions, ur = rq.want_unions(port, flag)
        assert all(r > 0 for r in hr) and all(r > 0 for r in ur)
        assert hulls[3][:4] == (0, 1, 0, 2) and hulls[3][4].shape[0] == 0            # the empty member's verdict, no rows
        assert unions[3][:4] == (0, 1, -1, 2) and unions[3][4].shape[0] == 0
        assert all(h[0] == 1 and h[4].shape[0] > 0 for h in hulls[:3]) and all(u[0] == 1 and u[4].shape[0] > 0 for u in unions[:3])


# ---- the restatement equals the real reference on these inputs -----------------------------------------------------------------------
def _cells(d, cols):
    return np.array(d["cells"], dtype=np.int32).reshape(d["rows"], cols, 2)


def test_the_restatement_reproduces_the_reference_fixture(port, gold):
    assert gold["per"] == rq.GOLDEN_PER and set(gold["families"]) == set(rq.SMALL)
    rescued = 0
    for f, cases in gold["families"].items():
        n = rq.depth(f)
        for c, m in zip(cases, rq.family(f, rq.GOLDEN_PER)):
            assert zlib.crc32(m.tobytes()) == c["crc"] and m.shape[:2] == (c["rows"], c["cols"]), (f, c["b"])   # the generator's input
            (ok, steps, levels, _, _), r = rq.counted(port, lc.stepped_levels, port, m, n, rq.elim_of(n))
            assert (ok, steps, r) == (c["ok"], c["steps"], c["appro_fme"]), (f, c["b"], ok, steps, r)
            assert len(levels) == len(c["levels"]) and all(rows_equal(lv, _cells(w, c["cols"])) for lv, w in zip(levels, c["levels"])), (f, c["b"])
            (cb_ok, bounds), r = rq.counted(port, port.calc_bound, m, n)
            assert (cb_ok, r) == (c["cb_ok"], c["appro_cb"]), (f, c["b"], cb_ok, r)
            assert len(bounds) == len(c["bounds"]) and all(rows_equal(x, _cells(w, c["cols"])) for x, w in zip(bounds, c["bounds"])), (f, c["b"])
            rescued += c["appro_fme"] > 0
            # the composition the device is held against is calcBound itself
            chained = bc.chains(port, m, n)
            assert chained[0] == cb_ok and (not cb_ok or all(rows_equal(x, y) for x, y in zip(chained[3], bounds))), (f, c["b"])
    assert rescued >= 14
    for n, per in gold["tmats"].items():
        ts = rq.tmats(int(n))
        assert set(per) == set(ts)
        for name, c in per.items():
            t = ts[name]
            assert zlib.crc32(t.tobytes()) == c["crc"], (n, name)
            det, r = rq.counted(port, port.rat_det, t)
            assert (list(det), r) == (c["det"], c["appro_det"]), (n, name, det, r)
            (ok, inv), r = rq.counted(port, port.rat_inv, t)
            assert (int(ok), r) == (c["inv_ok"], c["appro_inv"]) and np.array_equal(inv.reshape(-1), c["inv"]), (n, name)
        assert per["det_rescued"]["appro_det"] > 0


def _same_chain(a, b):
    return a[:2] == b[:2] and rows_equal(a[2], b[2])


def test_the_restatement_equals_the_reference_build(port, ref, chains):
    """Every system of every family, the mixed list, the groups and the transformed nests: what the GPU tests expect, computed by
    the reference's own build, with its own count of rescues."""
    for f in rq.FAMILIES:
        mats, n = rq.family(f), rq.depth(f)
        want, rescues = rq.want_project(ref, mats, n)
        assert rescues == chains[f][1] and all(_same_chain(a, b) for a, b in zip(want, chains[f][0])), f
        wb, rb = rq.want_bounds(ref, mats[:8], n)
        pb, prb = rq.want_bounds(port, mats[:8], n)
        assert rb == prb and all(a[:3] == b[:3] and all(rows_equal(x, y) for x, y in zip(a[3], b[3])) for a, b in zip(wb, pb)), f
    for flag in (False, True):
        for fn in (rq.want_hulls, rq.want_unions):
            (a, ra), (b, rb) = fn(ref, flag), fn(port, flag)
            assert ra == rb and all(x[:4] == y[:4] and rows_equal(x[4], y[4]) for x, y in zip(a, b)), (flag, fn.__name__)
    for n in (2, 3, 4):
        pairs = [(a, t) for t in rq.tmats(n).values() for a in rq.transform_nests(n, 2)]
        for mode in (0, 1):
            (a, ra), (b, rb) = rq.want_transformed(ref, pairs, mode, 64, 64), rq.want_transformed(port, pairs, mode, 64, 64)
            assert ra == rb, (n, mode)
            for x, y in zip(a, b):
                assert x[:4] == y[:4] and np.array_equal(x[4], y[4]) and all(rows_equal(p, q) for p, q in zip(x[5], y[5])), (n, mode)
