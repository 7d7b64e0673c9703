#!/usr/bin/env python3
"""Generates tests/golden/g14_hull.json from the REAL reference (oracle/_ref/libxpoly_ref.so, `make -C oracle ref`):
Lineq::ConvexHullUnionAndIntersect (linsys.cpp:283-336) composed from the reference's own fme chains and reduce
(tests/lineq_hull_cases.py hull), and the projected union of PolyTran::step_4 composed the same way, for the groups of the
hull tests. Authoring-container only; the fixture is data: the members of every group (num, den, cell by cell), the mode and
the expected verdict and rows.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.checker import Ref  # noqa: E402
import lineq_hull_cases as hc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g14_hull.json")


def enc(a):
    return [int(x) for x in np.asarray(a).reshape(-1)]


def main():
    ref = Ref()
    groups, rhss, names = hc.hull_batch(ref)
    cases = []
    for g, (members, rhs, name) in enumerate(zip(groups, rhss, names)):
        for flag in (0, 1):
            ok, member, chain, steps, rows, gathered = hc.hull(ref, members, rhs, bool(flag))
            cases.append(dict(kind="hull", name=name, rhs=rhs, is_intersect=flag,
                              members=[dict(rows=m.shape[0], cols=m.shape[1], cells=enc(m)) for m in members],
                              ok=ok, member=member, gathered=gathered, out_rows=int(rows.shape[0]), out=enc(rows)))
    good, _ = hc.pools(ref)
    for c, n in ((1, 3), (2, 2), (3, 4), (5, 17)):
        nv = hc.CLASSES[c][1]
        members = good[c][:n]
        elims = [list(range(nv - 1, 0, -1))] * n
        for flag in (0, 1):
            ok, member, chain, steps, rows, gathered = hc.project_union(ref, members, nv, elims, bool(flag))
            cases.append(dict(kind="union", name="c%d x%d" % (c, n), rhs=nv, is_intersect=flag, elim=elims[0],
                              members=[dict(rows=m.shape[0], cols=m.shape[1], cells=enc(m)) for m in members],
                              ok=ok, member=member, gathered=gathered, out_rows=int(rows.shape[0]), out=enc(rows)))
    json.dump(dict(cases=cases), open(OUT, "w"))
    print("%s: %d cases, %d bytes" % (OUT, len(cases), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
