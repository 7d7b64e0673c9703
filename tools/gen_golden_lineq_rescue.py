#!/usr/bin/env python3
"""Generates tests/golden/g17_lineq_rescue.json from the REAL reference (oracle/_ref/libxpoly_ref.so, `make -C oracle ref`):
for the first GOLDEN_PER systems of every family of tests/lineq_rescue_cases.py that runs at the default capacities -- loop
nests whose coefficients make the Rational take its float32 rescue inside the chain -- what the reference's own Lineq::fme
returns step after step over the list depth-1 .. 1, what its Lineq::calcBound returns, and for the transformations of the cases
its Matrix<Rational>::det and ::inv; next to each the delta of the reference's own appro counter. Authoring-container only.
The fixture is data: an input is named by its family and index (the generator's seed) with the CRC-32 of its cells, the outputs
are integer arrays.
"""
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.checker import Ref  # noqa: E402
import lineq_levels_cases as lc  # noqa: E402
import lineq_rescue_cases as rq  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g17_lineq_rescue.json")


def enc(a):
    return [int(x) for x in np.asarray(a).reshape(-1)]


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.int32).tobytes())


def main():
    ref = Ref()
    families = {}
    for name in rq.SMALL:
        n = rq.depth(name)
        out = []
        for b, m in enumerate(rq.family(name, rq.GOLDEN_PER)):
            (ok, steps, levels, _, _), r_fme = rq.counted(ref, lc.stepped_levels, ref, m, n, rq.elim_of(n))
            (cb_ok, bounds), r_cb = rq.counted(ref, ref.calc_bound, m, n)
            out.append(dict(b=b, crc=crc(m), rows=int(m.shape[0]), cols=int(m.shape[1]), ok=ok, steps=steps, appro_fme=r_fme,
                            levels=[dict(rows=int(lv.shape[0]), cells=enc(lv)) for lv in levels],
                            cb_ok=cb_ok, appro_cb=r_cb, bounds=[dict(rows=int(x.shape[0]), cells=enc(x)) for x in bounds]))
        families[name] = out
    tmats = {}
    for n in (2, 3, 4):
        per = {}
        for name, t in rq.tmats(n).items():
            det, r_det = rq.counted(ref, ref.rat_det, t)
            (inv_ok, inv), r_inv = rq.counted(ref, ref.rat_inv, t)
            per[name] = dict(crc=crc(t), det=[int(det[0]), int(det[1])], appro_det=r_det, inv_ok=int(inv_ok), appro_inv=r_inv, inv=enc(inv))
        tmats[str(n)] = per
    json.dump(dict(per=rq.GOLDEN_PER, families=families, tmats=tmats), open(OUT, "w"), separators=(",", ":"))
    print("%s: %d systems, %d transformations, %d bytes" % (OUT, sum(len(v) for v in families.values()),
                                                            sum(len(v) for v in tmats.values()), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
