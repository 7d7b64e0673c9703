"""A/B of Lineq.transform_levels_packed (k_transform_levels_batch: det, T^-1, A * T^-1 and every level in ONE launch on a shared
nest) against the composition a caller makes today out of the parent's entry points: Lineq.inv (one launch, one
synchronisation), the product A * T^-1 on the host, Lineq.levels_packed on the transformed nests (a second upload, launch and
synchronisation). On an MI355X:
    python tools/lab/run_transform_ab.py            (writes profiles/lineq_transform_ab.txt)

The search over transformations: ONE triangular nest 0 <= i0 <= 3, 0 <= ik <= i(k-1) + 2 of depth 3, 4 and 6 against 1, 1024
and 16384 unimodular candidates -- a skew, an interchange or a reversal, or the product of two of them (seeded). The candidates
are integer and unimodular, so T^-1 is integer and the host product of the composition is ONE vectorised integer matmul in
numpy written straight into the (num, den) array that levels_packed takes (the reference's operator* cell by cell in Python
would only make that side slower); that the inverses are integer is checked once, outside the timed calls. Before anything is
timed the two sides are compared bit for bit: level 0 with the host product, every further level and both verdicts with
levels_packed's. Each side: 2 warm-up calls, then 7 alternating rounds, wall clock around the Python call (host arrays in,
packed rows out as views); median, min and max are stated for each side. Then each side 7 times IN A ROW after 2 calls of its
own: the handle parks at most 16 device blocks and frees the largest first (ctx.hip.h DevBuf), so two alternating sides with
blocks of different sizes may pay hipMalloc / hipFree every round where one side alone does not -- the rows `in a row` show
whether a spread is the alternation's. Nothing else is left out."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "lineq_transform_ab.txt")


def to_rat(m):
    a = np.asarray(m, dtype=np.int32)
    out = np.empty(a.shape + (2,), dtype=np.int32)
    out[..., 0] = a
    out[..., 1] = 1
    return out


def nest(d):
    rows = []
    for k in range(d):
        lo = [0] * (d + 1); lo[k] = -1
        up = [0] * (d + 1); up[k] = 1
        if k:
            up[k - 1] = -1
        up[d] = 3 if k == 0 else 2
        rows += [lo, up]
    return np.array(rows, dtype=np.int64)


def candidate(rng, d):
    t = np.eye(d, dtype=np.int64)
    for _ in range(int(rng.integers(1, 3))):
        e = np.eye(d, dtype=np.int64)
        kind = int(rng.integers(0, 3))
        i, j = (int(x) for x in rng.choice(d, size=2, replace=False))
        if kind == 0:
            e[i, j] = int(rng.choice((-1, 1)))                  # a skew
        elif kind == 1:
            e[[i, j]] = e[[j, i]]                               # an interchange
        else:
            e[i, i] = -1                                        # a reversal
        t = e @ t
    return t


def main():
    import xpoly_amd
    from xpoly_amd.lineq import Lineq
    ctx = xpoly_amd.Context(0)
    lq = Lineq(ctx)
    lines = [ln for ln in __doc__.strip().split("\n")]
    text = ["# " + ln if ln else "#" for ln in lines] + ["#"]
    for d in (3, 4, 6):
        a = nest(d)
        a_rat = to_rat(a)
        elim = list(range(d - 1, 0, -1))
        for nb in (1, 1024, 16384):
            rng = np.random.default_rng(1000 * d + nb)
            ts = to_rat(np.stack([candidate(rng, d) for _ in range(nb)]))

            def one_call():
                return lq.transform_levels_packed(a_rat, ts, d, shared_nest=True, copy=False)

            def composition():
                ok, inv = lq.inv(ts)
                prod = np.empty((nb,) + a.shape + (2,), dtype=np.int32)      # the rational product, built once
                prod[..., 1] = 1
                prod[:, :, d:, 0] = a[None, :, d:]
                np.matmul(a[None, :, :d], inv[..., 0].astype(np.int64), out=prod[:, :, :d, 0], casting="unsafe")
                return (ok, inv, prod) + lq.levels_packed(prod, d, elim, copy=False)

            iok, inv, prod, cok, csteps, clev = composition()
            assert iok.all() and (inv[..., 1] == 1).all()                    # integer inverses: checked once, outside the timing
            clev = [[lv.copy() for lv in sysl] for sysl in clev]
            ok, steps, kind, det, mult, lev = one_call()
            assert not kind.any() and np.array_equal(mult, inv) and np.array_equal(ok, cok) and np.array_equal(steps, csteps)
            for b in range(nb):
                assert ok[b] != 1 or np.array_equal(lev[b][0], prod[b])
                assert all(x.shape[0] == y.shape[0] == 0 or np.array_equal(x, y) for x, y in zip(lev[b][1:], clev[b])), (d, nb, b)
            route = lq.transform_last_route()
            times = {"one call": [], "composition": []}
            for fn in (one_call, composition):
                fn(); fn()
            for _ in range(7):
                for name, fn in (("one call", one_call), ("composition", composition)):
                    t0 = time.perf_counter()
                    fn()
                    times[name].append((time.perf_counter() - t0) * 1e3)
            for name, fn in (("one call", one_call), ("composition", composition)):
                fn(); fn()
                times[name + ", in a row"] = []
                for _ in range(7):
                    t0 = time.perf_counter()
                    fn()
                    times[name + ", in a row"].append((time.perf_counter() - t0) * 1e3)
            text.append("depth %d  %2d x %d  nb %5d  verdicts ok %d, inconsistent %d, short %d" %
                        (d, a.shape[0], d + 1, nb, int((ok == 1).sum()), int((ok == 0).sum()), int((ok < 0).sum())))
            for name in ("one call", "composition", "one call, in a row", "composition, in a row"):
                v = times[name]
                note = ("" if name.endswith("row") else
                        "1 launch, grid %d, LDS %d B/system, level slots %d B" % (route["grid"], route["sys_lds"], route["level_bytes"])
                        if name == "one call" else "inv, host product, levels_packed: 2 launches, 2 uploads")
                text.append("   %-21s median %8.3f  min %8.3f  max %8.3f ms   %s" % (name, statistics.median(v), min(v), max(v), note))
    ctx.close()
    with open(OUT, "w") as f:
        f.write("\n".join(text) + "\n")
    print("\n".join(text))


if __name__ == "__main__":
    main()
