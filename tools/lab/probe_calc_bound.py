"""Call times and device memory of Lineq::calcBound for nb systems of one shape (run by tools/lab/run_calc_bound_ab.sh), host
arrays in, packed rows out, both sides through the C entry points themselves (no per-result Python work is timed):
  fused    xpg_lineq_bounds_batch_packed_rat32: every chain of a system in ONE launch, the chains' shared prefixes walked once
  chained  xpg_lineq_calc_bound_batch_packed_rat32: rhs (rhs - 1) k_fme_batch launches over three [nb][cap][cols] areas
Systems: triangular loop nests of --depth variables, the shape src/eng/ldtran.cpp hands over -- variable k is bounded below
and above by affine forms of the variables outside it (coefficients in -2 .. 2, about one outer variable per bound), 2 * depth
rows, no symbols. 64 distinct nests (seed 1000 * depth) tiled to nb. Before anything is timed every step of every chain of the distinct
nests is run on the CPU (oracle/checker.py Port) and must fit cap_rows (the default, 4 rows + 16), and the two sides must agree
bit for bit: verdicts, offsets and rows. One warm-up call per side, then --reps rounds in which the sides alternate; median,
min and max. Memory: what each side allocates on the device, from the shapes (fused: input, the nb * rhs result slots, the
seats' slots of xpg_lineq_bounds_last_route; chained: three [nb][cap][cols] areas and the [nb][rhs][cap][cols] results)."""
import argparse
import ctypes as C
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
ap = argparse.ArgumentParser()
ap.add_argument("--depth", type=int, required=True)
ap.add_argument("--nb", type=int, required=True)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, ROOT)

import numpy as np

import xpoly_amd
from oracle.checker import Port
from tools import gen
from xpoly_amd._capi import lib, vp
from xpoly_amd.lineq import Lineq

nv, rows, cols, nb = args.depth, 2 * args.depth, args.depth + 1, args.nb
cap = 4 * rows + 16
DISTINCT = 64


def nest(rng):
    m = np.zeros((rows, cols), dtype=np.int32)
    for k in range(nv):
        dens = min(0.5, 1.0 / max(k, 1))                                # about one outer variable per bound, as tiled nests have
        lo = rng.integers(-2, 3, size=k) * (rng.random(k) < dens)
        hi = rng.integers(-2, 3, size=k) * (rng.random(k) < dens)
        m[2 * k, :k] = lo; m[2 * k, k] = -1; m[2 * k, nv] = -int(rng.integers(0, 4))          # x_k >= lo . x + c
        m[2 * k + 1, :k] = -hi; m[2 * k + 1, k] = 1; m[2 * k + 1, nv] = int(rng.integers(8, 40))   # x_k <= hi . x + c'
    return gen.to_rat(m)


def sign(cell):
    return int(np.sign(int(cell[0]) * int(cell[1])))


def largest_need(port, mat):
    """The rows the largest step of any chain needs before it is reduced; the chains stop as the kernel's do."""
    worst = mat.shape[0]
    for j in range(nv):
        cur = mat
        for u in (i for i in range(nv - 1, -1, -1) if i != j):
            if cur.shape[0] == 0:
                break
            s = [sign(cur[i, u]) for i in range(cur.shape[0])]
            p, n = s.count(1), s.count(-1)
            worst = max(worst, s.count(0) + (1 if p + n == 1 else p * n))
            ok, cur = port.fme(cur, nv, u, False)
            if not ok:
                break
    return worst


rng = np.random.default_rng(1000 * args.depth)
base = np.stack([nest(rng) for _ in range(DISTINCT)])
port = Port()
need = max(largest_need(port, m) for m in base)
assert need <= cap, "a step needs %d rows, cap_rows is %d" % (need, cap)
mats = np.ascontiguousarray(np.tile(base, (nb // DISTINCT + 1, 1, 1, 1))[:nb])

ctx = xpoly_amd.Context(0)
nres = nb * nv
off_f = np.zeros(nres + 1, dtype=np.int64); off_c = np.zeros(nres + 1, dtype=np.int64)
ok_f = np.zeros(nb, dtype=np.int32); ok_c = np.zeros(nb, dtype=np.int32); chain = np.zeros(nb, dtype=np.int32); steps = np.zeros(nb, dtype=np.int32)
view_f, view_c = C.c_void_p(), C.c_void_p()


def fused():
    ctx.check(lib().xpg_lineq_bounds_batch_packed_rat32(ctx._h, C.c_int(nb), vp(mats), C.c_int(rows), C.c_int(cols), C.c_int(nv), C.c_int(0), C.c_int(0),
                                                        None, C.c_longlong(0), C.byref(view_f), vp(off_f), vp(ok_f), vp(chain), vp(steps)), "fused")


def chained():
    ctx.check(lib().xpg_lineq_calc_bound_batch_packed_rat32(ctx._h, C.c_int(nb), vp(mats), C.c_int(rows), C.c_int(cols), C.c_int(nv), C.c_int(0),
                                                            None, C.c_longlong(0), C.byref(view_c), vp(off_c), vp(ok_c)), "chained")


def rows_of(view, off):
    total = int(off[-1])
    out = np.empty((total, cols, 2), dtype=np.int32)
    if total:
        C.memmove(out.ctypes.data, view.value, out.nbytes)
    return out


fused(); rows_f = rows_of(view_f, off_f); route = Lineq.bounds_last_route()          # (both views are of one pinned buffer: copied out at once)
chained(); rows_c = rows_of(view_c, off_c)
assert route["launches"] == 1
assert np.array_equal(ok_f, ok_c) and np.array_equal(off_f, off_c) and np.array_equal(rows_f, rows_c), "the sides differ"   # before anything is timed
assert (ok_f >= 0).all()
times = {"fused": [], "chained": []}
for _ in range(args.reps):
    for name, fn in (("fused", fused), ("chained", chained)):
        t0 = time.perf_counter()
        fn()                                                                         # both calls end in a synchronise
        times[name].append((time.perf_counter() - t0) * 1e3)
slot = cap * cols * 8
mem = {"fused": mats.nbytes + nres * slot + route["seat_bytes"] + nres * 12 + nb * 12,
       "chained": 3 * nb * slot + nres * slot + nres * 12 + nb * 16}
print("depth %d (%d x %d) nb %d (%d distinct nests)  cap_rows %d, largest step need %d  ok %d inconsistent %d  rows out %d  steps per system %d against %d  route %s" % (
    nv, rows, cols, nb, DISTINCT, cap, need, int((ok_f == 1).sum()), int((ok_f == 0).sum()), int(off_f[-1]), route["steps"], nv * (nv - 1), route))
for name in ("fused", "chained"):
    t = sorted(times[name])
    print("   %-8s median %9.3f ms  min %9.3f  max %9.3f  (%d rounds after one warm-up)   device memory %10.1f KB (from the shapes)" % (
        name, t[len(t) // 2], t[0], t[-1], len(t), mem[name] / 1024.0))
tf, tc = sorted(times["fused"]), sorted(times["chained"])
print("   chained / fused, medians: %.2f" % (tc[len(tc) // 2] / tf[len(tf) // 2]))
ctx.close()
