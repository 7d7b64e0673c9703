"""Call times and device memory of a projection (a list of variables eliminated out of nb systems of one shape; run by
tools/lab/run_lineq_project_ab.sh), host arrays in, packed rows out:
  one      xpg_lineq_project_batch_packed_rat32: every step of a system in ONE launch
  ragged   what a caller can do without it: one xpg_lineq_fme_batch_ragged_rat32 call per variable, the intermediates
           (ragged by then) handed back as they come
  padded   the same with xpg_lineq_fme_batch_packed_rat32 (cap_rows as the one call's): the intermediates padded on the host
           to the tallest with 0 <= 0 rows (which the next step's reduce removes) and sent up again
Systems: gen.random_system(rows, cols - 1), seed rows * 100 + cols; of --cand candidates the first 64 whose every step fits
--cap rows are kept (the one call itself says which: the others answer -need) and tiled to nb. Every side that runs must agree with the one call bit for bit before anything is timed; a side
the package refuses at a shape (the ragged fme sizes for rows^2 / 4 + rows rows and refuses above 32767), or whose slots
would exceed 8 GB, is printed as not run. One warm-up call per side, then --reps rounds in which the sides alternate; median, min and
max of each side's times, and the median of the time spent inside the package's calls alone (the per-step sides' Python
loops over the systems are the caller's own work, so both figures are given). Memory: the one call's figure is what it allocates (input, final slots, the seats' slots from
xpg_lineq_project_last_route); the per-step sides' is the largest step's input plus the slots the packed fme
allocates for it (ragged: rows^2 / 4 + rows + 1 rows per system; padded: cap_rows), computed from the shapes."""
import argparse
import hashlib
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, required=True)
ap.add_argument("--cols", type=int, required=True)
ap.add_argument("--last", type=int, required=True, help="eliminate the last LAST variables, innermost first")
ap.add_argument("--nb", type=int, required=True)
ap.add_argument("--cap", type=int, default=1024)
ap.add_argument("--cand", type=int, default=4096, help="candidate systems the distinct ones are chosen from")
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, ROOT)

import numpy as np

import xpoly_amd
from tools import gen
from xpoly_amd.lineq import Lineq

rows, cols, nv = args.rows, args.cols, args.cols - 1
elim = list(range(nv - 1, nv - 1 - args.last, -1))
rng = np.random.default_rng(rows * 100 + cols)
cand = np.stack([gen.random_system(rng, rows, nv) for _ in range(args.cand)])
ctx = xpoly_amd.Context(0)
lq = Lineq(ctx)
ok, steps, res = lq.project_packed(cand, nv, elim, cap_rows=args.cap)
fit = [b for b in range(args.cand) if ok[b] >= 0][:64]
assert len(fit) >= 8, "fewer than 8 of the candidates fit --cap"
distinct = len(fit)
base = cand[fit]
cap_out = max(1, max(res[b].shape[0] for b in fit))
mats = np.ascontiguousarray(np.tile(base, (args.nb // distinct + 1, 1, 1, 1))[:args.nb])
nb = args.nb


lib_ms = [0.0]
PADDED_MAX = 8 << 30            # the padded side is not run where one step's worst-case slots exceed this


def timed(fn, *a, **k):
    t0 = time.perf_counter()
    r = fn(*a, **k)
    lib_ms[0] += (time.perf_counter() - t0) * 1e3
    return r


def one():
    return timed(lq.project_packed, mats, nv, elim, cap_rows=args.cap, cap_out_rows=cap_out, copy=False)


def per_step(padded, stats=None):
    cur = [mats[b] for b in range(nb)]
    okv = np.ones(nb, dtype=np.int32); st = np.full(nb, len(elim), dtype=np.int32)
    for k, u in enumerate(elim):
        alive = [b for b in range(nb) if okv[b] == 1 and cur[b].shape[0] > 0]
        if not alive:
            break
        tall = max(cur[b].shape[0] for b in alive)
        if padded:
            cap_step = max(args.cap, tall)                   # the capacity the one call was given, not fme's worst case
            worst = len(alive) * cap_step * cols * 8
            if worst > PADDED_MAX:
                raise MemoryError("step %d would allocate %.1f GB of worst-case slots" % (k, worst / 2.0 ** 30))
            stack = np.zeros((len(alive), tall, cols, 2), dtype=np.int32); stack[..., 1] = 1
            for i, b in enumerate(alive):
                stack[i, : cur[b].shape[0]] = cur[b]
            sok, off, packed = timed(lq.fme_packed, stack, nv, u, False, cap_step)
            out = [packed[off[i]: off[i + 1]] for i in range(len(alive))]
            if stats is not None:
                stats.append(stack.nbytes + worst)
        else:
            sok, out = timed(lq.fme_ragged, [cur[b] for b in alive], [u] * len(alive), [nv] * len(alive))
            if stats is not None:
                stats.append(sum(cur[b].nbytes + (cur[b].shape[0] ** 2 // 4 + cur[b].shape[0] + 1) * cols * 8 for b in alive))
        for b, o, r in zip(alive, sok, out):
            if o:
                cur[b] = r
            else:
                okv[b] = 0; st[b] = k; cur[b] = r[:0]
    return okv, st, [cur[b] if okv[b] == 1 else cur[b][:0] for b in range(nb)]


def digest(r):
    h = hashlib.sha256()
    h.update(np.asarray(r[0]).tobytes()); h.update(np.asarray(r[1]).tobytes())
    for m in r[2]:
        h.update(np.int64(m.shape[0]).tobytes()); h.update(np.ascontiguousarray(m).tobytes())
    return h.hexdigest()[:12]


sides = [("one", one), ("ragged", lambda: per_step(False)), ("padded", lambda: per_step(True))]
mem = {"ragged": [], "padded": []}
first = {"one": digest(one())}
warm = {}
for name, padded in (("ragged", False), ("padded", True)):
    try:
        t0 = time.perf_counter()
        first[name] = digest(per_step(padded, mem[name]))
        warm[name] = time.perf_counter() - t0
    except (MemoryError, xpoly_amd.XpgError) as e:              # a side the package refuses at this shape, or too large to try
        first[name] = "not run: %s" % e
        sides = [sd for sd in sides if sd[0] != name]
# a per-step side whose warm-up call took more than WARM_MAX seconds is not called five more times: its one time is printed
WARM_MAX = 20.0
slow = [name for name, _ in sides if warm.get(name, 0.0) > WARM_MAX]
sides = [sd for sd in sides if sd[0] not in slow]
r1 = lq.project_packed(mats, nv, elim, cap_rows=args.cap, cap_out_rows=cap_out); route = lq.project_last_route()
assert route["launches"] == 1
ran = [name for name in ("ragged", "padded") if not first[name].startswith("not run")]
assert all(first[name] == first["one"] for name in ran), first                  # bit-identical before anything is timed
times = {name: [] for name, _ in sides}
inlib = {name: [] for name, _ in sides}
for _ in range(args.reps):
    for name, fn in sides:
        lib_ms[0] = 0.0
        t0 = time.perf_counter()
        fn()                                                                    # every call of every side ends in a synchronise
        times[name].append((time.perf_counter() - t0) * 1e3)
        inlib[name].append(lib_ms[0])
mem_one = mats.nbytes + nb * cap_out * cols * 8 + route["seat_bytes"] + 3 * nb * 4
print("shape %dx%d eliminate %s nb %d (%d distinct, the first of %d candidates that fit; %d of them do)  cap_rows %d cap_out_rows %d  ok %d inconsistent %d  rows out %d  results %s  route %s" % (
    rows, cols, elim, nb, distinct, args.cand, int((ok >= 0).sum()), args.cap, cap_out, int((r1[0] == 1).sum()), int((r1[0] == 0).sum()), sum(m.shape[0] for m in r1[2]),
    first["one"], route))
for name in ("ragged", "padded"):
    if name not in ran:
        print("   %-7s %s" % (name, first[name]))
for name in slow:
    print("   %-7s warm-up call %9.1f ms, hashes included; not timed further   device memory %10.1f KB (largest step, from the shapes)" % (
        name, warm[name] * 1e3, max(mem[name]) / 1024.0))
for name, _ in sides:
    t = sorted(times[name])
    m = mem_one if name == "one" else max(mem[name])
    print("   %-7s median %9.3f ms  min %9.3f  max %9.3f  (%d rounds after one warm-up; inside the package's calls: median %9.3f ms)   device memory %10.1f KB%s" % (
        name, t[len(t) // 2], t[0], t[-1], len(t), sorted(inlib[name])[len(t) // 2], m / 1024.0, "" if name == "one" else " (largest step, from the shapes)"))
ctx.close()
