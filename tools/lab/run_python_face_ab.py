"""A/B of the host time inside the Python face (xpoly_amd/six.py, xpoly_amd/lineq.py): the PARENT's package against this tree's,
in front of a stand-in for the library that returns at once -- no device, no libxpoly_amd.so. The stand-in copies prepared
offsets, counts and verdicts into the call's outputs and points the view at a prepared buffer, the same work for both sides, so
what is timed is the face: shaping and checking the arguments, packing ragged systems, building the ctypes call, reading the
rows down and cutting them into the lists it returns.

Parent and tree run alternately three times (parent, tree, parent, tree, parent, tree), ONE CHILD PROCESS PER FIGURE, its
PYTHONPATH selecting the side; both sides run with MALLOC_MMAP_THRESHOLD_ and MALLOC_TRIM_THRESHOLD_ fixed at 1 GiB so that after
the warm-up no call pays for fresh pages (tools/lab/run_lineq_collectors_ab.py has the reason). Each figure is 5 warm-up calls,
then the median of 101, in microseconds. The reading is the rule of profiles/lineq_walks_ab.txt: the tree passes where the median
of its three medians lies inside the range of the parent's three, or above that range by no more than the range's width.

The figures: fme_packed on ONE 16 x 9 system with copy=False (the path of bench.py's fme_one_system_call_us); reduce_packed,
fme_packed, project_packed and levels_packed on 16384 such systems with copy=False, levels_packed also with copy=True; on the
692-system mixed SCoP of tools/lab/probe_lineq_ragged.py levels_ragged, bounds_ragged, hull_ragged (346 groups of 2 of one
class) and has_solution_ragged (the same row counts, every system widened to the SCoP's 7 columns: the call takes one vc);
six_batch_vc and has_solution_batch at 8192 problems of 8 + 2 rows x 6 columns.

Usage: python tools/lab/run_python_face_ab.py PARENT_WORKTREE   (a `git worktree` of the parent commit)"""
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HANDLE = 0x51DE
NAMES = ("fme_packed, 1 system, copy=False", "reduce_packed, 16384 systems, copy=False", "fme_packed, 16384 systems, copy=False",
         "project_packed, 16384 systems, copy=False", "levels_packed, 16384 systems, copy=False", "levels_packed, 16384 systems, copy=True",
         "levels_ragged, the 692-system SCoP, copy=False", "bounds_ragged, the 692-system SCoP, copy=False",
         "hull_ragged, 346 groups of 2, copy=False", "has_solution_ragged, the 692-system SCoP", "six_batch_vc, 8192 problems",
         "has_solution_batch, 8192 problems")


class Fast:
    """What xpoly_amd._capi._lib holds in a child: xpg_create and the entry points of the figure, nothing else."""

    def __init__(self):
        self.fns = {"xpg_create": self.create, "xpg_destroy": lambda h: None, "xpg_last_error": lambda h: b""}

    def __getattr__(self, name):
        try:
            return self.fns[name]
        except KeyError:
            raise AttributeError(name)

    @staticmethod
    def create(out, device):
        out._obj.value = HANDLE
        return 0

    def answer(self, name, fills, view=None):
        """name answers 0 after copying fills[position] into the array behind that argument and pointing the view argument
        (view = (position, buffer)) at the buffer."""
        fills = list(fills.items())
        vpos, vaddr = (view[0], view[1].ctypes.data) if view else (None, None)

        def fn(*args):
            for pos, val in fills:
                args[pos]._arr.reshape(-1)[: val.size] = val
            if vpos is not None:
                args[vpos]._obj.value = vaddr
            return 0
        self.fns[name] = fn


def to_rat(m):
    out = np.ones(m.shape + (2,), dtype=np.int32)
    out[..., 0] = m
    return out


def nest(rng, depth, extra):
    """tools/lab/probe_lineq_ragged.py's loop nest: 2 * depth + extra rows, depth + 1 columns"""
    m = np.zeros((2 * depth + extra, depth + 1), dtype=np.int32)
    for k in range(depth):
        m[2 * k, k] = -1
        m[2 * k + 1, k] = 1
        if k:
            m[2 * k + 1, k - 1] = -1
        m[2 * k + 1, depth] = rng.integers(4, 100)
    for e in range(extra):
        m[2 * depth + e, depth - 1 - e % depth] = 1
        m[2 * depth + e, depth] = rng.integers(4, 100)
    return to_rat(m)


def scop(rng):
    classes = [(d, e) for d in range(2, 7) for e in range(4)]
    return [nest(rng, *classes[(7 * b) % 20]) for b in range(692)]


def figures(fast):
    """{name: a function that prepares the stand-in and returns the call to time}"""
    import xpoly_amd
    from xpoly_amd import six
    from xpoly_amd.lineq import Lineq
    lq = Lineq(xpoly_amd.Context(0))
    ctx = lq.ctx
    rng = np.random.default_rng(9)
    ones = lambda n: np.ones(n, dtype=np.int32)
    buf = lambda cells: np.arange(2 * cells, dtype=np.int32)

    def packed(name, nb, nres_per, pos_view, pos_off, pos_ok, call, rows_per=2):
        def prepare():
            sysm = np.ascontiguousarray(to_rat(rng.integers(-9, 10, size=(nb, 16, 9))))
            nres = nb * nres_per
            off = np.arange(nres + 1, dtype=np.int64) * rows_per
            fast.answer("xpg_lineq_%s_rat32" % name, {pos_off: off, pos_ok: ones(nb)}, (pos_view, buf(nres * rows_per * 9)))
            return lambda: call(sysm)
        return prepare
    el = list(range(7, 0, -1))
    out = {
        "fme_packed, 1 system, copy=False": packed("fme_batch_packed", 1, 1, 11, 12, 13, lambda m: lq.fme_packed(m, 8, 3, copy=False), 8),
        "reduce_packed, 16384 systems, copy=False": packed("reduce_batch_packed", 16384, 1, 9, 10, 12, lambda m: lq.reduce_packed(m, 8, copy=False), 8),
        "fme_packed, 16384 systems, copy=False": packed("fme_batch_packed", 16384, 1, 11, 12, 13, lambda m: lq.fme_packed(m, 8, 3, copy=False), 8),
        "project_packed, 16384 systems, copy=False": packed("project_batch_packed", 16384, 1, 13, 14, 15, lambda m: lq.project_packed(m, 8, el, copy=False)),
        "levels_packed, 16384 systems, copy=False": packed("levels_batch_packed", 16384, 7, 13, 14, 15, lambda m: lq.levels_packed(m, 8, el, copy=False)),
        "levels_packed, 16384 systems, copy=True": packed("levels_batch_packed", 16384, 7, 13, 14, 15, lambda m: lq.levels_packed(m, 8, el)),
    }

    def ragged(name, pos_view, pos_off, pos_ok, nres_of, call):
        def prepare():
            mats = scop(rng)
            if name.startswith("hull"):                         # 346 groups of 2 systems of one class
                arg = [[m, m.copy()] for m in mats[:346]]
                widths = np.array([g[0].shape[1] for g in arg])
                nok = 346
            else:
                arg = mats
                widths = np.repeat([m.shape[1] for m in mats], [nres_of(m) for m in mats])
                nok = 692
            off = np.zeros(widths.size + 1, dtype=np.int64)
            off[1:] = np.cumsum(2 * widths)                     # 2 rows per result, in cells
            fast.answer("xpg_lineq_%s_batch_ragged_rat32" % name, {pos_off: off, pos_ok: ones(nok)}, (pos_view, buf(int(off[-1]))))
            return lambda: call(arg)
        return prepare
    out["levels_ragged, the 692-system SCoP, copy=False"] = ragged("levels", 14, 15, 17, lambda m: m.shape[1] - 2, lambda a: lq.levels_ragged(a, None, copy=False))
    out["bounds_ragged, the 692-system SCoP, copy=False"] = ragged("bounds", 11, 12, 14, lambda m: m.shape[1] - 1, lambda a: lq.bounds_ragged(a, copy=False))
    out["hull_ragged, 346 groups of 2, copy=False"] = ragged("hull", 15, 16, 18, None, lambda a: lq.hull_ragged(a, copy=False))

    def hs_ragged():
        wide = []
        for m in scop(rng):
            w = np.zeros((m.shape[0], 7, 2), dtype=np.int32)
            w[..., 1] = 1
            w[:, : m.shape[1] - 1] = m[:, :-1]
            w[:, 6] = m[:, -1]
            wide.append(w)
        vc = to_rat(np.concatenate([-np.eye(6, dtype=np.int32), np.zeros((6, 1), dtype=np.int32)], axis=1))
        fast.answer("xpg_has_solution_batch_ragged_rat32", {15: ones(692)})
        return lambda: six.has_solution_ragged(ctx, wide, None, vc, False, True)
    out["has_solution_ragged, the 692-system SCoP"] = hs_ragged

    def uniform(which):
        def prepare():
            nb = 8192
            leq = to_rat(rng.integers(-4, 9, size=(nb, 8, 6))); eq = to_rat(rng.integers(-4, 9, size=(nb, 2, 6)))
            tg = to_rat(rng.integers(-4, 9, size=(nb, 6)))
            vc = to_rat(np.concatenate([-np.eye(5, dtype=np.int32), np.zeros((5, 1), dtype=np.int32)], axis=1))
            if which == "six_batch_vc":
                fast.answer("xpg_six_batch_vc_rat32", {11: np.zeros(nb, dtype=np.int32), 12: buf(nb), 13: buf(nb * 6)})
                return lambda: six.six_batch_vc(ctx, six.RAT, True, tg, vc, leq, eq)
            fast.answer("xpg_has_solution_batch_rat32", {13: ones(nb)})
            return lambda: six.has_solution_batch(ctx, leq, eq, vc, False, True)
        return prepare
    out["six_batch_vc, 8192 problems"] = uniform("six_batch_vc")
    out["has_solution_batch, 8192 problems"] = uniform("has_solution_batch")
    return out


def child(name):
    from xpoly_amd import _capi
    fast = Fast()
    _capi._lib = fast
    every = figures(fast)
    assert tuple(every) == NAMES
    call = every[name]()
    for _ in range(5):
        call()
    took = []
    for _ in range(101):
        t0 = time.perf_counter()
        res = call()
        took.append(time.perf_counter() - t0)
        del res
    import xpoly_amd
    print("%s\t%.3f" % (os.path.dirname(os.path.dirname(os.path.abspath(xpoly_amd.__file__))), statistics.median(took) * 1e6))


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2])
    sides = {"parent": os.path.abspath(sys.argv[1]), "tree": ROOT}
    names = NAMES
    got = {"parent": {}, "tree": {}}
    for _ in range(3):
        for side, path in sides.items():
            env = dict(os.environ, PYTHONPATH=path, MALLOC_MMAP_THRESHOLD_=str(1 << 30), MALLOC_TRIM_THRESHOLD_=str(1 << 30))
            for name in names:
                where, us = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], stdout=subprocess.PIPE,
                                           universal_newlines=True, check=True, env=env, cwd="/").stdout.split("\t")
                assert where == path, "the %s side imported xpoly_amd from %s" % (side, where)
                got[side].setdefault(name, []).append(float(us))
    print("# host time of the Python face in front of a stand-in that returns at once; 5 warm-up calls, median of 101, microseconds")
    passed = 0
    for name in names:
        p, t = got["parent"][name], got["tree"][name]
        lo, hi, mid = min(p), max(p), statistics.median(t)
        if mid < lo:
            reading, ok = "below the parent's range", True
        elif mid <= hi:
            reading, ok = "inside the parent's range", True
        else:
            ok = mid - hi <= hi - lo
            reading = "above by %.2f %s width %.2f: %s" % (mid - hi, "<=" if ok else ">", hi - lo, "passes" if ok else "FAILS")
        passed += ok
        print(name)
        print("   parent  medians %s   median %.2f  min %.2f  max %.2f us" % ("  ".join("%.2f" % x for x in p), statistics.median(p), lo, hi))
        print("   tree    medians %s   median %.2f  min %.2f  max %.2f us   %s" % ("  ".join("%.2f" % x for x in t), mid, min(t), max(t), reading))
    print("# %d of %d pass" % (passed, len(names)))


if __name__ == "__main__":
    main()
