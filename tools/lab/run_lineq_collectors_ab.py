"""A/B of the host time inside include/xpoly_amd/lineq.hpp: tests/cxx/collectors_trace.cpp --time built at -O2, without
sanitizers, against the PARENT's include directory and against this tree's, the two programs run alternately (parent, tree,
parent, tree, parent, tree), ONE PROCESS PER COLLECTOR (--time NAME): in one process for all of them a collector's figure depends
on the heap the ones before it left behind (glibc moves its mmap threshold when a large block is freed), by more than the two
sides differ. For the same reason both sides run with MALLOC_MMAP_THRESHOLD_ and MALLOC_TRIM_THRESHOLD_ fixed at 1 GiB, so that
after the warm-up calls no call pays for fresh pages. No device and no library: the stand-ins for the C ABI return at once, so
what is timed is the packing, the class walk, the retry driver and the sinks. Prints, per collector, the three medians of each side in the order they
ran, their median, min and max, and the reading under the rule of profiles/lineq_walks_ab.txt: the tree passes where the median
of its three medians lies inside the range of the parent's three, or above that range by no more than the range's width.
Usage: python tools/lab/run_lineq_collectors_ab.py PARENT_INCLUDE_DIR   (e.g. a `git worktree` of the parent commit, /include)"""
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    parent_inc = sys.argv[1]
    tmp = tempfile.mkdtemp()
    exe = {}
    for side, inc in (("parent", parent_inc), ("tree", os.path.join(ROOT, "include"))):
        exe[side] = os.path.join(tmp, "collectors_trace_" + side)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", inc, os.path.join(ROOT, "tests", "cxx", "collectors_trace.cpp"), "-o", exe[side]])
    env = dict(os.environ, MALLOC_MMAP_THRESHOLD_=str(1 << 30), MALLOC_TRIM_THRESHOLD_=str(1 << 30))
    run = lambda side, *name: subprocess.run([exe[side], "--time"] + list(name), stdout=subprocess.PIPE, universal_newlines=True, check=True,
                                             env=env).stdout.splitlines()
    head = run("tree")
    print("# " + head[0])
    order = [ln.rsplit(None, 1)[0] for ln in head[1:]]
    got = {"parent": {}, "tree": {}}
    for _ in range(3):
        for side in ("parent", "tree"):
            for name in order:
                got[side].setdefault(name, []).append(float(run(side, name)[1].rsplit(None, 1)[1]))
    passed = 0
    for name in order:
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
    print("# %d of %d pass" % (passed, len(order)))


if __name__ == "__main__":
    main()
