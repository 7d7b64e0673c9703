"""Builds xpoly_amd/libxpoly_amd.so for gfx950 with hipcc (cross-compiles without a GPU).

-ffp-contract=off is part of the numerical contract, not a tuning flag: the
reference rounds after the multiply and again after the add (lpsol.h:1485-1489).

The library is ONE shared object linked from eight sources compiled side by side, each
holding the C entry points of one subsystem and including only the kernel headers they
launch: the device code of all kernels in one translation unit took 4.7 minutes, the
eight take about the time of the largest.
  api_core          handle, K1 pivot, the device-resident LP (every loop of lp_*.hip.h), warm-started MIP, test and debug hooks
  api_six           SIX::maxm / minm, the LDS-resident LP batches (k_batch), their multi-device and ragged forms
  api_mip           MIP (device tree walk + host controller), has_solution, DepPoly::is_empty front end
  api_lineq         rational / integer row elimination (Lineq, rank / det / inv / null, hnf, gcd)
  api_batch_hbm     LP batches beyond one CU's LDS (k_batch_hbm)
  api_six_vc_hbm    the same with equalities and free variables (k_six_batch_vc_hbm)
  api_mip_hbm       MIP tree walks whose node LPs are beyond 64 KB of LDS (k_mip_tree_hbm)
  api_has_solution  batched has_solution, its forms for mixed shapes and its integer form on the device
Template instances that one source compiles and another calls: csrc/part_instances.hip.h.
"""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libxpoly_amd.so")
OBJ = os.path.join(HERE, "csrc", "_obj")
# the same sources with -DXPG_TEST_HOOKS: fault injection, forced routes and debug prints are compiled in (scalar.hip.h
# xpg_hook). Loaded only by the tests that need a hook (tests/conftest.py needs_hooks) and by tools/lab.
HOOKS_OUT = os.path.join(HERE, "libxpoly_amd_hooks.so")
HOOKS_OBJ = os.path.join(HERE, "csrc", "_obj", "hooks")
CFLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-std=c++17"]
SOURCES = ["api_core", "api_six", "api_mip", "api_lineq", "api_batch_hbm", "api_six_vc_hbm", "api_mip_hbm", "api_has_solution"]


def closure(path):
    """The file and every file its #include "..." lines reach: a source is recompiled when one of them is newer than its object."""
    seen, todo = set(), [os.path.normpath(path)]
    while todo:
        p = todo.pop()
        if p not in seen:
            seen.add(p)
            todo += [os.path.normpath(os.path.join(os.path.dirname(p), m)) for m in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', open(p).read(), re.M)]
    return seen


def sources():
    inc = os.path.join(HERE, "..", "include", "xpoly_amd.h")
    return [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, f))] + [inc]


def stale(out=OUT):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(s) > t for s in sources())


def build_hooks(force=False):
    """xpoly_amd/libxpoly_amd_hooks.so (-DXPG_TEST_HOOKS)."""
    if not force and not stale(HOOKS_OUT):
        return HOOKS_OUT
    return build(force=force, extra=["-DXPG_TEST_HOOKS"], out=HOOKS_OUT, obj=HOOKS_OBJ)


def build_all(force=False):
    """The product library and the test-hooks variant, compiled side by side."""
    with ThreadPoolExecutor(max_workers=2) as ex:
        a = ex.submit(build, force)
        b = ex.submit(build_hooks, force)
        return a.result(), b.result()


def build(force=False, extra=(), out=None, obj=None):
    """force: recompile every source whatever the time stamps say (what __graft_entry__.build() asks for:
    the driver's build step proves the source, it does not re-link yesterday's objects).
    out / obj: another library path and object directory (diagnostic builds: -DXPG_STAMPS, -DXPG_LIFE)."""
    if out is None and not force and not stale():
        return OUT
    OUT_ = out or OUT
    OBJ_ = obj or OBJ
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    extra = list(extra) + os.environ.get("XPG_BUILD_FLAGS", "").split()
    os.makedirs(OBJ_, exist_ok=True)
    srcs = [os.path.join(CSRC, n + ".hip") for n in SOURCES]
    objs = [os.path.join(OBJ_, n + ".o") for n in SOURCES]

    flags_key = " ".join(CFLAGS + extra)
    key_file = os.path.join(OBJ_, "flags.txt")
    same_flags = os.path.exists(key_file) and open(key_file).read() == flags_key

    def one(k):
        fresh = not force and same_flags and os.path.exists(objs[k])
        if not fresh or any(os.path.getmtime(f) > os.path.getmtime(objs[k]) for f in closure(srcs[k])):
            subprocess.check_call([hipcc] + CFLAGS + extra + ["-c", srcs[k], "-o", objs[k]])

    with ThreadPoolExecutor(max_workers=len(SOURCES)) as ex:
        list(ex.map(one, range(len(SOURCES))))
    with open(key_file, "w") as f:
        f.write(flags_key)
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", OUT_] + objs)
    return OUT_


if __name__ == "__main__":
    import sys
    # `python -m xpoly_amd.build` recompiles the sources that changed, or that include a header that did; `--force` all of them
    if "--hooks" in sys.argv[1:]:
        print(build_hooks(force="--force" in sys.argv[1:]))
    elif "--product" in sys.argv[1:]:
        print(build(force="--force" in sys.argv[1:]))
    else:
        print(*build_all(force="--force" in sys.argv[1:]))
