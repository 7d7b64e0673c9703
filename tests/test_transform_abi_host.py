"""CPU suite: the faces above the transformed-nest entry points that need a compiler and no device -- include/xpoly_amd.h as
C99 with the new prototypes (tests/cxx/transform_abi_c99.c), and tests/cxx/transform_iter_space.cpp, which puts
xpoly_amd::LoopTran<RMat>::transformIterSpace and xpoly_amd::transform_levels_all to work: linked against the library with stub
matrix and list types (tests/test_gpu_lineq_transform.py runs that binary), and compiled for syntax against the reference's own
RMat and List<RMat*> where its sources lie (read at build time only, as tests/test_callsites_verbatim.py reads them)."""
import os
import shutil
import subprocess

import pytest

import lineq_transform_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src"


def build_iter_space_test():
    from xpoly_amd import build
    build.build()
    exe = os.path.join(ROOT, "tests", "cxx", "transform_iter_space")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "transform_iter_space.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "xpoly_amd"), "-lxpoly_amd", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "xpoly_amd")])
    return exe


def test_the_header_is_c99_with_the_new_prototypes():
    from xpoly_amd import build
    build.build()
    exe = os.path.join(ROOT, "tests", "cxx", "transform_abi_c99")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "transform_abi_c99.c"), "-o", exe,
                           "-L", os.path.join(ROOT, "xpoly_amd"), "-lxpoly_amd", "-Wl,-rpath," + os.path.join(ROOT, "xpoly_amd")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    want = tc.plan(65, 6, 4, 3)
    assert r.stdout.split() == [str(want[k]) for k in tc.PLAN_KEYS], (r.stdout, want)


def test_the_adapter_test_compiles_and_links():
    assert os.path.exists(build_iter_space_test())


@pytest.mark.skipif(not os.path.isdir(REF) or shutil.which("g++") is None, reason="needs the reference sources and g++")
def test_loop_tran_compiles_against_the_references_own_matrix_and_list():
    cmd = ["g++", "-fsyntax-only", "-std=c++17", "-DXPG_REFERENCE_TYPES", "-D_LINUX_", "-Wno-write-strings", "-w",
           "-I", os.path.join(REF, "com"), "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "transform_iter_space.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
