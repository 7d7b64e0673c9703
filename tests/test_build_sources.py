"""CPU suite: the library's eight sources (xpoly_amd/csrc/api_*.hip) and what build.py derives from them -- a text scan,
no compiler and no device. The include closure of a source is what decides when it is recompiled (build.closure), so a
wrong closure links a stale object; an entry point defined twice or nowhere is a link error minutes into a build.
"""
import os
import re

from xpoly_amd import build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "xpoly_amd", "csrc")
HEADER = os.path.join(REPO, "include", "xpoly_amd.h")
COMMON = {"scalar.hip.h", "ctx.hip.h", "../../include/xpoly_amd.h"}       # what every source includes


def _closure(name):
    src = os.path.join(CSRC, name + ".hip")
    return {os.path.relpath(p, CSRC) for p in build.closure(src)} - {name + ".hip"}


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_include_closures_of_the_smallest_and_the_largest_source():
    # written down by hand from the #include lines, not computed
    assert _closure("api_batch_hbm") == COMMON | {"batch_hbm.hip.h", "batch_kernels.hip.h", "lp_kernels.hip.h", "rat_ops.hip.h",
                                                  "part_instances.hip.h"}
    assert _closure("api_has_solution") == COMMON | {
        "has_solution_batch.hip.h", "has_solution_int.hip.h",
        "six_batch_vc_hbm.hip.h", "six_batch_vc.hip.h", "six_host.hip.h", "batch_hbm.hip.h", "batch_kernels.hip.h", "normalize_dev.hip.h",
        "mip_tree_hbm.hip.h", "mip_host.hip.h", "mip_kernels.hip.h", "lineq_shared.hip.h", "lp_kernels.hip.h", "rat_ops.hip.h",
        "part_instances.hip.h"}


def test_every_source_is_built_and_every_header_is_reached():
    on_disk = sorted(f for f in os.listdir(CSRC) if os.path.isfile(os.path.join(CSRC, f)))
    assert sorted(n + ".hip" for n in build.SOURCES) == [f for f in on_disk if f.endswith(".hip")]
    assert len(build.SOURCES) == 8
    reached = set().union(*(_closure(n) for n in build.SOURCES))
    assert reached - {"../../include/xpoly_amd.h"} == {f for f in on_disk if f.endswith(".hip.h")}
    for n in build.SOURCES:
        assert COMMON <= _closure(n), n


def test_every_declared_entry_point_is_defined_in_exactly_one_source():
    decl = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(xpg_\w+)\s*\(", decl))
    assert len(declared) > 100 and {"xpg_create", "xpg_version", "xpg_stream", "xpg_int_gcd_batch"} <= declared
    where = {}
    for n in build.SOURCES:
        for name in re.findall(r"^(?:int|void|const char \*|void \*) ?(xpg_\w+)\(", _text(n + ".hip"), re.M):
            where.setdefault(name, []).append(n)
    assert {k: v for k, v in where.items() if len(v) != 1} == {}
    assert declared - set(where) == set()
    # the rest are the diagnostic builds' entry points (-DXPG_STAMPS, -DXPG_LIFE), which the header leaves out
    assert all("debug" in name for name in set(where) - declared), sorted(set(where) - declared)


def test_no_part_conditionals_are_left():
    for f in os.listdir(CSRC):
        if os.path.isfile(os.path.join(CSRC, f)):
            text = _text(f)
            assert "XPG_PART" not in text and "XPG_IN(" not in text, f
    for n in build.SOURCES:
        conds = set(re.findall(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b(.*)$", _text(n + ".hip"), re.M))
        assert {c.strip() for c in conds} <= {"XPG_STAMPS", "XPG_LIFE", "XPG_TRACE", "XPG_TEST_HOOKS"}, n
