"""CPU suite: what the C++ collectors of include/xpoly_amd/lineq.hpp do, seen from below. tests/cxx/collectors_trace.cpp defines
every xpg_* entry point the header calls itself -- scripted stand-ins that print their arguments and answer 1, 0, -need or a
return code -- so the header is compiled and run under the address and undefined-behaviour sanitizers without the library and
without a device. Its output is compared line for line with tests/golden/g15_collectors_trace.txt, recorded from this project's
own header before the collectors' shared parts (the pack, the class walk, the retry rule, the sink) were stated once. The facts
the record rests on are asserted here in words as well: how many library calls each retry scenario makes, and that a call that
is never satisfied ends in XPG_ERR_UNSUPPORTED (false for the members), never in a silent empty result."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g15_collectors_trace.txt")

# the attempt limit of each retry loop, as lineq.hpp's comments promise it
LIMITS = {"Lineq::calcBound": 2, "Lineq::fmeLevels": 4, "project_all": 3, "levels_all": 4, "project_each": 4, "levels_nests": 4,
          "calc_bound_all": 3, "calc_bound_each": 3, "hull_all": 3, "project_union_each": 3}
MEMBERS = ("Lineq::calcBound", "Lineq::fmeLevels")
HULLS = ("hull_all", "project_union_each")


@pytest.fixture(scope="module")
def trace(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("collectors") / "collectors_trace")
    # the sanitizers' runtimes are linked into the program itself: it needs nothing from its environment
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-static-libasan",
                           "-static-libubsan", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "collectors_trace.cpp"),
                           "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]           # the sanitizers report nothing
    return run.stdout.splitlines()


def scenarios(lines):
    """{name: (lines between "== name" and "calls n", n)}"""
    out, name, body = {}, None, []
    for ln in lines:
        if ln.startswith("== "):
            assert name is None, ln
            name, body = ln[3:], []
        elif ln.startswith("calls "):
            assert name is not None and name not in out, ln
            out[name] = (body, int(ln.split()[1]))
            name = None
        else:
            body.append(ln)
    assert name is None
    return out


def test_the_trace_is_the_recorded_one(trace):
    want = open(GOLDEN).read().splitlines()
    for k, (g, w) in enumerate(zip(trace, want)):
        assert g == w, "line %d" % (k + 1)
    assert len(trace) == len(want)


def test_the_record_counts_the_calls_it_should():
    sc = scenarios(open(GOLDEN).read().splitlines())
    calls = lambda body: [ln for ln in body if ln.startswith("  call ")]
    for body, n in sc.values():
        assert len(calls(body)) == n
    for loop, limit in LIMITS.items():
        want = {"answered at once": 1, "a step short (need > cap)": 2, "a slot short (need <= cap)": 2,
                "a step short, then a slot": min(3, limit), "never satisfied": limit, "a return code on the second call": 2}
        if loop not in MEMBERS:
            want["both in one call"] = 2                           # the two needs are read out of ONE answer
        if loop in HULLS:
            want["a group short (member -1)"] = 2
            want["a member and a group short"] = 2
        assert {run: sc[loop + ": " + run][1] for run in want} == want, loop
        # never satisfied: exactly the loop's own number of calls, then XPG_ERR_UNSUPPORTED -- false for the members
        body = sc[loop + ": never satisfied"][0]
        verdicts = [ln for ln in body if ln.startswith("  rc ") or ln.startswith("  returns ")]
        assert verdicts == ["  returns false" if loop in MEMBERS else "  rc -4 XPG_ERR_UNSUPPORTED"], loop
        # a return code on the second call is passed through at once
        body = sc[loop + ": a return code on the second call"][0]
        assert calls(body)[1].endswith("-> -1")
        assert [ln for ln in body if ln.startswith("  rc ") or ln.startswith("  returns ")] == ["  returns false" if loop in MEMBERS else "  rc -1"]
    # the class walk: one call per class in order of first appearance, members in the caller's order, the empty system answered
    # without a call -- but refused by calc_bound_all, and only after the earlier classes were called
    for name in ("project_all", "levels_all"):
        body, n = sc["class walk: %s over A B A empty B A" % name]
        assert n == 2 and "nb=3 rows=3 cols=4" in body[0] and "nb=2 rows=5 cols=3" in body[1]
        assert "  rc 0" in body and "  ok=[1,1,0,1,1,1]" in body    # the script fails member 1 of the first class: system 2
    body, n = sc["class walk: calc_bound_all over A B A empty B A refuses the empty system when its class comes up"]
    assert n == 2 and "  rc -3 XPG_ERR_SHAPE" in body
    body, n = sc["class walk: calc_bound_all, equal shapes and different rhs_idx are two classes"]
    assert n == 2 and "nb=2 rows=3 cols=4 rhs=3" in body[0] and "nb=1 rows=3 cols=4 rhs=2" in body[1]
    assert sc["class walk: refusals before any call"][1] == 0
    assert sc["has_solution_all: every refusal is made before any call"][1] == 0
    # fme_all above 64 MiB of worst case: a call without outs, answered XPG_ERR_SHAPE with a total, then one with exactly that room
    body, n = sc["fme_all: above 64 MiB of worst case a sizing call, then one with exactly that many cells"]
    first, second = calls(body)
    total = int(re.search(r" total=(\d+) -> -3$", first).group(1))
    assert n == 2 and " outs=0/0 " in first and total > 0 and (" outs=1/%d " % total) in second + " "
    assert sc["has_solution_all: the plain call"][0][0].split()[2] == "has_solution_batch_ragged"
    assert sc["has_solution_all: the integer call"][0][0].split()[2] == "has_solution_int_batch_ragged"
