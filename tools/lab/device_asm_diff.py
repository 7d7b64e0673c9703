"""Device assembly of two sources, function by function: what a refactor that must not move the device code is checked with.

    python tools/lab/device_asm_diff.py A.hip B.hip [--a-flags="-DX=1 ..."] [--b-flags="..."] [--keep DIR]

Each source is compiled for gfx950 with the library's flags (xpoly_amd/build.py CFLAGS) plus
`--cuda-device-only -S -Rpass-analysis=kernel-resource-usage`, the two side by side. The text is stripped as
profiles/vc_kernels_shared_isa.txt describes -- comments, .loc / .file / .cfi lines, .Ltmp labels and the __hip_cuid_* symbol
go; the function index in .LBB<fn>_<n>, .Lfunc_begin<fn> / .Lfunc_end<fn> and the counter in .Lpost_getpc<n> go (they only
number the labels) -- and split per function (.type NAME,@function up to its .size); what lies outside the functions (kernel
descriptors, metadata) is compared as one more piece. Reported: the functions only one side has, the functions whose text
differs, and the compiler's resource notes of every kernel side by side where they differ (or all of them with --notes).
It compares text and looks for nothing in particular. Exit status 0 when nothing differs. No GPU is needed.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from xpoly_amd.build import CFLAGS  # noqa: E402

OUTSIDE = "(outside the functions)"


def compile_asm(src, flags, out):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc] + CFLAGS + flags + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", out]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, universal_newlines=True)
    if r.returncode:
        sys.exit("failed: %s\n%s" % (" ".join(cmd), r.stderr[-4000:]))
    return " ".join(cmd), r.stderr


def strip(text):
    out = []
    for ln in text.split("\n"):
        ln = ln.split(";", 1)[0].rstrip()
        s = ln.strip()
        if not s or s.startswith((".loc", ".file", ".cfi_")) or re.match(r"\.Ltmp\d+:", s) or "__hip_cuid_" in s:
            continue
        ln = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", ln)
        ln = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", ln)
        out.append(re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", ln))
    return out


def split(lines):
    fns, cur = {OUTSIDE: []}, OUTSIDE
    for ln in lines:
        m = re.match(r"\s*\.type\s+(\S+),@function", ln)
        if m:
            cur = m.group(1)
            assert cur not in fns, cur
            fns[cur] = []
        fns[cur].append(ln)
        if cur != OUTSIDE and re.match(r"\s*\.size\s+%s," % re.escape(cur), ln):
            cur = OUTSIDE
    return fns


def notes(stderr):
    """{function: {figure: value}} from the kernel-resource-usage remarks."""
    out, cur = {}, None
    for ln in stderr.split("\n"):
        m = re.search(r"remark:\s+([^:]+): (.*?)\s*\[-Rpass-analysis", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--a-flags", default="")
    ap.add_argument("--b-flags", default="")
    ap.add_argument("--keep", help="directory the two .s files and remark logs are left in")
    ap.add_argument("--notes", action="store_true", help="print every kernel's resource notes, not only those that differ")
    o = ap.parse_args()
    d = o.keep or tempfile.mkdtemp(prefix="asmdiff_")
    os.makedirs(d, exist_ok=True)
    with ThreadPoolExecutor(max_workers=2) as ex:
        ja = ex.submit(compile_asm, o.a, o.a_flags.split(), os.path.join(d, "a.s"))
        jb = ex.submit(compile_asm, o.b, o.b_flags.split(), os.path.join(d, "b.s"))
        (cmd_a, err_a), (cmd_b, err_b) = ja.result(), jb.result()
    print("A: " + cmd_a)
    print("B: " + cmd_b)
    side = []
    for name, err in (("a", err_a), ("b", err_b)):
        with open(os.path.join(d, name + ".s")) as f:
            lines = strip(f.read())
        with open(os.path.join(d, name + ".remarks"), "w") as f:
            f.write(err)
        side.append((len(lines), split(lines), notes(err)))
    (na, fa, ra), (nb, fb, rb) = side
    only_a, only_b = sorted(set(fa) - set(fb)), sorted(set(fb) - set(fa))
    differ = sorted(k for k in set(fa) & set(fb) if fa[k] != fb[k])
    notes_differ = sorted(k for k in set(ra) | set(rb) if ra.get(k) != rb.get(k))
    print("stripped lines A %d, B %d; functions A %d, B %d; only in A %d, only in B %d; text differs %d; kernels with resource notes A %d, B %d, "
          "differing %d" % (na, nb, len(fa) - 1, len(fb) - 1, len(only_a), len(only_b), len(differ), len(ra), len(rb), len(notes_differ)))
    for k in only_a:
        print("   only in A: " + k)
    for k in only_b:
        print("   only in B: " + k)
    for k in differ:
        sa, sb = set(fa[k]), set(fb[k])
        print("   text differs: %s (%d / %d lines; A-only %d, B-only %d)" % (k, len(fa[k]), len(fb[k]), len(sa - sb), len(sb - sa)))
    for k in (sorted(set(ra) | set(rb)) if o.notes else notes_differ):
        print("   notes %s %s" % ("SAME" if ra.get(k) == rb.get(k) else "DIFFER", k))
        for tag, r in (("A", ra.get(k)), ("B", rb.get(k))):
            print("      %s: %s" % (tag, ", ".join("%s %s" % kv for kv in r.items()) if r else "-"))
    if not o.keep:
        shutil.rmtree(d)
    return 1 if only_a or only_b or differ or notes_differ else 0


if __name__ == "__main__":
    sys.exit(main())
