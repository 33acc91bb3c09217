#!/usr/bin/env python3
"""Are the kernels of this tree the same instructions as those of an earlier commit?

  scripts/isa_identity.py BASE_REV rref.hip rank.hip ... [--tree a.hip b.hip ...] [--pair 'BASE NAME=HEAD NAME']

Compiles each file of rlnc_amd/csrc to gfx950 assembly -- the listed files from `git archive BASE_REV`, and the --tree
files (default: the same list) from the working tree -- and compares every kernel's body as text after normalising its
own symbol and the function index of local labels.  A kernel is paired by name across the whole set of files of each
side, so one that moved to another translation unit is still compared (both file names are printed).
Prints one line per kernel (SGPRs, VGPRs, scratch, static LDS and kernarg bytes of both sides; identical or the differing
lines, with the count of those that lie inside a loop) and exits 1 when any paired kernel differs in its instructions or in a figure other than the kernarg bytes.  A
kernel whose name changed is paired by hand with --pair (demangled names without the namespace).  No GPU needed.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXXFILT = os.environ.get("CXXFILT", "c++filt")
FIGURES = ("TotalNumSgprs", "NumVgprs", "ScratchSize", "LDSByteSize")


def kernels(csrc, name, out):
    """{demangled kernel name: (normalised body lines, figures)} of csrc/name."""
    asm = os.path.join(out, name + ".s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           os.path.join(csrc, name), "-o", asm], stderr=subprocess.DEVNULL)
    lines = open(asm).read().split("\n")
    found = {}
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.type\s+(\S+),@function", lines[i])
        if not m:
            i += 1
            continue
        sym = m.group(1)
        end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
        body = []
        for l in lines[i + 1:end]:
            if l.startswith("\t.section"):  # the kernel descriptor follows the code
                break
            l = l.split(";")[0].rstrip().replace(sym, "KERNEL")
            l = re.sub(r"\.LBB\d+_", ".LBB_", l)
            if l:
                body.append(l)
        figs = {}
        for l in lines[i + 1:end]:
            fm = re.match(r"\s*\.amdhsa_kernarg_size (\d+)", l)
            if fm:
                figs["kernarg"] = int(fm.group(1))
        for l in lines[end:end + 40]:
            fm = re.match(r"; (\w+): (\d+)", l)
            if fm and fm.group(1) in FIGURES:
                figs[fm.group(1)] = int(fm.group(2))
        nice = subprocess.check_output([CXXFILT, sym], text=True).strip()
        nice = re.sub(r"^void ", "", nice).replace("rlnc::(anonymous namespace)::", "").replace("rlnc::", "")
        found[re.sub(r"\(.*\)$", "", nice)] = (body, figs)
        i = end
    return found


def in_loops(body):
    """Indices of the body's lines that lie inside a loop: between a label and a later branch back to it."""
    at = {l[:-1]: i for i, l in enumerate(body) if l.endswith(":")}
    inside = set()
    for i, l in enumerate(body):
        m = re.match(r"\s*s_c?branch\S*\s+(\S+)", l)
        if m and at.get(m.group(1), i) < i:
            inside.update(range(at[m.group(1)], i + 1))
    return inside


def diff_lines(bb, hb, rev):
    """The differing lines ('-' base, '+' tree), and how many of them lie inside a loop of their side."""
    out, looped = [], 0
    bl, hl = in_loops(bb), in_loops(hb)
    for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, bb, hb, autojunk=False).get_opcodes():
        if tag == "equal":
            continue
        out += ["-" + bb[i] for i in range(i1, i2)] + ["+" + hb[j] for j in range(j1, j2)]
        looped += sum(i in bl for i in range(i1, i2)) + sum(j in hl for j in range(j1, j2))
    return out, looped


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("base")
    ap.add_argument("files", nargs="+")
    ap.add_argument("--tree", nargs="+", default=None, help="the working tree's files when they differ from the base's")
    ap.add_argument("--pair", action="append", default=[], help="'BASE NAME=HEAD NAME' of a renamed kernel")
    a = ap.parse_args()
    pairs = dict(p.split("=", 1) for p in a.pair)
    rev = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", a.base], text=True).strip()
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.Popen(["git", "-C", ROOT, "archive", a.base, "rlnc_amd/csrc", "include"], stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", tmp], stdin=tar.stdout)
        tar.wait()
        os.makedirs(os.path.join(tmp, "b"))
        os.makedirs(os.path.join(tmp, "h"))
        base, head = {}, {}  # kernel name: (body, figures, file)
        for f in a.files:
            for n, (b, fg) in kernels(os.path.join(tmp, "rlnc_amd", "csrc"), f, os.path.join(tmp, "b")).items():
                base.setdefault(n, (b, fg, f))
        for f in a.tree or a.files:
            for n, (b, fg) in kernels(os.path.join(ROOT, "rlnc_amd", "csrc"), f, os.path.join(tmp, "h")).items():
                head.setdefault(n, (b, fg, f))
        print("== %s: %s (%d kernels) against the working tree: %s (%d kernels)" %
              (rev, " ".join(a.files), len(base), " ".join(a.tree or a.files), len(head)))
        paired = set()
        for bn in sorted(base, key=lambda n: (base[n][2], n)):
            hn = pairs.get(bn, bn)
            if hn not in head:
                print("  only in %s (%s): %s %s" % (rev, base[bn][2], bn, base[bn][1]))
                continue
            paired.add(hn)
            (bb, bf, bfile), (hb, hf, hfile) = base[bn], head[hn]
            diff, looped = diff_lines(bb, hb, rev)
            same = not diff and {**bf, "kernarg": 0} == {**hf, "kernarg": 0}
            where = bfile if bfile == hfile else "%s -> %s" % (bfile, hfile)
            print("  [%s] %s%s: %d instructions and labels, %s -> %s" %
                  (where, bn, "" if hn == bn else " = " + hn, len(hb), bf, "identical" if same and bf == hf else hf))
            if diff:
                print("      %d differing lines, %d of them inside a loop" % (len(diff), looped))
            for l in diff:
                print("      " + l)
            bad += 0 if same else 1
        for hn in sorted(set(head) - paired):
            print("  only in the working tree (%s): %s %s" % (head[hn][2], hn, head[hn][1]))
    print("differing kernels: %d" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
