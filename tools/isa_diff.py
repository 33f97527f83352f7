#!/usr/bin/env python3
"""Per-kernel comparison of two `hipcc --cuda-device-only -S` outputs of the same translation unit: is each kernel's
instruction stream the same text, and what do the two builds say about its registers, scratch and spills.

    tools/isa_diff.py parent.s new.s [--rename REGEX REPL]... [--memops]

A kernel's stream is the lines between its label and .Lfunc_end with comments, directives, the function number of
.LBB labels and the number of .Lpost_getpc labels (a long branch's own anchor, counted through the whole file) removed
("identical" = the same instructions, registers and operands).  The figures come from the code
object metadata the compiler writes behind the code (.vgpr_count, .sgpr_count, .private_segment_fixed_size,
.vgpr_spill_count, .sgpr_spill_count).  Kernels are paired by demangled name; --rename rewrites the parent's names first
(a template parameter that went away: --rename '(conv_mfma_kernel<(?:[^,]+, ){6})true, ' '\\1').  --memops adds, for the
streams that differ, the counts of global / buffer memory instructions by mnemonic.  Text and metadata only: no
instruction is looked for.  Exit status 1 when a kernel exists on one side only."""
import argparse
import collections
import re
import subprocess
import sys

FIELDS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}
    return {n: short(d) for n, d in zip(names, out)}


def short(d):
    """`void f<1, 2>(ConvK)` -> `f<1, 2>`; the integral-constant spellings of clang shortened"""
    d = re.sub(r"^void ", "", d.strip()).replace("(anonymous namespace)::", "")      # (its bracket is not the argument list's)
    depth = 0
    for i, c in enumerate(d):
        depth += c == "<"
        depth -= c == ">"
        if c == "(" and depth == 0:
            d = d[:i]
            break
    return re.sub(r"\((?:bool|int)\)", "", d)


def parse(path):
    text = open(path).read()
    meta = {}
    m = re.search(r"^\s*\.amdgpu_metadata\n(.*?)^\s*\.end_amdgpu_metadata", text, flags=re.M | re.S)
    for block in re.split(r"^  - ", m.group(1) if m else "", flags=re.M)[1:]:
        name = re.search(r"^\s*\.name:\s*(\S+)", block, flags=re.M)
        if not name or ".kd" not in block:
            continue
        meta[name.group(1)] = {f: int(re.search(r"\.%s:\s*(\d+)" % f, block).group(1)) for f in FIELDS}
    streams = {}
    for name in meta:
        start = re.search(r"^%s:[ \t]*(;.*)?$" % re.escape(name), text, flags=re.M)
        body = text[start.end():text.index(".Lfunc_end", start.end())]
        lines = []
        for l in body.splitlines():
            l = l.split(";")[0].strip()
            if not l or (l.startswith(".") and not l.startswith(".LBB")):
                continue
            lines.append(re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", re.sub(r"\.LBB\d+_", ".LBB_", l)))
        streams[name] = lines
    return meta, streams


def memops(lines):
    c = collections.Counter(l.split()[0] for l in lines if re.match(r"(buffer|global|flat|scratch)_", l))
    return " ".join("%s x%d" % kv for kv in sorted(c.items())) or "-"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("REGEX", "REPL"))
    ap.add_argument("--memops", action="store_true")
    a = ap.parse_args()
    pm, ps = parse(a.parent)
    nm, ns = parse(a.new)
    pd, nd = demangle(list(pm)), demangle(list(nm))
    for rx, repl in a.rename:
        pd = {k: re.sub(rx, repl, v) for k, v in pd.items()}
    new_by_name = {v: k for k, v in nd.items()}
    width = max([len(v) for v in list(pd.values()) + list(nd.values())] + [6])
    print("%-*s  %-9s  %13s  %9s  %9s  %9s  %11s  %11s" % (width, "kernel", "stream", "instr p/n", "VGPR p/n", "SGPR p/n", "scratch B", "VGPR spills", "SGPR spills"))
    differ, missing, same = [], 0, 0
    for pk, name in pd.items():
        nk = new_by_name.pop(name, None)
        if nk is None:
            print("%-*s  only in parent" % (width, name))
            missing += 1
            continue
        ident = ps[pk] == ns[nk]
        same += ident
        if not ident:
            differ.append((name, pk, nk))
        p, n = pm[pk], nm[nk]
        pair = lambda f: "%d/%d" % (p[f], n[f])
        print("%-*s  %-9s  %13s  %9s  %9s  %9s  %11s  %11s" % (width, name, "identical" if ident else "DIFFERS", "%d/%d" % (len(ps[pk]), len(ns[nk])),
                                                           pair("vgpr_count"), pair("sgpr_count"), pair("private_segment_fixed_size"),
                                                           pair("vgpr_spill_count"), pair("sgpr_spill_count")))
    for name in new_by_name:
        print("%-*s  only in new" % (width, name))
        missing += 1
    print("kernels: %d identical, %d differ, %d on one side only" % (same, len(differ), missing))
    if a.memops:
        for name, pk, nk in differ:
            print("\n%s\n  parent memory ops: %s\n  new    memory ops: %s" % (name, memops(ps[pk]), memops(ns[nk])))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
