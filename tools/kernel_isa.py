#!/usr/bin/env python3
"""Static VALU instruction counts of one kernel of a HIP source, per basic block, by issue class
(tools/isa_count.py's classes), compiled with the library's flags.

usage: tools/kernel_isa.py <file.hip | file.s> <mangled-substring> [--path FROM[:TAKEN,...]] [extra flags...]

A block starts at a `.LBB` label AND at a `; %bb.N:` comment: the compiler labels only the blocks
something jumps to; a block that is entered by falling out of the one before it (the arm behind a
conditional branch that is usually taken, such as the closed-form PQ fall-backs of the map chain) has
the comment alone, and counted into the preceding block it makes a path look longer than the one the
waves execute. Such blocks are named `%bb.N`.

Without --path every block of MINB (default 40) or more vector instructions is listed; loop bodies
show up as blocks, the caller multiplies by trip counts.

--path FROM[:TAKEN,...] lists only the blocks ONE pass of the code executes, starting at block FROM:
from a block the walk follows an unconditional `s_branch`, follows a conditional branch only if its
target is one of TAKEN, and otherwise falls through into the next block; it ends when it comes back
to FROM (one turn of a loop) or reaches `s_endpgm`. All blocks of the path are printed, whatever
their size, and their sum.

A .s file (hipcc -S --cuda-device-only output) is read as it is; a .hip file is compiled first."""
import collections
import os
import re
import subprocess
import sys
import tempfile
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_count import classify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COST = {"A": 2.5, "B": 4.4, "C": 8.3, "P": 9.5}


def assembly(src, extra):
    if src.endswith(".s"):
        return open(src).read()
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "x.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                               "-fno-slp-vectorize", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-S",
                               src, "-o", out] + extra, stderr=subprocess.DEVNULL)
        return open(out).read()


def parse(dis, pat):
    """-> [(kernel, [block, ...])]; a block is {name, counts, branches: [(op, target)], last}"""
    kernels, cur, blk = [], None, None
    for line in dis.splitlines():
        m = re.match(r"^([.A-Za-z_][A-Za-z_0-9$.]*):", line)
        f = re.match(r"^; (%bb\.\d+):", line)
        if m or f:
            lab = m.group(1) if m else f.group(1)
            if m and not lab.startswith(".L"):
                cur = lab if pat in lab else None
                if cur:
                    kernels.append((cur, []))
            if cur:
                blk = {"name": lab, "counts": collections.Counter(), "branches": [], "last": None}
                kernels[-1][1].append(blk)
            continue
        if not cur or blk is None:
            continue
        if ".end_amdhsa_kernel" in line:
            cur = None
            continue
        m = re.match(r"^\s+([a-z_0-9]+)(\s|$)", line)
        if not m:
            continue
        op, c = m.group(1), blk["counts"]
        blk["last"] = op
        if op.startswith("v_"):
            c[classify(op)] += 1
        elif op.startswith("ds_"):
            c["LDS"] += 1
        elif op.startswith(("global_", "flat_", "buffer_")):
            c["VMEM"] += 1
        elif op.startswith("s_"):
            c["S"] += 1
            if op.startswith("s_cbranch") or op == "s_branch":
                blk["branches"].append((op, line.split()[-1]))
    return kernels


def row(b):
    c = b["counts"]
    valu = c["A"] + c["B"] + c["C"] + c["P"]
    br = " ".join(t for _, t in b["branches"])[:60]
    return ("  %-12s VALU %4d (A %4d B %4d C %3d) ~%5.0f cyc MFMA %3d LDS %3d VMEM %3d S %4d  -> %s" %
            (b["name"][:12], valu, c["A"], c["B"], c["C"], sum(COST[k] * c[k] for k in COST),
             c["M"], c["LDS"], c["VMEM"], c["S"], br))


def walk(blocks, start, taken):
    index = {b["name"]: i for i, b in enumerate(blocks)}
    if start not in index:
        sys.exit("no block %s in this kernel" % start)
    i, path = index[start], []
    while True:
        b = blocks[i]
        path.append(b)
        nxt = i + 1
        for op, target in b["branches"]:
            if op == "s_branch" or target in taken:
                nxt = index[target]
                break
        if b["last"] == "s_endpgm" or nxt >= len(blocks) or nxt == index[start] or len(path) > len(blocks):
            return path
        i = nxt


def main():
    args = sys.argv[1:]
    path = None
    if "--path" in args:
        k = args.index("--path")
        path = args[k + 1]
        del args[k:k + 2]
    src, pat, extra = args[0], args[1], args[2:]
    for name, blocks in parse(assembly(src, extra), pat):
        print(name)
        tot = collections.Counter()
        if path:
            start, _, taken = path.partition(":")
            shown = walk(blocks, start, set(filter(None, taken.split(","))))
        else:
            shown = blocks
        for b in shown:
            c = b["counts"]
            tot.update({k: c[k] for k in "ABCPM"})
            if path or c["A"] + c["B"] + c["C"] + c["P"] + c["M"] >= int(os.environ.get("MINB", "40")):
                print(row(b))
        print("  %s VALU %d (A %d B %d C %d) ~%.0f cyc MFMA %d" %
              ("path" if path else "total", tot["A"] + tot["B"] + tot["C"] + tot["P"], tot["A"], tot["B"], tot["C"],
               sum(COST[k] * tot[k] for k in COST), tot["M"]))


main()
