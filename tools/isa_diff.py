#!/usr/bin/env python3
"""Compare the device assembly of two builds of one HIP unit, kernel by kernel.

usage: tools/isa_diff.py <before.s> <after.s>        (hipcc -S --cuda-device-only output)

Comment lines, directives and trailing comments are dropped. Per function, one of
  identical   the same instructions with the same operands in the same order
  reordered   the same number of instructions and, block by block in order (blocks as
              tools/kernel_isa.py draws them: `.LBB` labels and `; %bb.N:` comments), the same sorted
              list of mnemonics: the compiler moved independent instructions or renamed registers
              inside a block and did nothing else. The number of differing lines is printed.
  CHANGED     anything else (also: a function that only one of the files has)
Exit status 1 if any function is CHANGED."""
import difflib
import re
import sys


def functions(path):
    """-> {name: [block, ...]}, a block a list of instruction lines"""
    out, cur = {}, None
    for line in open(path):
        if ".amdgpu_metadata" in line:      # (the code object's notes: no code behind it)
            break
        m = re.match(r"^([.A-Za-z_][A-Za-z_0-9$.]*):", line)
        f = re.match(r"^; (%bb\.\d+):", line)
        if m and not m.group(1).startswith(".L"):
            cur = out.setdefault(m.group(1), [[]])
        elif (m or f) and cur is not None:
            cur.append([])
        elif cur is not None:
            if ".end_amdhsa_kernel" in line or re.match(r"^\s+\.(section|text)\b", line):
                cur = None
                continue
            ins = line.split(";")[0].strip()
            if ins and not ins.startswith("."):
                cur[-1].append(" ".join(ins.split()))
    return {k: v for k, v in out.items() if any(v)}


def verdict(a, b):
    fa, fb = [i for blk in a for i in blk], [i for blk in b for i in blk]
    if fa == fb:
        return "identical", 0
    ndiff = sum(1 for d in difflib.unified_diff(fa, fb, "a", "b", n=0, lineterm="")
                if d[0] in "+-" and not d.startswith(("+++", "---")))
    same = len(a) == len(b) and all(sorted(i.split()[0] for i in x) == sorted(i.split()[0] for i in y)
                                    for x, y in zip(a, b))
    return ("reordered" if same else "CHANGED"), ndiff


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    tally = {"identical": 0, "reordered": 0, "CHANGED": 0}
    for name in sorted(set(a) | set(b)):
        v, n = verdict(a[name], b[name]) if name in a and name in b else ("CHANGED", -1)
        tally[v] += 1
        if v != "identical":
            print("%-9s %6d differing lines, %d -> %d instructions  %s" %
                  (v, n, sum(map(len, a.get(name, []))), sum(map(len, b.get(name, []))), name))
    print("%d functions: %d identical, %d reordered, %d changed" %
          (sum(tally.values()), tally["identical"], tally["reordered"], tally["CHANGED"]))
    sys.exit(1 if tally["CHANGED"] else 0)


if __name__ == "__main__":
    main()
