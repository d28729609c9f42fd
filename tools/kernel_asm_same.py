#!/usr/bin/env python3
"""Are the kernels of one device-assembly file still the same instructions after a change to the sources?

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S -o before.s gaq.hip          (the parent commit)
    hipcc ... -S -o a.s gaq.hip ; ... -o b.s gaq_policy.hip ; ...                      (the units that now hold its kernels)
    python tools/kernel_asm_same.py before.s a.s b.s ...

Per kernel (.globl function) of before.s: its body (label to .Lfunc_end) and its .amdhsa_kernel descriptor, comments stripped and the
function index taken out of local labels (.LBB12_3 -> .LBB_3: it counts the functions in front), compared line by line with the one kernel
of that name in the new files.  Exit status 1 if a kernel differs, is missing from the new files or is defined there more than once.
This is the check behind "every other instantiation stays exactly what it was" (quad_core.hpp, mfma_layer's Kernel parameter).
"""
import re
import sys


def kernels(path):
    """{symbol: [normalised lines of its body + its kernel descriptor]} of one assembly file, in a list of (symbol, lines)"""
    text = open(path).read()
    found = []
    for sym in re.findall(r"^\s*\.globl\s+(\S+)", text, re.M):
        body = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(sym), text, re.M | re.S)
        desc = re.search(r"^\s*\.amdhsa_kernel %s$.*?\.end_amdhsa_kernel" % re.escape(sym), text, re.M | re.S)
        if not body or not desc:
            continue                                                  # a .globl object that is no kernel (__hip_cuid_...)
        lines = [re.sub(r"\s+", " ", l.split(";")[0]).strip() for l in (body.group(0) + "\n" + desc.group(0)).split("\n")]
        found.append((sym, [re.sub(r"(\.L[A-Za-z_]+?)\d+(_\d+|:)", r"\1\2", l) for l in lines if l]))
    return found


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    new = [k for path in argv[2:] for k in kernels(path)]
    bad = 0
    for sym, lines in kernels(argv[1]):
        twins = [l for s, l in new if s == sym]
        if len(twins) != 1:
            verdict = "MISSING" if not twins else "DEFINED %d TIMES" % len(twins)
        else:
            ndiff = sum(a != b for a, b in zip(lines, twins[0])) + abs(len(lines) - len(twins[0]))
            verdict = "same (%d lines)" % len(lines) if ndiff == 0 else "DIFFERS in %d of %d lines" % (ndiff, len(lines))
        bad += not verdict.startswith("same")
        print("%-18s %s" % (verdict, sym))
    print("%d kernels of %s, %d not the same" % (len(kernels(argv[1])), argv[1], bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
