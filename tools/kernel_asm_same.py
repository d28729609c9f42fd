#!/usr/bin/env python3
"""Are the kernels of one device-assembly file still the same instructions after a change to the sources?

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S -o before.s gaq.hip          (the parent commit)
    hipcc ... -S -o a.s gaq.hip ; ... -o b.s gaq_policy.hip ; ...                      (the units that now hold its kernels)
    python tools/kernel_asm_same.py [--map renames.txt] before.s a.s b.s ...

Per kernel (.globl function) of before.s: its body (label to .Lfunc_end) and its .amdhsa_kernel descriptor, comments stripped and the
function index taken out of local labels (.LBB12_3 -> .LBB_3: it counts the functions in front), compared line by line with the one kernel
of that name in the new files.  Exit status 1 if a kernel differs, is missing from the new files or is defined there more than once.
--map FILE: lines `old new` of kernel names as the source writes them (`policy_mfma_norm_kernel policy_mfma_kernel<PolObsNorm>`,
`policy_mfma_kernel policy_mfma_kernel<>`), or `old -> new` (or a tab between them) where a name has blanks of its own
(`grad_seq_idx_kernel -> grad_seq_kernel<false, true, true>`): a kernel of before.s with the name `old` is compared with the one kernel of the new files
with the name `new` instead of the one with its own symbol -- a kernel that became an instantiation of a template has another mangled
name.  Names come from c++filt, namespaces dropped.  The renamed kernel's symbol is put in place of the new one's before the lines are
compared; bodies and descriptors are compared exactly as without a map.
This is the check behind "every other instantiation stays exactly what it was" (quad_core.hpp, mfma_layer's Kernel parameter).
"""
import re
import subprocess
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


def names(symbols):
    """{symbol: its kernel's name as the source writes it, template arguments included, namespaces and parameters dropped}"""
    out = subprocess.run(["c++filt"], input="\n".join(symbols), capture_output=True, text=True, check=True).stdout.split("\n")
    short = {}
    for sym, full in zip(symbols, out):
        full = re.sub(r"\(anonymous namespace\)::|\b\w+::", "", full)
        short[sym] = re.sub(r"^void ", "", full[:full.index("(")] if "(" in full else full)
    return short


def main(argv):
    renames = {}
    if len(argv) > 2 and argv[1] == "--map":
        renames = dict(tuple(n.strip() for n in re.split(r"\t| -> ", l, 1)) if re.search(r"\t| -> ", l) else l.split()
                       for l in open(argv[2]) if l.strip() and not l.startswith("#"))
        argv = argv[:1] + argv[3:]
    if len(argv) < 3:
        sys.exit(__doc__)
    new = [k for path in argv[2:] for k in kernels(path)]
    old = kernels(argv[1])
    name = names([s for s, _ in old + new]) if renames else {}
    bad = 0
    for sym, lines in old:
        if name.get(sym) in renames:                                  # the one kernel of that name, under this kernel's symbol
            twins = [[l.replace(s, sym) for l in ls] for s, ls in new if name[s] == renames[name[sym]]]
        else:
            twins = [l for s, l in new if s == sym]
        if len(twins) != 1:
            verdict = "MISSING" if not twins else "DEFINED %d TIMES" % len(twins)
        else:
            ndiff = sum(a != b for a, b in zip(lines, twins[0])) + abs(len(lines) - len(twins[0]))
            verdict = "same (%d lines)" % len(lines) if ndiff == 0 else "DIFFERS in %d of %d lines" % (ndiff, len(lines))
        bad += not verdict.startswith("same")
        print("%-18s %s" % (verdict, sym))
    print("%d kernels of %s, %d not the same" % (len(old), argv[1], bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
