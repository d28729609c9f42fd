#!/usr/bin/env python
"""kernarg_touch.py -- in what order a kernel first touches the 64-byte lines of its kernel-argument segment.

Every launch gets a fresh argument slot, so the first wave of a CU that reads an argument line misses the scalar cache (and L2), and
every `s_waitcnt lgkmcnt(0)` that stands between two first touches is one more exposed round trip at the start of the launch.  This
tool reads the gfx950 code objects out of libgaq.so (or out of the objects under build/obj), disassembles one kernel with the ROCm
llvm-objdump and walks its text in layout order -- the fall-through path; branches are not followed -- printing

  * every scalar load from the argument segment (offset, width, the lines it covers, which of them are new),
  * every scalar wait (`s_waitcnt` with an lgkmcnt field) and what it waits for: `kernarg` (argument loads issued since the last
    wait), `deref` (a load through a pointer that itself came out of the arguments is among them, e.g. the graph-safe `*step_ctr`),
    `other` (no scalar load outstanding: LDS traffic, or a second wait right behind the first),
  * the position of the first `buffer_load ... lds` (the first LDS-DMA state load),

and a summary: argument lines in order of first touch, the scalar waits before the first DMA, the lines first touched after them.

    python tools/kernarg_touch.py 'step_kernel<148>' 'rollout_kernel<20>'            # the built library
    python tools/kernarg_touch.py --lib build/obj/gaq_inst4.o 'step_kernel<148>'

Only `s_load_*`, `s_waitcnt`, the instructions that derive a second base from the argument pointer (`s_add_u32` / `s_addc_u32` /
`s_mov_b64`) and the `lds` marker of a buffer load are interpreted.  The argument pointer is taken to be the base of the kernel's
first scalar load (hipcc reads arguments before anything else it could dereference).
"""
import argparse
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "gym_art_amd", "libgaq.so")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
LINE = 64


def find_objdump():
    for c in (os.environ.get("LLVM_OBJDUMP"), "/opt/rocm/llvm/bin/llvm-objdump", shutil.which("llvm-objdump")):
        if c and os.path.exists(c):
            return c
    return None


def code_objects(path, arch="gfx950"):
    """The device code objects for `arch` inside a host object / shared library: every uncompressed clang offload bundle found in
    the file, as a list of bytes objects.  (A file that is itself an AMDGPU ELF is returned as it is.)"""
    data = open(path, "rb").read()
    out = []
    pos = data.find(MAGIC)
    if pos < 0 and data[:4] == b"\x7fELF":
        return [data]
    while pos >= 0:
        (count,) = struct.unpack_from("<Q", data, pos + len(MAGIC))
        q = pos + len(MAGIC) + 8
        for _ in range(count):
            off, size, idlen = struct.unpack_from("<QQQ", data, q)
            ident = data[q + 24:q + 24 + idlen].decode("ascii", "replace")
            q += 24 + idlen
            if ident.startswith("hip") and ident.endswith(arch) and size:
                out.append(data[pos + off:pos + off + size])
        pos = data.find(MAGIC, pos + len(MAGIC))
    return out


def mangled_prefix(kernel):
    """'step_kernel<148>' -> '_ZN4gaqk11step_kernelILj148EE' (the kernels live in namespace gaqk and take one uint32_t mask)."""
    m = re.fullmatch(r"\s*(\w+)\s*<\s*(\d+)u?\s*>\s*", kernel)
    if not m:
        raise ValueError("kernel name must look like step_kernel<148>: %r" % kernel)
    return "_ZN4gaqk%d%sILj%sEE" % (len(m.group(1)), m.group(1), m.group(2))


def disassemble(kernel, lib=DEFAULT_LIB, objdump=None):
    """Text of the kernel's disassembly (llvm-objdump -d), or None when no code object of `lib` defines it."""
    objdump = objdump or find_objdump()
    if objdump is None:
        raise FileNotFoundError("llvm-objdump")
    prefix = mangled_prefix(kernel)
    with tempfile.TemporaryDirectory() as tmp:
        for k, blob in enumerate(code_objects(lib)):
            if prefix.encode() not in blob:
                continue
            co = os.path.join(tmp, "co%d.elf" % k)
            with open(co, "wb") as f:
                f.write(blob)
            syms = subprocess.run([objdump, "-t", co], check=True, capture_output=True, text=True).stdout
            names = [ln.split()[-1] for ln in syms.splitlines() if prefix in ln and " F " in ln and not ln.rstrip().endswith(".kd")]
            if not names:
                continue
            return subprocess.run([objdump, "-d", "--no-show-raw-insn", "--disassemble-symbols=" + names[0], co], check=True,
                                  capture_output=True, text=True).stdout
    return None


_SREG = re.compile(r"s\[(\d+):(\d+)\]|s(\d+)")
_WIDTH = {"dword": 4, "dwordx2": 8, "dwordx3": 12, "dwordx4": 16, "dwordx8": 32, "dwordx16": 64}


def _first(reg):
    m = _SREG.fullmatch(reg.strip())
    if not m:
        return None
    return int(m.group(1)) if m.group(1) is not None else int(m.group(3))


def _span(reg):
    m = _SREG.fullmatch(reg.strip())
    if not m:
        return None, 0
    if m.group(1) is not None:
        return int(m.group(1)), int(m.group(2)) - int(m.group(1)) + 1
    return int(m.group(3)), 1


def _imm(tok):
    tok = tok.strip()
    try:
        return int(tok, 0)
    except ValueError:
        return None


def parse(text):
    """Walk a kernel's disassembly in layout order.  Returns a dict:
      events: list of (index, kind, detail) with kind in {'load', 'wait', 'dma'}
      order: argument lines in order of first touch
      first_dma: instruction index of the first LDS-DMA load (None if the kernel has none)
      waits_before_dma: {'kernarg': n, 'deref': n, 'other': n}
      late_lines: argument lines first touched after the first kernarg wait
      lines_after_dma: argument lines first touched after the first LDS-DMA load"""
    insns = []
    for ln in text.splitlines():
        ln = ln.split("//")[0].strip()
        if not ln or ln.endswith(":") or ln.startswith("Disassembly") or "file format" in ln:
            continue
        insns.append(ln)
    bases = {}            # first SGPR of a 64-bit pair -> byte offset from the argument pointer
    half = {}             # s_add_u32 seen, waiting for its s_addc_u32: dst lo -> (src lo, offset)
    events, order, seen = [], [], set()
    pending_kernarg = pending_deref = 0
    base_known = False
    first_dma = None
    first_kernarg_wait = None
    waits_before_dma = {"kernarg": 0, "deref": 0, "other": 0}
    late, after_dma = [], []
    for idx, ins in enumerate(insns):
        parts = ins.split(None, 1)
        op = parts[0]
        args = [a.strip() for a in parts[1].split(",")] if len(parts) > 1 else []
        if op.startswith("s_load_") and len(args) >= 3:
            width = _WIDTH.get(op[len("s_load_"):])
            base = _first(args[1])
            off = _imm(args[2].split()[0])
            if not base_known and base is not None:
                bases[base] = 0                                  # the kernel's first scalar load reads the arguments
                base_known = True
            dst, n = _span(args[0])
            if base in bases and width is not None and off is not None:
                o = bases[base] + off
                lines = list(range(o // LINE, (o + width - 1) // LINE + 1))
                new = [l for l in lines if l not in seen]
                for l in new:
                    seen.add(l)
                    order.append(l)
                    if first_kernarg_wait is not None:
                        late.append(l)
                    if first_dma is not None:
                        after_dma.append(l)
                events.append((idx, "load", {"offset": o, "bytes": width, "lines": lines, "new": new}))
                pending_kernarg += 1
            else:
                events.append((idx, "load", {"offset": None, "bytes": width, "lines": [], "new": [], "text": ins}))
                pending_deref += 1
            if dst is not None:
                for r in range(dst, dst + n):                    # the destination no longer holds a base
                    bases.pop(r, None)
                    bases.pop(r - 1, None)
            continue
        if op == "s_waitcnt":
            if "lgkmcnt" in ins:
                kind = "deref" if pending_deref else "kernarg" if pending_kernarg else "other"
                events.append((idx, "wait", {"kind": kind, "text": ins}))
                if first_dma is None:
                    waits_before_dma[kind] += 1
                if kind == "kernarg" and first_kernarg_wait is None:
                    first_kernarg_wait = idx
                pending_kernarg = pending_deref = 0
            continue
        if op.startswith("buffer_load_") and re.search(r"\blds\b", ins):
            if first_dma is None:
                first_dma = idx
                events.append((idx, "dma", {"text": ins}))
            continue
        # bases derived from the argument pointer: s_mov_b64 d, s | s_add_u32 d.lo, s.lo, imm + s_addc_u32 d.hi, s.hi, 0
        if op == "s_mov_b64" and len(args) == 2:
            d, s = _first(args[0]), _first(args[1])
            if s in bases and d is not None:
                bases[d] = bases[s]
                continue
        if op == "s_add_u32" and len(args) == 3:
            d, s, k = _first(args[0]), _first(args[1]), _imm(args[2])
            if s in bases and k is not None and d is not None:
                half[d] = (s, bases[s] + k)
                if d == s:
                    bases.pop(s)
                continue
        if op == "s_addc_u32" and len(args) == 3:
            d, k = _first(args[0]), _imm(args[2])
            if d is not None and d - 1 in half and k == 0:
                bases[d - 1] = half.pop(d - 1)[1]
                continue
        # any other scalar instruction that writes a tracked pair drops it
        if op.startswith("s_") and args:
            d, n = _span(args[0])
            if d is not None:
                for r in range(d, d + n):
                    bases.pop(r, None)
                    if r - 1 in bases:
                        bases.pop(r - 1)
                    half.pop(r, None)
    return {"events": events, "order": order, "first_dma": first_dma, "waits_before_dma": waits_before_dma,
            "late_lines": late, "lines_after_dma": after_dma, "instructions": len(insns)}


def report(kernel, res, out=sys.stdout):
    w = out.write
    w("== %s: %d instructions\n" % (kernel, res["instructions"]))
    for idx, kind, d in res["events"]:
        if kind == "load":
            if d["offset"] is None:
                w("  %6d  s_load through a loaded pointer (%s B)\n" % (idx, d["bytes"]))
            else:
                w("  %6d  s_load  0x%03x +%-2d lines %-8s new %s\n" % (idx, d["offset"], d["bytes"], ",".join(map(str, d["lines"])),
                                                                   ",".join(map(str, d["new"])) or "-"))
        elif kind == "wait":
            w("  %6d  ---- scalar wait (%s) ----\n" % (idx, d["kind"]))
        else:
            w("  %6d  ==== first LDS-DMA load ====\n" % idx)
    wb = res["waits_before_dma"]
    w("  lines in order of first touch: %s\n" % " ".join(map(str, res["order"])))
    w("  scalar waits before the first LDS-DMA load: %d on arguments, %d on a dereference, %d other\n"
      % (wb["kernarg"], wb["deref"], wb["other"]))
    w("  lines first requested after the first argument wait: %s\n" % (" ".join(map(str, res["late_lines"])) or "none"))
    w("  lines first requested after the first LDS-DMA load: %s\n\n" % (" ".join(map(str, res["lines_after_dma"])) or "none"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("kernels", nargs="+", help="e.g. 'step_kernel<148>' 'rollout_kernel<20>'")
    ap.add_argument("--lib", default=DEFAULT_LIB, help="libgaq.so or one of the objects it is linked from")
    ap.add_argument("--label", default=None, help="a heading printed first (e.g. which build this is)")
    a = ap.parse_args(argv)
    if find_objdump() is None:
        sys.exit("llvm-objdump not found (set LLVM_OBJDUMP)")
    if a.label:
        print("#### %s" % a.label)
    rc = 0
    for k in a.kernels:
        text = disassemble(k, a.lib)
        if text is None:
            print("== %s: not in %s" % (k, a.lib))
            rc = 1
            continue
        report(k, parse(text))
    return rc


if __name__ == "__main__":
    sys.exit(main())
