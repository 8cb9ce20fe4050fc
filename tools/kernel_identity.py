#!/usr/bin/env python3
"""Are the kernels of two builds of the library the same machine code?

    python tools/kernel_identity.py A.so B.so

For every function of either library's gfx950 code objects - the kernels, and the device functions that are not inlined
(fe29_sqrt, bip340_challenge ...), which every unit that calls them compiles for itself - this compares
  * the instruction list isa_count.disassemble reads (offset, opcode, branch target), cut at the symbol's size (what follows
    is padding up to the next function), and
  * for kernels the code-object notes tools/kernel_regs.sh prints (VGPRs, SGPRs, spills, scratch) plus the LDS size.
A name stands for the SET of distinct bodies it has over the code objects of a library: one body for nearly every kernel,
several where units compile their own copy of a device function.  One line per name; exit status 1 when the sets of any name
differ, which includes a name only one library has.  What a change that moves kernels between translation units is checked
with."""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_count

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
NOTES = (("vgpr", ".vgpr_count"), ("sgpr", ".sgpr_count"), ("spill", ".vgpr_spill_count"), ("scratch", ".private_segment_fixed_size"),
         ("lds", ".group_segment_fixed_size"))


def functions(lib):
    """{name: set of (notes, instructions)} over the gfx950 code objects of `lib`; notes: () for a device function."""
    tmp, objs = isa_count.code_objects(lib)
    out = {}
    try:
        for obj in objs:
            notes = {}
            text = subprocess.run([READELF, "--notes", obj], capture_output=True, text=True, check=True).stdout
            # a kernel's entry of amdhsa.kernels: from one "- .agpr_count" (its first key) to the next
            for entry in re.split(r"\n\s*- \.agpr_count:", text)[1:]:
                field = lambda key: re.search(r"\s%s:\s+(\S+)" % re.escape(key), entry).group(1)
                notes[field(".name")] = tuple((short, field(key)) for short, key in NOTES)
            syms = subprocess.run([isa_count.OBJDUMP, "-t", obj], capture_output=True, text=True, check=True).stdout
            for l in syms.splitlines():
                m = re.search(r"\sF\s+\S+\s+([0-9a-fA-F]+)\s+(?:\.\w+\s+)?(\S+)$", l)      # ... F .text <size> [.protected] <name>
                if not m or m.group(2).endswith(".kd"):
                    continue
                name, size = m.group(2), int(m.group(1), 16)
                ins = tuple(i for i in isa_count.disassemble_symbol(obj, name) if i[0] < size)
                out.setdefault(name, set()).add((notes.get(name, ()), ins))
    finally:
        subprocess.run(["rm", "-rf", tmp])
    return out


def describe(bodies):
    return " | ".join("%d instructions %s" % (len(ins), " ".join("%s=%s" % kv for kv in notes)) for notes, ins in sorted(bodies))


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            verdict = "ONLY IN " + (sys.argv[1] if name in a else sys.argv[2]) + ": " + describe(a.get(name) or b[name])
        elif a[name] == b[name]:
            verdict = "identical: " + describe(a[name])
        else:
            verdict = "DIFFERENT: " + describe(a[name]) + "  ->  " + describe(b[name])
        bad += not verdict.startswith("identical")
        print("%-110s %s" % (name, verdict))
    print("%d functions, %d not identical" % (len(set(a) | set(b)), bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
