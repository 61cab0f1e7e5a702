#!/usr/bin/env python
"""Kernel-by-kernel companion of tools/isa_cmp.sh, for a change that ADDS kernels to a unit and must leave the existing ones alone.

isa_cmp.sh compares whole units, so a unit that gains an instantiation reads DIFFERENT.  This reads the stripped assembly it leaves in
$ISA_CMP_OUT (<unit>.<variant>.{a,b}.s), cuts both sides into kernels (the text from `<symbol>:` to its `.Lfunc_end`, and the kernel's
`.amdhsa_kernel` descriptor block: registers, LDS, scratch) and compares the kernels both sides have.  Basic-block labels are
renumbered per kernel (.LBB<function>_<block> counts functions from the start of the file).

    tools/isa_cmp.sh <checkout A> <checkout B> frames model; python tools/isa_cmp_kernels.py frames model [--pair A_SYMBOL=B_SYMBOL ...]

--pair: a kernel that changed its (mangled) name only — one that became the `false` instantiation of a template — is compared under
its old name.  Prints one line per unit and variant: common kernels identical / the names that differ, and the kernels only one side has.  Exit 1 if a
common kernel differs or side A has a kernel side B lacks.
"""
import os
import re
import sys


def kernels(path):
    out, descr, name, body = {}, {}, None, []
    in_descr = None
    for line in open(path):
        line = line.rstrip()
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            in_descr, descr[m.group(1)] = m.group(1), []
            continue
        if in_descr is not None:
            if ".end_amdhsa_kernel" in line:
                in_descr = None
            else:
                descr[in_descr].append(line.strip())
            continue
        m = re.match(r"^([A-Za-z_][\w$.]*):$", line)
        if m and not m.group(1).startswith(".L"):
            name, body = m.group(1), []
            continue
        if name is not None:
            if re.match(r"^\.Lfunc_end\d+:", line):
                out[name] = body
                name = None
            elif not re.match(r"^\s*\.(text|section)\b", line):  # (a template instantiation sits in a COMDAT section of its own)
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", line.strip()))
    return {k: (v, descr.get(k)) for k, v in out.items() if k in descr}


def main():
    out = os.environ.get("ISA_CMP_OUT", "/tmp/isa_cmp")
    bad = 0
    args, pairs = sys.argv[1:], {}
    while "--pair" in args:
        i = args.index("--pair")
        old, new = args[i + 1].split("=")
        pairs[new] = old
        del args[i:i + 2]
    for unit in args:
        for variant in ("fp16", "bf16"):
            a, b = (kernels(os.path.join(out, f"{unit}.{variant}.{side}.s")) for side in "ab")
            for new, old in pairs.items():  # (the symbol also appears in the kernel's own text: its end label, the descriptor's references)
                if new in b:
                    code, descr = b.pop(new)
                    b[old] = ([x.replace(new, old) for x in code], [x.replace(new, old) for x in descr])
            common = sorted(set(a) & set(b))
            differ = [k for k in common if a[k] != b[k]]
            gone, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
            print(f"{unit} {variant}: {len(common) - len(differ)} of {len(common)} common kernels identical (code and descriptor); "
                  f"{len(new)} new, {len(gone)} gone")
            for k in differ:
                print(f"  DIFFERENT {k}")
            for k in gone:
                print(f"  GONE {k}")
            for k in new:
                print(f"  new {k}")
            bad |= bool(differ or gone)
    sys.exit(bad)


if __name__ == "__main__":
    main()
