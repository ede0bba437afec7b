#!/usr/bin/env python3
"""Are the gfx950 kernels of a source file the same code in two checkouts?  Compares the device assembly that
`hipcc --save-temps` leaves (<name>-hip-amdgcn-amd-amdhsa-gfx950.s) and the `-Rpass-analysis=kernel-resource-usage` remarks
(hipcc's stderr, saved to a file) of two compilations with the directory's flags:

  hipcc $HIPFLAGS --save-temps -Rpass-analysis=kernel-resource-usage -c csrc/range_query.hip -o range_query.o 2> range_query.remarks.txt
  python3 tools/kernel_asm_compare.py PARENT_DIR NEW_DIR range_query point_query

Assembly: comments (everything from ';'), blank lines, .file / .ident / .loc / .cfi directives and the per-compilation
`__hip_cuid_<hash>` symbol are dropped; every other line must match.  Remarks: the `remark:` texts with the source position
dropped (a moved function keeps its numbers but not its line).  Needs no GPU.  Exit code 1 when anything differs."""
import hashlib
import re
import sys


def asm_lines(path):
    out = []
    for l in open(path):
        l = re.sub(r";.*$", "", l).rstrip()
        l = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", l)
        if l.strip() and not l.strip().startswith((".file", ".ident", ".loc ", ".cfi")):
            out.append(l)
    return out


def remark_lines(path):
    return [re.sub(r"^.*?remark: \S+ +", "", l).rstrip() for l in open(path) if "remark:" in l]


def main():
    old, new, names = sys.argv[1], sys.argv[2], sys.argv[3:]
    same = True
    for n in names:
        a, b = (asm_lines(f"{d}/{n}-hip-amdgcn-amd-amdhsa-gfx950.s") for d in (old, new))
        ra, rb = (remark_lines(f"{d}/{n}.remarks.txt") for d in (old, new))
        sha = [hashlib.sha1("\n".join(x).encode()).hexdigest()[:16] for x in (a, b)]
        print(f"{n}: assembly {len(a)} / {len(b)} lines, sha1 {sha[0]} / {sha[1]}: {'IDENTICAL' if a == b else 'DIFFERENT'}; "
              f"resource remarks {len(ra)} / {len(rb)} lines: {'IDENTICAL' if ra == rb else 'DIFFERENT'}")
        same &= a == b and ra == rb
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
