#!/usr/bin/env python3
"""Are the gfx950 kernels of a source file the same code in two checkouts?  Compares the device assembly that
`hipcc --save-temps` leaves (<name>-hip-amdgcn-amd-amdhsa-gfx950.s) and the `-Rpass-analysis=kernel-resource-usage` remarks
(hipcc's stderr, saved to a file) of two compilations with the directory's flags:

  hipcc $HIPFLAGS --save-temps -Rpass-analysis=kernel-resource-usage -c csrc/range_query.hip -o range_query.o 2> range_query.remarks.txt
  python3 tools/kernel_asm_compare.py PARENT_DIR NEW_DIR range_query point_query

Assembly: comments (everything from ';'), blank lines, .file / .ident / .loc / .cfi directives and the per-compilation
`__hip_cuid_<hash>` symbol are dropped; every other line must match.  Remarks: the `remark:` texts with the source position
dropped (a moved function keeps its numbers but not its line).  Needs no GPU.  Exit code 1 when anything differs.

  python3 tools/kernel_asm_compare.py --kernels PARENT_DIR NEW_DIR range_query

compares kernel by kernel instead (a kernel = its code from `.type <symbol>,@function` to its resource block: the .text
section, the .amdhsa_ kernel descriptor and the .set lines, plus its resource remarks; the function number inside local
labels is dropped), for files that gained or lost kernels: a kernel on one side only is listed and not counted as a
difference; a differing kernel of equal length has its (first eight) differing lines printed, and whether the two sides are
permutations of each other.

  python3 tools/kernel_asm_compare.py --pairs PAIRS.txt PARENT_DIR NEW_DIR

compares the kernels PAIRS.txt lists, for kernels that were renamed or moved to another file.  A line of it is
`file:symbol file:symbol` (first tree, second tree; `#` starts a comment); `symbol` is any part of the mangled name that only
one kernel of that file contains.  Both symbols are replaced by KERNEL before the comparison.

Ignored in both kernel modes: the visibility directives (.globl / .protected / .weak / .hidden), whether the kernel has a
.text.<symbol> section of its own (a template) or sits in .text, and the alignment padding behind the last kernel of a file
(it comes after the kernel's resource block)."""
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


def kernels(d, n):
    """{kernel: (assembly lines, remark lines)} of source file n compiled in directory d, the symbol written as KERNEL"""
    out, cur, name = {}, None, None
    for l in asm_lines(f"{d}/{n}-hip-amdgcn-amd-amdhsa-gfx950.s"):
        m = re.match(r"\s*\.type\s+(\w+),@function", l)
        if m:
            name = m.group(1)
            cur = out.setdefault(name, ([], []))
        elif re.match(r"\s*\.section\s+\.AMDGPU\.", l):
            cur = None
        if cur is not None and not re.match(r"\s*\.(globl|protected|weak|hidden)\s", l):
            l = re.sub(r"\.section\s+\.text\.\S+", ".text", re.sub(r"\.L(BB|func_begin|func_end|tmp)\d+", r".L\1", l))
            cur[0].append(l.replace(name, "KERNEL"))
    cur = None
    for l in remark_lines(f"{d}/{n}.remarks.txt"):
        m = re.match(r"Function Name: (\w+)", l)
        if m:
            name = m.group(1)
            cur = out.get(name)
        if cur is not None:
            cur[1].append(l.replace(name, "KERNEL"))
    return out


def compare_kernel(title, ka, kb):
    (a, ra), (b, rb) = ka, kb
    print(f"{title}: assembly {len(a)} / {len(b)} lines: {'IDENTICAL' if a == b else 'DIFFERENT'}; "
          f"resource remarks: {'IDENTICAL' if ra == rb else 'DIFFERENT'}")
    if a != b and len(a) == len(b):
        pairs = [(x, y) for x, y in zip(a, b) if x != y]
        print(f"    {len(pairs)} lines differ in place; the two sides are "
              f"{'permutations of each other' if sorted(a) == sorted(b) else 'NOT permutations of each other'}")
        for x, y in pairs[:8]:
            print(f"    < {x.strip()}\n    > {y.strip()}")
    return a == b and ra == rb


def compare_kernels(old, new, names):
    same = True
    for n in names:
        ka, kb = kernels(old, n), kernels(new, n)
        for k in sorted(set(ka) | set(kb)):
            if k not in ka or k not in kb:
                print(f"{n}: {k}: only in {'the first' if k in ka else 'the second'}")
                continue
            same &= compare_kernel(f"{n}: {k}", ka[k], kb[k])
    sys.exit(0 if same else 1)


def compare_pairs(listing, old, new):
    same = True
    for line in open(listing):
        sides = re.sub(r"#.*$", "", line).split()
        if not sides:
            continue
        found = []
        for d, spec in zip((old, new), sides):
            n, part = spec.split(":")
            hits = [(k, v) for k, v in kernels(d, n).items() if part in k]
            if len(hits) != 1:
                sys.exit(f"{spec}: {len(hits)} kernels of {d}/{n} contain it")
            found.append(hits[0])
        same &= compare_kernel(f"{sides[0]} = {sides[1]}", found[0][1], found[1][1])
    sys.exit(0 if same else 1)


def main():
    if sys.argv[1] == "--kernels":
        return compare_kernels(sys.argv[2], sys.argv[3], sys.argv[4:])
    if sys.argv[1] == "--pairs":
        return compare_pairs(sys.argv[2], sys.argv[3], sys.argv[4])
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
