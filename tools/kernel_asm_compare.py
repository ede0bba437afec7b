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

compares kernel by kernel instead (a kernel = its .text section, kernel descriptor and resource remarks; the function
number inside local labels is dropped), for files that gained or lost kernels: a kernel on one side only is listed and not
counted as a difference; a differing kernel of equal length has its (first eight) differing lines printed."""
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


def kernels(path, remarks):
    """{kernel: (assembly lines, remark lines)}"""
    out, cur = {}, None
    for l in asm_lines(path):
        m = re.match(r"\s*\.section\s+\.text\.(\w+)", l)
        if m:
            cur = out.setdefault(m.group(1), ([], []))
        elif re.match(r"\s*\.section\s+\.AMDGPU\.gpr_maximums", l):
            cur = None
        if cur is not None:
            cur[0].append(re.sub(r"\.L(BB|func_begin|func_end|tmp)\d+", r".L\1", l))
    cur = None
    for l in remark_lines(remarks):
        m = re.match(r"Function Name: (\w+)", l)
        if m:
            cur = out.get(m.group(1))
        if cur is not None:
            cur[1].append(l)
    return out


def compare_kernels(old, new, names):
    same = True
    for n in names:
        ka, kb = (kernels(f"{d}/{n}-hip-amdgcn-amd-amdhsa-gfx950.s", f"{d}/{n}.remarks.txt") for d in (old, new))
        for k in sorted(set(ka) | set(kb)):
            if k not in ka or k not in kb:
                print(f"{n}: {k}: only in {'the first' if k in ka else 'the second'}")
                continue
            (a, ra), (b, rb) = ka[k], kb[k]
            print(f"{n}: {k}: assembly {len(a)} / {len(b)} lines: {'IDENTICAL' if a == b else 'DIFFERENT'}; "
                  f"resource remarks: {'IDENTICAL' if ra == rb else 'DIFFERENT'}")
            if a != b and len(a) == len(b):
                pairs = [(x, y) for x, y in zip(a, b) if x != y]
                print(f"    {len(pairs)} lines differ in place")
                for x, y in pairs[:8]:
                    print(f"    < {x.strip()}\n    > {y.strip()}")
            same &= a == b and ra == rb
    sys.exit(0 if same else 1)


def main():
    if sys.argv[1] == "--kernels":
        return compare_kernels(sys.argv[2], sys.argv[3], sys.argv[4:])
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
