#!/usr/bin/env python3
"""Compare two builds of the library kernels, kernel by kernel, from their device assembly
(`hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S unit.hip -o unit.s`; several units of
one build: concatenate them).  Per kernel symbol prints `identical`, or the instruction-count
delta per mnemonic and both sides' resource figures.  Exit status 1 if a kernel is on one side
only.  No GPU and no project import.

    python tools/lib_isa_diff.py A.s B.s
"""
import collections
import re
import sys

FIGURES = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size", "accum_offset")
DROP = re.compile(r"__hip_cuid|^\s*\.(file|ident)\b")
BLOCK = re.compile(r"\.L(BB|func_end|tmp)\d+")  # local labels carry the function's number in its unit


def kernels(path):
    """{symbol: (body lines, {figure: value})} of every .amdhsa_kernel of the file."""
    lines = [ln.rstrip() for ln in open(path) if not DROP.search(ln)]
    start = {m.group(1): i for i, ln in enumerate(lines) if (m := re.match(r"^(\w+):\s*(;.*)?$", ln))}
    out = {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        name = m.group(1)
        # the code, up to its descriptor, without the comments (they name blocks by number too)
        body = [BLOCK.sub(r".L\1", x.split(";")[0].rstrip()) for x in lines[start[name] + 1:i]]
        fig = {}
        for x in lines[i:]:
            if ".end_amdhsa_kernel" in x:
                break
            f = re.match(r"\s*\.amdhsa_(\w+)\s+(\S+)", x)
            if f and f.group(1) in FIGURES:
                fig[f.group(1)] = f.group(2)
        out[name] = (body, fig)
    return out


def mnemonics(body):
    ops = (ln.split(";")[0].split() for ln in body)
    return collections.Counter(t[0] for t in ops if t and not t[0].endswith(":") and not t[0].startswith("."))


def main(a_path, b_path):
    a, b = kernels(a_path), kernels(b_path)
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"{name}: MISSING in {b_path if name in a else a_path}")
            continue
        (ba, fa), (bb, fb) = a[name], b[name]
        if ba == bb and fa == fb:
            print(f"{name}: identical")
            continue
        ma, mb = mnemonics(ba), mnemonics(bb)
        delta = {op: mb[op] - ma[op] for op in sorted(set(ma) | set(mb)) if mb[op] != ma[op]}
        print(f"{name}: differs; instructions {sum(ma.values())} -> {sum(mb.values())}, per mnemonic {delta or 'none'}")
        for f in FIGURES:
            print(f"    {f}: {fa.get(f)} -> {fb.get(f)}")
    same = sum(1 for n in a if n in b and a[n] == b[n])
    print(f"{len(a)} kernels in {a_path}, {len(b)} in {b_path}, {same} identical")
    return 0 if set(a) == set(b) else 1


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
