#!/usr/bin/env python3
"""Do two builds hold the same device code?  Compares, kernel by kernel (keyed by symbol, so
emission order does not count), the instruction text and the .amdhsa_kernel descriptor of the
device assembly of the kernel units:

    hipcc <HIPFLAGS of the Makefile> --cuda-device-only -S csrc/UNIT.hip -o DIR/UNIT.s
    tools/asm_equal.py BEFORE_DIR AFTER_DIR

Exit status 0 when every kernel of every unit present in both directories is identical."""
import glob, os, re, sys


def kernels(path):
    text = open(path).read()
    body = {m.group(1): m.group(2) for m in re.finditer(
        r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S)}
    desc = {m.group(1): m.group(2) for m in re.finditer(
        r"^\s*\.amdhsa_kernel (\w+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S)}
    return {k: (body.get(k), desc[k]) for k in desc}


bad = 0
for before in sorted(glob.glob(os.path.join(sys.argv[1], "*.s"))):
    unit = os.path.basename(before)
    a, b = kernels(before), kernels(os.path.join(sys.argv[2], unit))
    diff = sorted(set(a) ^ set(b)) + sorted(k for k in set(a) & set(b) if a[k] != b[k])
    assert all(v[0] for v in a.values()), "a kernel without a body: the pattern is wrong"
    print(f"{unit}: {len(a)} kernels before, {len(b)} after, {len(a) - len(set(diff) & set(a))} of {len(a)} identical")
    for k in diff:
        print("   differs:", k)
    bad += len(diff)
sys.exit(1 if bad else 0)
