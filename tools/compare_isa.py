#!/usr/bin/env python3
"""Compare two gfx950 assembly files (hipcc -save-temps: *-hip-amdgcn-amd-amdhsa-gfx950.s) kernel by kernel, order aside.
    python tools/compare_isa.py before.s after.s      -> kernel counts, names on one side only, kernels whose text differs; exit 1 on any
    python tools/compare_isa.py --map 'REGEX=REPLACEMENT' [--map ...] before.s after.s
A kernel's text runs from its label to its .Lfunc_end: the code and the .amdhsa_kernel descriptor; labels are numbered per function in file
order, so the numbers are masked.
--map renames kernels of `before` (re.sub on its whole text, in the order given, before anything is compared): a template whose name or
parameters changed otherwise shows as kernels on one side only.  The whole text, because a kernel's symbol also stands inside its body
and its descriptor."""
import re
import sys


def kernels(path, maps=()):
    text = open(path).read()
    for pattern, repl in maps:
        text = re.sub(pattern, repl, text)
    out = {}
    for m in re.finditer(r"^(\S+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        if ".amdhsa_kernel " + m.group(1) + "\n" in m.group(2):
            body = re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+", r".L\1", m.group(2))
            out[m.group(1)] = re.sub(r"\s*;[^\n]*", "", body)   # (comments carry block frequencies and source positions)
    return out


args, maps = sys.argv[1:], []
while args and args[0] == "--map":
    maps.append(tuple(args[1].split("=", 1)))
    args = args[2:]
a, b = kernels(args[0], maps), kernels(args[1])
only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
print(f"kernels: {len(a)} before ({sum(v.count(chr(10)) for v in a.values())} lines), {len(b)} after ({sum(v.count(chr(10)) for v in b.values())} lines); only before: {len(only_a)}; only after: {len(only_b)}; bodies that differ: {len(differ)}")
for k in only_a + only_b + differ:
    print("  ", k)
sys.exit(1 if (only_a or only_b or differ) else 0)
