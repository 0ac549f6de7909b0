#!/usr/bin/env python3
"""Per-mnemonic instruction counts of line ranges of an assembly listing (hipcc -S), for the static records under profiles/.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -S --cuda-device-only csrc/attention.hip -o attention.s
    python tools/isa_mnemonics.py attention.s 2918:3252 [FIRST:LAST ...]

A range is FIRST:LAST in 1-based line numbers, both included: the listing's block labels move with the compiler version, so the ranges
are read off the listing by hand (profiles/attention_fastpath_isa.txt says which blocks they were).  Labels, comments, directives and the
;;#ASMSTART / ;;#ASMEND markers are not instructions; the instructions of an inline-asm statement are counted like any other."""
import collections
import sys


def mnemonics(lines):
    out = collections.Counter()
    for line in lines:
        s = line.split(";")[0].strip()
        if not s or s.endswith(":") or s.startswith("."):
            continue
        out[s.split()[0]] += 1
    return out


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    with open(argv[1]) as f:
        lines = f.read().splitlines()
    for rng in argv[2:]:
        a, b = (int(x) for x in rng.split(":"))
        c = mnemonics(lines[a - 1:b])
        print(f"lines {a}..{b}: {sum(c.values())} instructions")
        for name, n in sorted(c.items(), key=lambda kv: (-kv[1], kv[0])):
            print(f"    {n:4d}  {name}")


if __name__ == "__main__":
    main(sys.argv)
