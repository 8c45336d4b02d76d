#!/usr/bin/env python3
"""Compare the kernel bodies of two `make asm` outputs symbol by symbol.

    make -C sac-td3-cudagraphs-pytorch_amd/csrc asm ASM_OUT=/tmp/a.s      (at one commit)
    make -C sac-td3-cudagraphs-pytorch_amd/csrc asm ASM_OUT=/tmp/b.s      (at another)
    python tools/asm_same.py /tmp/a.s /tmp/b.s

A body is the text between `<symbol>:` and its `.Lfunc_end`, without comments and without the labels' numbering (a label number is
global to the file and moves when a kernel is added in front).  Prints the symbols only one side has and those whose bodies differ;
exit status 1 if a symbol present in both differs.  Needs no GPU."""
import re
import sys


def bodies(path):
    txt = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):", txt, re.M):
        name = m.group(1)
        end = txt.index(".Lfunc_end", m.end())
        lines = []
        for line in txt[m.end():end].splitlines():
            line = line.split(";")[0].rstrip()
            if not line.strip() or line.lstrip().startswith((".loc", ".file", ".cfi")):
                continue
            lines.append(line)
        body = "\n".join(lines)
        # labels: .LBB<function number>_<block> -> .LBB_<block>
        body = re.sub(r"\.LBB\d+_", ".LBB_", body)
        body = re.sub(r"\.Ltmp\d+", ".Ltmp", body)
        out[name] = body
    return out


def main():
    a, b = bodies(sys.argv[1]), bodies(sys.argv[2])
    both = sorted(set(a) & set(b))
    diff = [n for n in both if a[n] != b[n]]
    print(f"symbols: {len(a)} / {len(b)}, in both: {len(both)}, identical: {len(both) - len(diff)}, different: {len(diff)}")
    for n in sorted(set(a) - set(b)):
        print("only in", sys.argv[1] + ":", n)
    for n in sorted(set(b) - set(a)):
        print("only in", sys.argv[2] + ":", n)
    for n in diff:
        print("DIFFERENT:", n)
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
