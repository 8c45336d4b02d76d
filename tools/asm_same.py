#!/usr/bin/env python3
"""Compare the kernel bodies of two `make asm` outputs symbol by symbol.

    python tools/asm_same.py --rev HEAD~1          (that commit's sources against the working tree: both are built here)

or, with two outputs already made,

    make -C sac-td3-cudagraphs-pytorch_amd/csrc asm ASM_OUT=/tmp/a.s      (at one commit)
    make -C sac-td3-cudagraphs-pytorch_amd/csrc asm ASM_OUT=/tmp/b.s      (at another)
    python tools/asm_same.py /tmp/a.s /tmp/b.s

or, to renew the record the suite holds `make asm` to (tests/test_native_rollout_host.py) in a change that means to alter a kernel,

    python tools/asm_same.py --record /tmp/b.s     (-> tests/golden/engine_kernels_sha256.json: the SHA-256 of every body)

A body is the text between `<symbol>:` and its `.Lfunc_end`, without comments and without the labels' numbering (a label number is
global to the file and moves when a kernel is added in front).  Prints the symbols only one side has and those whose bodies differ,
and whether the symbols both sides have stand in the same order; exit status 1 if a symbol present in both differs.  Needs no GPU."""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "sac-td3-cudagraphs-pytorch_amd/csrc"
RECORD = os.path.join(ROOT, "tests", "golden", "engine_kernels_sha256.json")


def bodies(path):
    """{symbol: body}, in the order the file defines them"""
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


def digests(path):
    """{symbol: SHA-256 of its body}"""
    return {name: hashlib.sha256(body.encode()).hexdigest() for name, body in bodies(path).items()}


def record(path):
    got = digests(path)
    with open(RECORD, "w") as f:
        json.dump({"what": "SHA-256 of every kernel body of `make asm` (csrc/engine.hip, gfx950) as tools/asm_same.py reads it", "kernels": got},
                  f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(got)} symbols -> {RECORD}")
    return 0


def compare(path_a, path_b):
    a, b = bodies(path_a), bodies(path_b)
    both = [n for n in a if n in b]
    diff = [n for n in both if a[n] != b[n]]
    print(f"symbols: {len(a)} / {len(b)}, in both: {len(both)}, identical: {len(both) - len(diff)}, different: {len(diff)}")
    for n in sorted(set(a) - set(b)):
        print("only in", path_a + ":", n)
    for n in sorted(set(b) - set(a)):
        print("only in", path_b + ":", n)
    for n in sorted(diff):
        print("DIFFERENT:", n)
    moved = [(x, y) for x, y in zip(both, [n for n in b if n in a]) if x != y]
    print("order of the common symbols:", "unchanged" if not moved else f"CHANGED (first at {moved[0][0]} / {moved[0][1]})")
    return 1 if diff else 0


def make_asm(csrc, out):
    subprocess.run(["make", "-C", csrc, "asm", "ASM_OUT=" + out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def compare_rev(rev):
    with tempfile.TemporaryDirectory(prefix="asm_same_") as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, CSRC, "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        old, new = os.path.join(tmp, rev.replace("/", "_") + ".s"), os.path.join(tmp, "worktree.s")
        make_asm(os.path.join(tmp, CSRC), old)
        make_asm(os.path.join(ROOT, CSRC), new)
        return compare(old, new)


def main():
    args = sys.argv[1:]
    if len(args) == 2 and args[0] == "--rev":
        return compare_rev(args[1])
    if len(args) == 2 and args[0] == "--record":
        return record(args[1])
    if len(args) == 2 and not args[0].startswith("-"):
        return compare(args[0], args[1])
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main())
