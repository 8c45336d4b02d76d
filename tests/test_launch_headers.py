"""CPU: the launch headers of the B < 1024 update kernels in the compiled gfx950 code (kernels.h, SACTD3_HDR).
`make asm` twice -- the shipped mask and HDR=0 -- and tools/asm_rounds.py over both listings."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sac-td3-cudagraphs-pytorch_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import asm_rounds  # noqa: E402

# build-mask bit -> (what the mangled names of the family's instances contain, header size in dwords)
FAMILIES = {1: ("_Z4k_tnI", 8), 2: ("_Z4k_ntI", 10)}


def shipped_mask():
    src = open(os.path.join(CSRC, "kernels.h")).read()
    return int(re.search(r"#ifndef SACTD3_HDR\s*\n#define SACTD3_HDR (\d+)", src).group(1))


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    """{"shipped" | "off": (hipcc's resource-usage remarks, assembly text), "stamps": (make's exit status, its output, library
    written)}; the two `make asm` runs and `make stamps` side by side"""
    d = tmp_path_factory.mktemp("hdr_asm")
    jobs = {}
    for key, extra in (("shipped", []), ("off", ["HDR=0"])):
        path = d / f"{key}.s"
        jobs[key] = (path, subprocess.Popen(["make", "-C", CSRC, "asm", f"ASM_OUT={path}"] + extra, stdout=subprocess.PIPE,
                                            stderr=subprocess.STDOUT, text=True))
    stamps = subprocess.Popen(["make", "-C", CSRC, "stamps", f"STAMPS_OUT={d / 'stamps.so'}"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = {}
    log = stamps.communicate()[0]
    out["stamps"] = (stamps.returncode, log, os.path.exists(d / "stamps.so"))
    for key, (path, proc) in jobs.items():
        log = proc.communicate()[0]
        assert proc.returncode == 0, log[-2000:]
        out[key] = (log, path.read_text())
    return out


def instances(txt, mask):
    res = asm_rounds.analyse(txt, [key for bit, (key, _) in FAMILIES.items() if mask & bit])
    return {n: (d, next(dw for bit, (key, dw) in FAMILIES.items() if key in n)) for n, d in res.items()}


def test_makefile_passes_the_preload_switch_to_every_target():
    """the library, the stamps build and the listing the assembly-reading tests see are built alike"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "-amdgpu-kernarg-preload-count=16" in mk
    recipes = re.findall(r"^\t\$\(HIPCC\)(?:.*\\\n)*.*", mk, re.M)
    assert len(recipes) == 3 and all("$(PRELOAD)" in r and "$(HDRFLAG)" in r for r in recipes), recipes


def test_stamps_build_compiles(listings):
    """the stamps build (tools/blocks_probe.py's per-block timelines) has per-thread branches in front of the register pins of k_tn and
    k_nt; an "s" operand the compiler believes divergent does not compile ("illegal VGPR to SGPR copy"), hence kernels.h's uni()"""
    rc, log, written = listings["stamps"]
    assert rc == 0 and written, log[-2000:]


def test_shipped_families_get_their_header_preloaded(listings):
    """every instance of a family whose bit is on in the shipped mask: the kernel descriptor asks the packet processor for exactly
    the family's header (`.amdhsa_user_sgpr_kernarg_preload_length`, >= 1), and the kernel still needs no scratch"""
    mask = shipped_mask()
    log, txt = listings["shipped"]
    inst = instances(txt, mask)
    if mask == 0:
        assert not inst
        return
    for bit, (key, _) in FAMILIES.items():
        assert not (mask & bit) or sum(key in n for n in inst) >= 8, (key, sorted(inst))
    names = re.findall(r"Function Name: (\S+)", log)
    scratch = dict(zip(names, (int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", log))))
    for name, (d, dwords) in inst.items():
        assert d["preload_length"] == dwords >= 1, (name, d)
        assert d["user_sgpr_count"] >= dwords + 2, (name, d)          # + the kernel-argument pointer
        assert scratch[name] == 0, (name, scratch[name])


def test_one_scalar_round_in_front_of_the_operand_batch(listings):
    """A tile block of k_tn and of k_nt decides its role and picks its descriptor from the header and then needs ONE round of scalar
    loads -- the descriptor by value with the common fields of its first requests -- before its operand batch goes out (the parent's
    code, by the same tool: 4 rounds in k_tn, 5 to 8 in k_nt).  `rounds` is that count on the cheapest path, which branches around
    the optional parts of the requests; test_the_round_count_sees_a_split_batch shows that it moves."""
    mask = shipped_mask()
    for name, (d, _) in instances(listings["shipped"][1], mask).items():
        assert d["rounds"] is not None and d["rounds"] <= 1 and d["first"] <= 1, (name, d)
        assert d["batch"] >= 4, (name, d)


def test_rounds_on_the_longest_way_to_the_operand_requests(listings):
    """`rounds_max`: the largest count over ALL forward paths from the block's first scalar load to any vector load in front of the
    first barrier -- the optional parts included: k_nt's ring-reading groups (Philox draw or injected index, then the record's
    address), k_tn's folded LayerNorm operands and the optimiser state it requests behind its operands.
    - k_tn and the unfused k_nt instances: 1.  k_tn's batch also brings the fields its optimiser-state requests need.
    - fused k_nt instances, which hold the ring branch: at most 2, the issue's bound for ring groups.  The control words are VECTOR
      loads through the header's pointer, issued in front of the descriptor round; the ring's record size and the bits of the ring
      and index pointers come with the descriptor, so 16 of the 24 fused instances count 1.  The 8 instances with four 16-wide
      chunks of first-layer input (C1 = 4) count 2: there the compiler fetches `ga[0].ring` a second time behind the Philox loop
      instead of keeping it in registers across it.
    test_the_longest_way_sees_a_round_in_the_ring_branch shows that this count moves."""
    mask = shipped_mask()
    inst = instances(listings["shipped"][1], mask)
    for name, (d, _) in inst.items():
        fused = "_Z4k_ntI" in name and re.match(r"_Z4k_ntILi\dELb1E", name)
        assert d["rounds_max"] is not None and d["rounds_max"] <= (2 if fused else 1), (name, d)
    fused = [d for n, (d, _) in inst.items() if re.match(r"_Z4k_ntILi\dELb1E", n)]
    assert not (mask & 2) or (len(fused) == 24 and sum(d["rounds_max"] == 1 for d in fused) >= 16 and all(d["off_path_lines"] for d in fused))


def test_the_longest_way_sees_a_round_in_the_ring_branch(listings):
    """two more dependent scalar rounds in front of a load that only the optional branches reach (the cheapest path goes around them:
    the ring group's index and row loads) leave `rounds` where it is and take `rounds_max` past the bound, for the three fused
    instances of the flagship graphs"""
    mask = shipped_mask()
    if not mask & 2:
        return
    txt = listings["shipped"][1]
    inst = instances(txt, mask)
    extra = ["\ts_load_dword s100, s[0:1], 0x0", "\ts_waitcnt lgkmcnt(0)"] * 2
    for key in ("_Z4k_ntILi1ELb1ELi2ELi1ELi1ELb0E", "_Z4k_ntILi1ELb1ELi2ELi1ELi2ELb0E", "_Z4k_ntILi1ELb1ELi4ELi1ELi1ELb0E"):
        name = next(n for n in inst if n.startswith(key))
        base = inst[name][0]
        body = next(b for n, b in asm_rounds._functions(txt) if n == name)
        lines = body.split("\n")
        for at in (base["off_path_lines"][0], base["off_path_lines"][-1]):
            got = asm_rounds.analyse(txt.replace(body, "\n".join(lines[:at] + extra + lines[at:])), [name])[name]
            assert got["rounds"] == base["rounds"] and got["rounds_max"] >= 3 > base["rounds_max"], (name, at, base, got)


def with_rounds(txt, name, where, count=2):
    """the listing with `count` more dependent scalar rounds in `name`, `where` lines behind the first load of its operand batch (0: in
    front of the batch)"""
    body = next(b for n, b in asm_rounds._functions(txt) if n == name)
    lines = body.split("\n")
    at = asm_rounds.analyse(txt, [name])[name]["batch_line"] + where
    extra = ["\ts_load_dword s100, s[0:1], 0x0", "\ts_waitcnt lgkmcnt(0)"] * count
    return txt.replace(body, "\n".join(lines[:at] + extra + lines[at:]))


def test_the_round_count_sees_a_split_batch(listings):
    """the bound above is checked against a number that moves: two more scalar rounds between the descriptor round and the operand
    batch of an instance -- what the compiled code looks like when the register pin no longer holds the batch together -- are
    counted, in front of the batch and in the middle of it, for one fused k_nt instance (control words requested first), one
    unfused one and one k_tn instance"""
    mask = shipped_mask()
    txt = listings["shipped"][1]
    inst = instances(txt, mask)
    picks = [next((n for n in inst if key in n), None) for key in ("_Z4k_ntILi1ELb1E", "_Z4k_ntILi1ELb0E", "_Z4k_tnI")]
    for name in filter(None, picks):
        base = inst[name][0]
        assert base["rounds"] <= 1
        split = asm_rounds.analyse(with_rounds(txt, name, 0), [name])[name]
        assert split["rounds"] == base["rounds"] + 2, (name, base, split)
        inside = asm_rounds.analyse(with_rounds(txt, name, 1), [name])[name]
        assert inside["rounds"] == base["rounds"] + 2, (name, base, inside)
    assert mask == 0 or any(picks)


def test_mask_zero_reads_the_decisions_from_the_struct(listings):
    """HDR=0 really switches the form: the same instances take the same parameters (so the descriptor's preload length stays -- the
    signature decides it, not the use) but read role and descriptor from the argument struct again: at least the three dependent
    rounds role -> choice -> descriptor, and more than the shipped form."""
    mask = shipped_mask()
    on, off = instances(listings["shipped"][1], mask), instances(listings["off"][1], mask)
    assert set(on) == set(off)
    for name, (d, dwords) in off.items():
        assert d["preload_length"] == dwords, (name, d)
        assert d["rounds"] >= 3 and d["rounds"] > on[name][0]["rounds"], (name, d, on[name][0])
