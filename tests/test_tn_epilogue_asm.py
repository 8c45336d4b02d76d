"""CPU: the compiled gfx950 code of the weight-gradient kernels commits the optimiser state in 16-byte stores.

k_tn / k_tn_bc keep their tile transposed in the accumulators, so the committing wave writes G, m, v, P and the Polyak targets as
one global_store_dwordx4 per array (csrc/tn_body.inc, adam_commit4).  Before that, every instance unrolled four rows of 4-byte
stores: 37 global_store_dword in the gradient-keeping instances of k_tn (4 rows x 7 arrays, 7 of the bias / folded vectors, 2 of
the riding blocks), 32 in the others (no G), and 2 more each in k_tn_bc (the loss and its tick).  The counts are those of the
parent commit's `make asm`; what is left now is the bias path, the riding blocks and the rolled per-element form for layouts
that are not float4 aligned.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 4-byte global stores per instance before the 16-byte epilogue: (kernel, KEEP_G) -> count
STORES_4B_BEFORE = {("k_tn", True): 37, ("k_tn", False): 32, ("k_tn_bc", True): 39, ("k_tn_bc", False): 34}


@pytest.fixture(scope="module")
def tn_functions(tmp_path_factory):
    """`make asm` into a private temporary file: {(kernel, KT, FOLD, KEEP_G): assembly text of the instance}"""
    csrc = os.path.join(ROOT, "sac-td3-cudagraphs-pytorch_amd", "csrc")
    path = tmp_path_factory.mktemp("asm") / "sactd3_engine.s"
    out = subprocess.run(["make", "-C", csrc, "asm", f"ASM_OUT={path}"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    txt = path.read_text()
    fns = {}
    for name in re.findall(r"^(_Z[\w]+):\s*;?.*$", txt, re.M):
        m = re.match(r"_Z\d(k_tn|k_tn_bc)ILi(\d)ELb([01])ELb([01])EE", name)
        if m:
            i = txt.index("\n" + name + ":")
            fns[(m.group(1), int(m.group(2)), m.group(3) == "1", m.group(4) == "1")] = txt[i:txt.index(".Lfunc_end", i)]
    return fns


def test_every_instance_is_there(tn_functions):
    assert sorted(tn_functions) == sorted((k, kt, f, g) for k in ("k_tn", "k_tn_bc") for kt in (1, 2) for f in (False, True) for g in (False, True))


def test_tn_instances_commit_in_16_byte_stores(tn_functions):
    for (kernel, kt, fold, keep_g), body in sorted(tn_functions.items()):
        wide = len(re.findall(r"^\s*global_store_dwordx4\s", body, re.M))
        narrow = len(re.findall(r"^\s*global_store_dword\s", body, re.M))
        # Mo, Vo, P, T, T2, T3 (and G) of the tile, on top of the riding Polyak blocks' one
        assert wide >= (7 if keep_g else 6) + 1, (kernel, kt, fold, keep_g, wide)
        assert narrow < STORES_4B_BEFORE[(kernel, keep_g)], (kernel, kt, fold, keep_g, narrow)


def test_tn_state_fetch_is_one_batch_of_16_byte_loads(tn_functions):
    """the tile's P, m, v, T requests stand behind the operand batch without a wait in between: 8 (KT = 1) or 12 (KT = 2) operand
    float4 and the state's 4 in one run of loads that no s_waitcnt vmcnt interrupts (a joined 4-byte form once put vmcnt(0) there)"""
    for (kernel, kt, fold, keep_g), body in sorted(tn_functions.items()):
        if fold:              # (the folded instance requests its LayerNorm operands in between, under a branch of its own)
            continue
        ev = []
        for line in body.splitlines():
            ins = line.strip()
            if ins.startswith("global_load_dwordx4"):
                ev.append("L")
            elif ins.startswith("s_waitcnt") and "vmcnt" in ins:
                ev.append("W")
        assert "L" * (4 * (kt + 1) + 4) in "".join(ev), (kernel, kt, keep_g, "".join(ev))
