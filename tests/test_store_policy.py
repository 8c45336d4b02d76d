"""Store policy of the B < 1024 update kernels (profiles/store_policy.json) and the stores that the period
graphs leave out because only inspection reads them (TnArgs::keep_g, sactd3_engine::grads_stale)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sac-td3-cudagraphs-pytorch_amd", "csrc")
POLICY = json.load(open(os.path.join(ROOT, "profiles", "store_policy.json")))

# kernels in scope, by the mangled-name fragment of their instances
IN_SCOPE = ("4k_ntI", "10k_ctail_nnI", "10k_qtail_nnI", "12k_headbwd_nn", "4k_tnI", "14k_actor_tail_sI", "15k_actor_tail_s2I", "15k_actor_tail_s5I")
# a write to memory by the scalar unit, of any kind (stores, buffer / scratch stores, atomics, data-cache write-back or discard): a
# mnemonic that starts with "s_", optionally "buffer_" / "scratch_", then "store" / "atomic"; or the scalar data cache's two commands
_S = "s" + "_"
SCALAR_WRITE = re.compile(r"^\s*" + _S + r"(?:buffer_|scratch_)?(?:store|atomic)\w*|^\s*" + _S + "dcache" + r"_(?:wb|discard)\w*", re.M)


def make_asm(tmp_path_factory, wt):
    path = tmp_path_factory.mktemp("asm_wt%s" % ("shipped" if wt is None else wt)) / "sactd3_engine.s"
    cmd = ["make", "-C", CSRC, "asm", f"ASM_OUT={path}"] + ([] if wt is None else [f"WT={wt}"])
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    return out.stdout, path.read_text()


def kernel_bodies(txt):
    out = {}
    for name in re.findall(r"^(_Z[\w]+):\s*;?.*$", txt, re.M):
        i = txt.index("\n" + name + ":")
        out[name] = txt[i:txt.index(".Lfunc_end", i)]
    return out


def wt_stores(body):
    return [ln.strip() for ln in body.splitlines() if re.match(r"\s*(global_store|buffer_store)\w*\s", ln) and re.search(r"\bsc1\b", ln)]


def scratch_by_kernel(remarks):
    names = re.findall(r"Function Name: (\S+)", remarks)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks)]
    assert len(names) == len(scratch) and len(names) >= 15
    return dict(zip(names, scratch))


def shipped_mask():
    src = open(os.path.join(CSRC, "kernels.h")).read()
    return int(re.search(r"#ifndef SACTD3_WT\s*\n#define SACTD3_WT (\d+)", src).group(1))


def test_policy_table_is_what_the_library_is_built_with():
    """profiles/store_policy.json lists every class with its build-mask bit and the decision; the default of SACTD3_WT in kernels.h is
    the sum of the bits of the classes marked write-through, and the Makefile passes no other mask unless asked (WT=...)."""
    classes = POLICY["classes"]
    assert len({c["bit"] for c in classes}) == len(classes) >= 3
    assert shipped_mask() == sum(c["bit"] for c in classes if c["write_through"])
    assert POLICY["shipped_mask"] == shipped_mask()


@pytest.mark.parametrize("which", ["shipped", "all"])
def test_write_through_sites_compile_to_sc1_vector_stores(tmp_path_factory, which):
    """From `make asm`: every store site of a class that the policy table marks write-through is a `global_store` / `buffer_store`
    carrying `sc1` in the kernels that hold the site -- checked on the shipped build for the classes it ships with, and on the build
    with every class switched on (the A/B builds' form: all sites of the table).  A class that stays plain has no such store in the
    shipped build.  The kernels in scope hold no scalar memory write, and no instance spills to scratch."""
    classes = POLICY["classes"]
    all_mask = sum(c["bit"] for c in classes)
    mask = shipped_mask() if which == "shipped" else all_mask
    remarks, txt = make_asm(tmp_path_factory, None if which == "shipped" else all_mask)
    bodies = kernel_bodies(txt)
    scope = {n: b for n, b in bodies.items() if any(k in n for k in IN_SCOPE)}
    assert len(scope) >= 10, sorted(bodies)
    for n, b in scope.items():
        assert not SCALAR_WRITE.search(b), (n, SCALAR_WRITE.search(b).group(0))
    bad = {n: s for n, s in scratch_by_kernel(remarks).items() if s != 0}
    assert not bad, bad
    # each class names the kernel instances that hold its sites (regular expressions on the mangled name) and its store width: in
    # every one of them a write-through store of that width exists when the class is on, and none when it is off (the classes that
    # share a kernel differ in width; no kernel of a class had an `sc1` store before)
    for c in classes:
        width = re.compile(r"_store_dwordx4\s" if c["bytes_per_store"] == 16 else r"_store_dword\s")
        inst = {n: [s for s in wt_stores(b) if width.search(s)] for n, b in scope.items() if any(re.search(k, n) for k in c["kernels"])}
        assert inst, c["name"]
        for n, st in inst.items():
            assert bool(st) == bool(mask & c["bit"]), (c["name"], n, st[:3])


# ------------------------------------------------------------------------------------------------------------------ GPU

@pytest.mark.gpu
@pytest.mark.parametrize("algo,env,B", [("sac", "hopper", 256), ("td3", "halfcheetah", 256)])
def test_period_graphs_without_inspection_stores_equal_single_iterations(algo, env, B):
    """The period and cut-short period graphs do not write the gradient arenas or dz1 (keep_g == 0).  Nothing on the device reads
    them, so 4 whole periods + a cut-short one through run_iterations leave parameters, targets, log alpha, Adam state, metrics
    and the sampled indices bit-identical to the same iterations issued singly; debug_read of the gradients raises behind a period
    call and, behind a following single iteration, returns the bits of an engine that only ever stepped singly."""
    from tests.gpu_support import P, _lib, assert_same_state, engine_state, make_pair
    from tests.helpers import synth_transitions
    res, grads = [], []
    for mode in ("period", "single"):
        ref, eng, (o, a, bound) = make_pair(algo, env, B, seed=9)
        eng.rb_extend(*[t.numpy() for t in synth_transitions(3000, o, a, bound, seed=31)])
        n = 4 * 3 + 2                                        # periods 0-2, 3-5, 6-8, 9-11, then 12, 13 as a cut-short period
        if mode == "period":
            assert eng.run_iterations(0, n) == n
            for name in ("grad_critics", "c_dz1", "grad_actor", "a_dz1"):
                with pytest.raises(P.EngineError):
                    eng.debug_read(name)
        else:
            for i in range(n):
                eng.step(i % 3 == 0)
        res.append(engine_state(eng, "index"))
        eng.step(False)                                      # iteration 14: rewrites the critics' arenas in full
        grads.append((eng.debug_read("grad_critics"), eng.debug_read("c_dz1")))
        if mode == "period":
            with pytest.raises(P.EngineError):               # the actor's were not rewritten by a critic-only iteration
                eng.debug_read("grad_actor")
            eng.update_actor()
            assert eng.debug_read("grad_actor").size == eng.param_count(_lib.ACTOR) and eng.debug_read("a_dz1").size == B * 256
        eng.close()
    assert_same_state(*res, what="periods against single iterations")
    for x, y in zip(*grads):
        assert np.array_equal(x, y) and np.isfinite(x).all() and np.abs(x).max() > 0
