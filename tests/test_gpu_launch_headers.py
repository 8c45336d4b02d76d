"""GPU: the launch headers of k_tn and k_nt (kernels.h, SACTD3_HDR) against the argument structs they are built from.  A header
that disagreed with its struct -- a role word, a problem's first tile, M, N, the group divisor, the ring's control block -- would send
blocks to the wrong role, problem, net or rows in SOME launch shape but not in all of them: the captured period graphs, the plain
launch sequences they are captured from and the single-iteration graphs put different riders and different numbers of problems in
the same kernels, so the three must leave the same bits.  Shapes: the smallest at which a header can be wrong while the struct is
right -- B = 40 (a clamped last row block, fewer blocks than rider slots), 64 (one row block per wave split), 256 (the flagship);
SAC Hopper and TD3 HalfCheetah dimensions; a ring of 700 rows.

What this file cannot see: all three forms build their headers with the same host functions (launch_k_tn, launch_k_nt), so a header
word that is wrong in the same way in every launch -- M, say -- leaves them equal.  That the values are RIGHT rests on the oracle
comparisons of tests/test_gpu_engine.py, which run the same kernels, and on the bit-for-bit comparison of `bench.py --dump-outputs`
against the parent commit's library (profiles/kernarg_preload.json, dump_outputs)."""
import numpy as np
import pytest
import torch

from tests.gpu_support import DEV, _lib, assert_same_bits, assert_same_state, close_engines, engine_state, make_pair, stream  # noqa: F401
from tests.helpers import synth_transitions

pytestmark = pytest.mark.gpu

SHAPES = [("sac", "hopper"), ("td3", "halfcheetah")]
BATCHES = [40, 64, 256]


def engine(algo, env, B, use_graphs):
    _, eng, (o, a, bound) = make_pair(algo, env, B, use_graphs=use_graphs, seed=3)
    eng.rb_extend(*[t.numpy() for t in synth_transitions(700, o, a, bound, seed=22)])
    return eng


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("algo,env", SHAPES)
def test_graphs_launch_sequences_and_single_steps_leave_the_same_bits(algo, env, B):
    """run_iterations(1, 10) then (11, 4): the opening graph, whole periods, both cut-short forms and a single iteration -- with
    hipGraphs, as plain launch sequences, and against an engine stepped one iteration at a time (step(i % 3 == 0)).  The single
    steps run TD3's Polyak blocks and SAC's temperature step where the period graphs let them ride in other launches (T2 / T3
    arenas, the deferred temperature rider), carry fewer noise and gather riders, and launch k_tn with other problem counts."""
    states = {}
    for key, use_graphs in (("graphs", True), ("launches", False)):
        eng = engine(algo, env, B, use_graphs)
        assert eng.run_iterations(1, 10) == 11 and eng.run_iterations(11, 4) == 15
        states[key] = engine_state(eng, "index")
        eng.close()
    eng = engine(algo, env, B, True)
    for i in range(1, 15):
        eng.step(i % 3 == 0)
    states["single"] = engine_state(eng, "index")
    for key in ("launches", "single"):
        assert_same_state(states["graphs"], states[key], what=key)
    assert all(np.isfinite(v).all() for k, v in states["graphs"].items() if k.startswith("metrics."))
    assert states["graphs"]["adam_t.critics"] == 14


@pytest.mark.parametrize("B", [40, 256])
@pytest.mark.parametrize("algo,env", SHAPES)
def test_weighted_critic_update_with_unit_weights(algo, env, B):
    """the weighted critic update (its own tail kernel, the same k_nt and k_tn launches) with weights of 1.0 on caller-chosen rows
    against the plain update on the same rows: parameters, Adam state, loss and gradients, bit for bit"""
    idx = np.random.default_rng(B).integers(0, 700, B).astype(np.int64)
    idx[0], idx[-1] = 0, 699
    out = []
    for weighted in (True, False):
        eng = engine(algo, env, B, True)
        eps = torch.randn(B, eng.cfg.ac_dim, generator=torch.Generator().manual_seed(4))
        eng.set_noise(_lib.SITE_CRITIC, eps)
        if weighted:
            di, dw = torch.as_tensor(idx, device=DEV), torch.ones(B, device=DEV)
            eng.rb_sample_indices_device(di.data_ptr(), 1, dw.data_ptr(), 1, B, stream())
        else:
            eng.rb_sample_with_indices(idx)
        eng.update_qnets()
        m, v, t = eng.get_adam_state(_lib.CRITICS)
        out.append(dict(params=eng.get_params(_lib.CRITICS), m=m, v=v, t=np.float64(t), grad=eng.debug_read("grad_critics"),
                        loss=np.float32(eng.read_metrics()["loss/qf_loss"])))
        eng.close()
    assert_same_bits(out[0], out[1], what="weights of 1.0 against the plain update")
