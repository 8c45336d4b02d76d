"""The 16-byte optimiser epilogue of k_tn at ragged tiles, every element against float64.

A weight-gradient block of k_tn keeps its 16 x 16 tile transposed in the accumulators (X is the MFMA's A operand), so a lane of
the committing wave owns 4 consecutive columns of ONE weight row and fetches / commits P, m, v, T (and G) as one float4 per array.
What can go wrong there is the lane -> element map at the tile edges: the row predicate (n < N) now holds per lane instead of per
register, the zero-gradient rule for the pad columns (k >= K) per component instead of per lane.  Two shapes outside
tests/test_gpu_large_batch.py's CASES (gpu_stage_checks.LARGE_BATCH_CASES) put every such edge into one iteration:
  * SAC Hopper, B = 33: a last row block of one row; the actor head N = 6 < 16 (10 of the tile's 16 row lanes commit nothing) and
    the critics' layer 1 with K = 14 in rows of 16 floats (the last float4 of a row is half gradient, half pad);
  * TD3 `td3_7`, B = 49, no LayerNorm: a = 7 (head N = 7, odd; actor K = 13 in rows of 16: a float4 with one gradient and three pad
    columns), and the plain (unfolded) layer-1 problem.
Both run update_qnets / update_actor / update_targ_nets stage by stage (run_one_iteration, stages=True: the gradient-keeping
instances) and one fused critic iteration (the Polyak targets stepped in the same epilogue).  Every element of p, m, v and of the
targets must fall within the a-priori bounds of tests/bounds.py; no tolerance here is taken from an observed error.
"""
import pytest

from tests.gpu_stage_checks import LARGE_BATCH_CASES as CASES, run_fused_critic_iteration, run_one_iteration
from tests.gpu_support import close_engines  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = [("sac", "hopper", 33, True), ("td3", "td3_7", 49, False)]


@pytest.mark.parametrize("algo,env,B,ln", SHAPES, ids=[f"{a}-{e}-{b}-{'ln' if ln else 'noln'}" for a, e, b, ln in SHAPES])
def test_tn_epilogue_ragged_tiles_against_float64(algo, env, B, ln):
    assert (algo, env, B, ln) not in CASES
    rec = f"tn_epilogue[{algo}-{env}-{B}-{ln}]"
    run_one_iteration(algo, env, B, ln, rec, stages=True)
    run_fused_critic_iteration(algo, env, B, ln, rec, stages=True)
