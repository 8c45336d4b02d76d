"""GPU: coloured exploration noise (include/sactd3_noise.h, csrc/noise_kernels.h, Engine.colored_noise, NativeRollout.collect(colored=True))
-- the generator against the float64 model with its a-priori bound (tests/colored_noise_model.py), the purity of a chunk, the coloured
collected segment against the generator, the actor model and a twin env, and the refusals.  (The white draw beside it is
tests/test_gpu_collect.py's: its kernel's text and machine code are unchanged.)"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import bounds, collect_model, colored_noise_model as M, eval_model
from tests.gpu_support import DEV, P, _lib, assert_same_state, build_engines, close_engines, engine_state, loop, same_bits, track  # noqa: F401

pytestmark = pytest.mark.gpu
envs = P.envs
SHAPES = [(64, 1), (64, 2), (128, 3), (1024, 2), (4096, 2)]      # the smallest, a half-empty pair, an odd power of two, the largest
CASES = [(L, S, beta, 0, 0) for L, S in SHAPES for beta in (0.0, 1.0, 2.0)] + [(64, 2, 1.0, c, e) for c, e in ((3, 0), (0, 2), (3, 2))]


def host(x):
    return x.cpu().numpy()


def dims_of(name):
    return envs.SPECS[envs.kind_of(name)][:3]


def one_engine(**kw):
    return build_engines("sac", dims_of("pendulum"), 64, **kw)[1][0]


@pytest.mark.parametrize("L,S,beta,chunk,epoch", CASES)
def test_generator_sits_inside_the_model_bound(L, S, beta, chunk, epoch):
    eng = one_engine()
    got = host(eng.colored_noise(beta, L, S, chunk=chunk, epoch=epoch))
    want, bound = M.chunk(eng.cfg.seed, beta, L, S, chunk, epoch)
    assert got.shape == (L, S) and got.dtype == np.float32
    worst = bounds.check("x", got, want, bound)
    print(f"L {L} S {S} beta {beta} chunk {chunk} epoch {epoch}: worst |err| / bound {worst:.3g}, worst |err| {np.abs(got - want).max():.3g}")
    assert 0.0 < worst <= 1.0
    if chunk or epoch:
        assert not same_bits(got, host(eng.colored_noise(beta, L, S)))


def test_a_chunk_is_a_pure_function_of_its_inputs():
    eng, L = one_engine(), 128
    two = host(eng.colored_noise(1.0, L, 2, chunk=1))
    eng.colored_noise(1.0, L, 5, chunk=0)
    eng.colored_noise(0.5, L, 5, chunk=1)
    five = host(eng.colored_noise(1.0, L, 5, chunk=1))
    pad = torch.full((L, 8), 7.0, device=DEV)
    wide = host(eng.colored_noise(1.0, L, 5, chunk=1, out=pad))
    assert same_bits(two, five[:, :2]) and same_bits(five, wide)
    assert same_bits(host(pad[:, 5:]), np.full((L, 3), 7.0, np.float32))
    assert not same_bits(five[:, 0], five[:, 1])


@pytest.mark.parametrize("algo", ["sac", "td3"])
@pytest.mark.parametrize("name", ["pendulum", "pointgoal"])
def test_colored_collect_explores_with_the_generated_chunks(name, algo):
    n, T, L, seed, sac = 5, 40, 64, 3, algo == "sac"
    o, a, bound = dims_of(name)
    eng = build_engines(algo, (o, a, bound), 64, count=1, seed=4, cap=512, max_envs=8)[1][0]
    rb = P.ReplayBuffer(512)
    rb._bind(eng)
    A = SimpleNamespace(engine=eng, rb=rb, timesteps_so_far=0)
    new_env = lambda: track(envs.NativeVecEnv(name, n, seed=seed, device=DEV, horizon=7))      # noqa: E731
    env, twin = new_env(), new_env()
    ro = track(loop.NativeRollout(env, A, seed, 10 ** 9, 1))
    twin.reset(seed=seed)
    ro.configure_noise(1.0, L)
    epoch = ro.noise_stats()["epoch"]
    layout = eng.rb_layout()
    lay = (layout["record_floats"], layout["next_obs_offset"], layout["next_obs_width"])
    p = eval_model.actor_params(eng.get_params(_lib.ACTOR), o, (2 if sac else 1) * a, True)
    rec, obs, used = torch.zeros((n, lay[0]), device=DEV), torch.zeros((n, o), device=DEV), []
    for call in range(2):                        # the second call straddles the chunk boundary
        slab, eps = ro.collect(T, eps=True, colored=True)
        slab, eps = host(slab), host(eps)
        used.append(eps)
        f = collect_model.fields(slab, lay, o, a)
        lo, hi = collect_model.action_intervals(p, f["s"], eps.reshape(T * n, a), mode=_lib.ROLLOUT_EXPLORE, sac=sac, ln=True,
                                                scale=np.full(a, bound, np.float32), bias=np.zeros(a, np.float32), noise_std=eng.cfg.actor_noise_std)
        assert bounds.check_interval("a", f["a"], lo, hi) <= 1.0
        rebuilt = []
        for t in range(T):
            twin.step_records(torch.as_tensor(np.ascontiguousarray(f["a"].reshape(T, n, a)[t]), device=DEV), layout, rec, obs)
            rebuilt.append(host(rec))
        assert same_bits(slab, np.concatenate(rebuilt, 0)) and same_bits(host(ro.obs), host(obs)), call
    chunks = torch.cat([eng.colored_noise(1.0, L, n * a, chunk=c, epoch=epoch) for c in (0, 1)])
    assert same_bits(np.concatenate(used), host(chunks)[:2 * T].reshape(2 * T, n, a))
    assert ro.noise_stats() == dict(length=L, pos=2 * T, chunks_generated=2, epoch=epoch)
    assert ro.collect_stats() == dict(calls=2, env_steps=2 * T, calls_that_drew=0, collect_ctr=0)
    # a fresh process: another epoch, other noise
    ro.configure_noise(1.0, L)
    assert ro.noise_stats() == dict(length=L, pos=0, chunks_generated=2, epoch=epoch + 1)
    _, again = ro.collect(T, eps=True, colored=True)
    assert not same_bits(host(again), used[0])


def test_refusals_leave_the_engine_untouched():
    name, n = "pendulum", 5
    (eng,) = build_engines("sac", dims_of(name), 64, count=1, cap=512, max_envs=8)[1]
    rb = P.ReplayBuffer(512)
    rb._bind(eng)
    ro = track(loop.NativeRollout(track(envs.NativeVecEnv(name, n, seed=1, device=DEV)), SimpleNamespace(engine=eng, rb=rb, timesteps_so_far=0), 1, 10 ** 9, 1))
    before = engine_state(eng, "ring")
    with pytest.raises(P.EngineError, match="no process"):
        ro.collect(8, colored=True)
    for beta, length in ((-0.1, 64), (2.5, 64), (float("nan"), 64), (1.0, 32), (1.0, 96), (1.0, 8192)):
        with pytest.raises(P.EngineError):
            ro.configure_noise(beta, length)
        with pytest.raises((P.EngineError, ValueError)):
            eng.colored_noise(beta, length, 2)
    for kw in (dict(sequences=0), dict(epoch=65536)):
        with pytest.raises((P.EngineError, ValueError)):
            eng.colored_noise(1.0, 64, **{"sequences": 2, **kw})
    out = torch.full((64, 4), 7.0, device=DEV)      # the library's own refusals, past the binding's checks: a short row stride, no output,
    elsewhere = np.zeros(256, np.float32)           # memory that is not the engine's device's (one device here: the host's stands for it)
    call = lambda ptr, ld: eng.lib.sactd3_colored_noise_device(eng._h, 1.0, 64, 2, 0, 0, ptr, ld, None, 0)      # noqa: E731
    assert call(out.data_ptr(), 1) == _lib.EINVAL and call(None, 4) == _lib.EINVAL and call(elsewhere.ctypes.data, 4) == _lib.EINVAL
    assert call(out.data_ptr(), 4) == 0
    assert same_bits(host(out[:, 2:]), np.full((64, 2), 7.0, np.float32))
    ro.configure_noise(1.0, 64)
    with pytest.raises(P.EngineError, match="chunk length"):
        ro.collect(65, colored=True)
    ro.configure_noise(1.0, 0)
    with pytest.raises(P.EngineError, match="no process"):
        ro.collect(8, colored=True)
    assert ro.stats()["steps"] == 0 and ro.noise_stats()["pos"] == 0 and ro.noise_stats()["chunks_generated"] == 0
    assert_same_state(before, engine_state(eng, "ring"))
