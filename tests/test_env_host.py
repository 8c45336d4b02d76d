"""CPU: the host side of the GPU-resident environments -- include/sactd3_env.h and its binding cover each other, a NULL handle is
refused, `envs.HostVecEnv` keeps the gymnasium protocol and its episode books, its resets are the Philox model's bit for bit, and the
launcher plans the new env ids."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import sac_td3_cudagraphs_pytorch_amd as P
from sac_td3_cudagraphs_pytorch_amd import _lib, envs, launcher, loop
from tests import env_model as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["pendulum", "cartpole"]


def test_header_and_binding_cover_each_other():
    src = open(os.path.join(ROOT, "include", "sactd3_env.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(sactd3_env_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted(_lib.ENV_SYMBOLS) and len(declared) == 10
    assert not set(_lib.ENV_SYMBOLS) & set(_lib.SYMBOLS)                    # include/sactd3.h and its list stay what they were
    if not os.path.exists(P.library_path()):
        P.build_library()
    raw = C.CDLL(P.library_path())
    for name in declared:
        assert hasattr(raw, name), f"{name} is declared in include/sactd3_env.h but not exported"
    lib = P.load_library()
    assert all(getattr(lib, name).argtypes is not None for name in declared)
    # the struct mirrors have the C layout (plain 4- and 8-byte fields, natural alignment)
    assert C.sizeof(_lib.CEnvConfig) == 24 and _lib.CEnvConfig.seed.offset == 16
    assert C.sizeof(_lib.CEnvInfo) == 24 and C.sizeof(_lib.CEnvOut) == 96 and C.sizeof(_lib.CEnvState) == 40 and C.sizeof(_lib.CEnvStats) == 72
    assert (_lib.ENV_PENDULUM, _lib.ENV_CARTPOLE, _lib.ENV_STATE_DIM) == (0, 1, 4)
    for word, value in (("SACTD3_ENV_PENDULUM", 0), ("SACTD3_ENV_CARTPOLE", 1)):
        assert re.search(rf"{word}\s*=\s*{value}\b", src)


def test_a_null_handle_is_refused_by_every_call():
    lib = P.load_library()
    assert lib.sactd3_env_spec(None, C.byref(_lib.CEnvInfo())) == _lib.EINVAL
    assert lib.sactd3_env_reset(None, 0, None, 0, None) == _lib.EINVAL
    assert lib.sactd3_env_step(None, None, 0, None, None) == _lib.EINVAL
    assert lib.sactd3_env_sample_actions(None, None, 0, None) == _lib.EINVAL
    assert lib.sactd3_env_episode_stats(None, C.byref(_lib.CEnvStats()), None) == _lib.EINVAL
    assert lib.sactd3_env_get_state(None, C.byref(_lib.CEnvState()), None) == _lib.EINVAL
    assert lib.sactd3_env_set_state(None, C.byref(_lib.CEnvState()), None) == _lib.EINVAL
    lib.sactd3_env_destroy(None)                                             # a no-op
    h = C.c_void_p()
    assert lib.sactd3_env_create(None, C.byref(h)) == _lib.EINVAL and not h.value
    assert b"NULL" in lib.sactd3_env_last_error(None)
    for bad in (_lib.CEnvConfig(7, 4, 0, 0, 0), _lib.CEnvConfig(0, 0, 0, 0, 0), _lib.CEnvConfig(0, 4, -1, 0, 0)):
        assert lib.sactd3_env_create(C.byref(bad), C.byref(h)) == _lib.EINVAL and not h.value
    assert b"horizon" in lib.sactd3_env_last_error(None)


def test_no_cpu_fallback_for_the_device_env():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(P.EngineError, match="no HIP device|not gfx950"):
        envs.NativeVecEnv("pendulum", 4)
    with pytest.raises(ValueError):
        envs.NativeVecEnv("pendulum", 4, device="cpu")


def test_the_product_restates_what_the_model_states():
    """envs.py carries its own Philox and its own physics (the product imports neither tests/ nor oracle/): the same bits as the
    model's draws, and a step inside the model's bound"""
    for name in KINDS:
        kind = envs.kind_of(name)
        idx, ep = np.arange(300), np.arange(300) % 7
        assert np.array_equal(envs.first_states(kind, 2 ** 40 + 5, idx, ep), em.first_states(kind, 2 ** 40 + 5, idx, ep))
        assert np.array_equal(envs.random_actions(kind, 9, idx, ep), em.random_actions(kind, 9, idx, ep))
        assert envs.SPECS[kind][:3] == (em.OB_DIM[kind], 1, em.BOUND[kind]) and envs.STREAM_ENV == em.STREAM_ENV
    src = open(os.path.join(ROOT, "sac-td3-cudagraphs-pytorch_amd", "envs.py")).read()
    assert not re.search(r"^\s*(from|import)\s+(tests|oracle)\b", src, re.M)


@pytest.mark.parametrize("name", KINDS)
def test_host_env_steps_inside_the_models_bound(name):
    kind, n, seed = envs.kind_of(name), 9, 4
    env = envs.HostVecEnv(name, n, seed=seed)
    obs, info = env.reset(seed=seed)
    assert info == {} and obs.shape == (n, em.OB_DIM[kind]) and obs.dtype == np.float32
    assert np.array_equal(env.state()["phys"], em.first_states(kind, seed, np.arange(n), np.zeros(n)))      # bit for bit
    worst, ends = 0.0, 0
    for _ in range(230):
        before = env.state()
        act = env.action_space.sample()
        assert np.array_equal(act, em.random_actions(kind, seed, np.arange(n), before["draws"]))
        if not em.conditioned(kind, before, act).all():
            continue                                                          # (rolled states: none is expected this close to a threshold)
        nobs, rew, term, trunc, infos = env.step(act)
        ended = term | trunc
        final = nobs.copy()
        for k in np.flatnonzero(ended):
            final[k] = infos["final_observation"][k]
        got = {"obs": nobs, "final_obs": final, "reward": rew, "terminated": term, "truncated": trunc, "ended": ended}
        worst = max(worst, em.check_step(kind, seed, env.horizon, before, act, got, env.state()))
        ends += int(ended.sum())
    assert ends >= n and 0.0 < worst <= 1.0


@pytest.mark.parametrize("name", KINDS)
def test_host_env_protocol_and_episode_books(name):
    n = 3
    env = envs.HostVecEnv(name, n, seed=1, horizon=25)
    env.reset(seed=1)
    lengths, returns, run = [], [], np.zeros(n, np.float32)
    first = {}
    for t in range(80):
        obs, rew, term, trunc, infos = env.step(env.action_space.sample())
        run = (run + rew).astype(np.float32)
        assert rew.dtype == np.float32 and term.dtype == bool and trunc.dtype == bool and not (term & trunc).any()
        ended = term | trunc
        assert ("final_info" in infos) == ("final_observation" in infos) == bool(ended.any())
        for k in range(n):
            if ended[k]:
                ep = infos["final_info"][k]["episode"]
                assert infos["final_observation"].dtype == object and infos["final_observation"][k].shape == obs[k].shape
                assert np.float32(ep["r"][0]) == run[k] and 1 <= int(ep["l"][0]) <= 25 and (int(ep["l"][0]) == 25) == bool(trunc[k])
                lengths.append(int(ep["l"][0]))
                first.setdefault(k, (np.float32(ep["r"][0]), int(ep["l"][0])))
                returns.append(float(ep["r"][0]))
                run[k] = 0.0
            elif ended.any():
                assert infos["final_info"][k] is None and infos["final_observation"][k] is None
    st = env.episode_stats()
    assert st["episodes"] == len(lengths) >= 3 * n and st["length_sum"] == sum(lengths) and st["return_sum"] == pytest.approx(sum(returns))
    assert st["bad_actions"] == 0
    assert [(st["first_return"][k], int(st["first_length"][k])) for k in range(n)] == [first[k] for k in range(n)]      # one episode per env: its first
    if name == "pendulum":
        assert set(lengths) == {25}                                           # never terminates
    # NaN / infinite actions: replaced by 0, counted, and the state stays finite
    env.step(np.array([[np.nan], [np.inf], [0.5]], np.float32))
    assert env.episode_stats()["bad_actions"] == 2 and np.isfinite(env.state()["phys"]).all()
    # the largest finite float is an action like any other beyond the bounds: clamped, not counted
    u, bad = envs.clean_actions(env.kind, np.array([[3.4028235e38], [-3.3e38], [np.inf]], np.float32), 3)
    assert list(bad) == [False, False, True] and list(u) == [env.bound, -env.bound, 0.0]
    # state round trip
    s = env.state()
    env.step(env.action_space.sample())
    env.set_state(s)
    assert all(np.array_equal(env.state()[k], s[k]) for k in s)
    with pytest.raises(ValueError):
        env.set_state({"phys": np.full((n, 4), np.nan, np.float32)})


def test_host_env_serves_the_loops_evaluation_as_it_stands():
    """loop.episode / loop.evaluate on a one-env HostVecEnv: lengths and returns from final_info, a greedy stub policy"""
    agent = SimpleNamespace(predict=lambda td, explore: np.zeros((1, 1), np.float32))
    got = loop.evaluate(SimpleNamespace(seed=3, num_episodes=3), envs.HostVecEnv("pendulum", 1, seed=3, horizon=20), agent)
    assert got["length"] == 20.0 and got["return"] < 0.0
    got = loop.evaluate(SimpleNamespace(seed=3, num_episodes=3), envs.HostVecEnv("cartpole", 1, seed=3), agent)
    assert 5.0 <= got["length"] == got["return"] < 200.0                      # the unforced pole falls
    # greedy_returns on the host twin: the same figure from the env's own books
    env = envs.HostVecEnv("pendulum", 4, seed=3, horizon=20)
    agent = SimpleNamespace(predict=lambda td, explore: np.zeros((len(td["observations"]), 1), np.float32))
    got = envs.greedy_returns(env, agent, 4)
    assert got["episodes"] == 4 and got["length"] == 20.0 and got["return"] == float(got["returns"].astype(np.float64).mean())
    # the cart-pole falls early and goes on with further episodes: one episode per env counts, its first
    env = envs.HostVecEnv("cartpole", 4, seed=3)
    got = envs.greedy_returns(env, agent, 4)
    st = env.episode_stats()
    assert st["episodes"] > 4 and got["episodes"] == 4 and np.array_equal(got["returns"], st["first_return"])
    assert got["length"] == got["return"] == float(st["first_length"].mean()) and not np.array_equal(st["first_return"], st["last_return"])
    with pytest.raises(ValueError):
        envs.greedy_returns(env, agent, 5)


def test_launcher_plans_the_native_ids():
    assert launcher.ENV_BUNDLES["native"] == ["Pendulum-native", "CartPole-native"]
    assert launcher.ENV_DIMS["Pendulum-native"] == (3, 1, 2.0) and launcher.ENV_DIMS["CartPole-native"] == (4, 1, 1.0)
    for env_id, kind in launcher.NATIVE_ENVS.items():
        o, a, bound = launcher.ENV_DIMS[env_id]
        assert envs.SPECS[envs.kind_of(kind)][:3] == (o, a, bound)
    assert launcher.sweep_jobs("native", 2) == [("Pendulum-native", 0), ("Pendulum-native", 1), ("CartPole-native", 0), ("CartPole-native", 1)]
    assert launcher.env_plan("Pendulum-native", False) == dict(train="HostVecEnv", eval="HostVecEnv")
    assert launcher.env_plan("CartPole-native", True) == dict(train="NativeVecEnv", eval="NativeVecEnv")      # no host env step in the job
    assert launcher.env_plan("Hopper-v4", False) == dict(train="SyntheticVecEnv", eval="SyntheticVecEnv")    # as before
    assert launcher.env_plan("Hopper-v4", True) == dict(train="SyntheticDeviceVecEnv", eval="SyntheticVecEnv")
    assert launcher.env_plan("Pendulum-native", True, has_factory=True) == dict(train="SyntheticDeviceVecEnv", eval="factory")
    # the older bundles are what they were
    assert launcher.ENV_BUNDLES["debug"] == ["Hopper-v4"] and launcher.ENV_DIMS["Hopper-v4"] == (11, 3, 1.0)


def test_launcher_dry_run_of_the_native_bundle():
    import json
    import subprocess
    import sys
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "sac_td3_cudagraphs_pytorch_amd.launcher", "--env_bundle", "native", "--device_env", "--num_seeds", "1",
                          "--dry-run"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    jobs = [json.loads(ln[4:]) for ln in out.stdout.splitlines() if ln.startswith("JOB ")]
    assert [j["env_id"] for j in jobs] == ["Pendulum-native", "CartPole-native"] and all(j["dry_run"] for j in jobs)
    sweep = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("SWEEP ")][-1][6:])
    assert sweep["expected_jobs"] == sweep["jobs"] == 2


def test_the_stamps_build_loads_through_the_binding(tmp_path):
    """`make stamps` is a whole library: tools/blocks_probe.py points SACTD3_LIBRARY at it and the binding resolves every declared symbol,
    the environments' among them.  Built into a private directory and loaded in a fresh process (the binding caches its library)."""
    import subprocess
    import sys
    out_so = tmp_path / "libsactd3_hip_stamps.so"
    built = subprocess.run(["make", "-C", os.path.join(ROOT, "sac-td3-cudagraphs-pytorch_amd", "csrc"), "stamps", f"STAMPS_OUT={out_so}"],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout[-2000:]
    env = dict(os.environ, SACTD3_LIBRARY=str(out_so), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = ("import sac_td3_cudagraphs_pytorch_amd as P; lib = P.load_library(); assert P.library_path().endswith('stamps.so'); "
            "assert lib.sactd3_env_step(None, None, 0, None, None) == -1 and lib.sactd3_abi_version() == 1; print('loaded')")
    got = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert got.returncode == 0 and "loaded" in got.stdout, got.stderr[-2000:]
