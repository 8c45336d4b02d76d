"""CPU: the host side of the native rollout -- include/sactd3_rollout.h and its binding cover each other, the library builds and exports
it, every call refuses a NULL handle, `envs.pack_records` is the record layout include/sactd3.h states, `loop.train` and the launcher
refuse what they say they refuse, and `make asm` of engine.hip still gives the recorded machine code of every kernel."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import sac_td3_cudagraphs_pytorch_amd as P
from sac_td3_cudagraphs_pytorch_amd import _lib, envs, launcher, loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (ob_dim, ac_dim) -> (record_floats, next_obs_offset, next_obs_width) the engine reports (csrc/engine.hip: [s|a] and s' padded to 4
# floats, the record to 16): the pendulum, the cart-pole, and the Hopper for a layout with other pads
LAYOUTS = {(3, 1): (16, 4, 4), (4, 1): (16, 8, 4), (11, 3): (32, 16, 12)}


def declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return src, sorted(set(re.findall(r"\b(sactd3_[a-z0-9_]+)\s*\(", src)))


def test_header_and_binding_cover_each_other():
    src, names = declared("sactd3_rollout.h")
    assert names == sorted(_lib.ROLLOUT_SYMBOLS) and len(names) == 8
    assert all(n.startswith("sactd3_rollout_") for n in names)                                # none claims the env's prefix
    assert not set(_lib.ROLLOUT_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.ENV_SYMBOLS))
    assert {"sactd3_rb_extend_records_device", "sactd3_get_config"} <= set(_lib.SYMBOLS) and _lib.ABI_VERSION == 1
    assert declared("sactd3_env.h")[1] == sorted(_lib.ENV_SYMBOLS)                            # ... which is what it was
    P.build_library()                                                                         # hipcc --offload-arch=gfx950, here (a no-op when current)
    raw = C.CDLL(P.library_path())
    for name in names + ["sactd3_rb_extend_records_device", "sactd3_get_config"]:
        assert hasattr(raw, name), f"{name} is declared but not exported"
    lib = P.load_library()
    assert all(getattr(lib, name).argtypes is not None for name in names)
    # the struct mirrors have the C layout
    assert C.sizeof(_lib.CRecordLayout) == 12 and C.sizeof(_lib.CRolloutBuffers) == 40 and _lib.CRolloutBuffers.records.offset == 32
    for k, word in enumerate(("RANDOM", "EXPLORE", "EXPLOIT", "REPEAT")):
        assert re.search(rf"SACTD3_ROLLOUT_{word}\s*=\s*{k}\b", src) and getattr(_lib, "ROLLOUT_" + word) == k


def test_a_null_handle_is_refused_by_every_call():
    lib = P.load_library()
    lay, buf, h = _lib.CRecordLayout(16, 4, 4), _lib.CRolloutBuffers(), C.c_void_p()
    assert lib.sactd3_rollout_env_step(None, None, 1, C.byref(lay), None, None, 3, None) == _lib.EINVAL
    assert lib.sactd3_rollout_create(None, None, C.byref(buf), None, C.byref(h)) == _lib.EINVAL and not h.value
    assert b"NULL" in lib.sactd3_rollout_last_error(None)
    assert lib.sactd3_rollout_create(None, None, None, None, None) == _lib.EINVAL
    assert lib.sactd3_rollout_reset(None, 0) == _lib.EINVAL
    for mode in range(4):
        assert lib.sactd3_rollout_choose(None, mode) == _lib.EINVAL
    assert lib.sactd3_rollout_advance(None) == _lib.EINVAL
    assert lib.sactd3_rollout_stats(None, (C.c_int64 * 4)()) == _lib.EINVAL
    lib.sactd3_rollout_destroy(None)                                                          # a no-op
    assert lib.sactd3_rb_extend_records_device(None, None, 0, None, 0) == _lib.EINVAL
    assert lib.sactd3_get_config(None, C.byref(_lib.CConfig())) == _lib.EINVAL


def per_row(layout, o, a, obs, act, rew, nobs, done):
    """the layout comment of include/sactd3.h, one row and one field at a time:
    record = [s (ob_dim) | a (ac_dim) | 0-pad][s' (ob_dim) | 0-pad][r, d (0/1)][0-pad to a 64-byte multiple]"""
    rec_len, next_off, next_width = layout
    rows = []
    for i in range(len(obs)):
        row = [np.float32(0.0)] * rec_len
        for j in range(o):
            row[j] = obs[i][j]
        for j in range(a):
            row[o + j] = act[i][j]
        for j in range(o):
            row[next_off + j] = nobs[i][j]
        row[next_off + next_width] = rew[i]
        row[next_off + next_width + 1] = np.float32(1.0) if done[i] else np.float32(0.0)
        rows.append(np.array(row, np.float32))
    return np.stack(rows)


@pytest.mark.parametrize("dims", sorted(LAYOUTS))
def test_pack_records_is_the_layout_the_header_states(dims):
    o, a = dims
    layout = LAYOUTS[dims]
    assert layout[0] % 16 == 0 and layout[1] == -(-(o + a) // 4) * 4 and layout[2] == -(-o // 4) * 4      # 64-byte records, 16-byte fields
    rng = np.random.default_rng(o)
    n = 9
    obs, arrived, final = (rng.standard_normal((n, o)).astype(np.float32) for _ in range(3))
    act = rng.uniform(-3, 3, (n, a)).astype(np.float32)
    act[0, 0], act[1, 0], act[2, 0] = np.nan, np.inf, -0.0                                    # copied bit for bit
    rew = rng.standard_normal(n).astype(np.float32)
    term = np.arange(n) % 3 == 1
    trunc = np.arange(n) % 3 == 2                                                             # rows that are truncated, terminated or neither
    stored = np.where(trunc[:, None], final, arrived)                                         # the stored-next rule of the rollout
    got = envs.pack_records(layout, obs, act, rew, stored, term)
    want = per_row(layout, o, a, obs, act, rew, stored, term)
    assert got.dtype == np.float32 and got.shape == (n, layout[0]) and got.tobytes() == want.tobytes()
    tail = layout[1] + layout[2]
    assert np.array_equal(got[trunc, layout[1]:layout[1] + o], final[trunc]) and not got[trunc, tail + 1].any()      # a time limit is no termination
    assert np.array_equal(got[term, layout[1]:layout[1] + o], arrived[term]) and (got[term, tail + 1] == 1.0).all()
    # the dict of Engine.rb_layout() is the same layout; [n, 1] rewards and flags are the loop's shapes
    as_dict = dict(record_floats=layout[0], next_obs_offset=layout[1], next_obs_width=layout[2], capacity=7)
    assert envs.pack_records(as_dict, obs, act, rew.reshape(-1, 1), stored, term.reshape(-1, 1)).tobytes() == want.tobytes()
    for bad in ((layout[0], o + a - 1, layout[2]), (layout[0], layout[1], o - 1), (tail + 1, layout[1], layout[2])):
        with pytest.raises(ValueError):
            envs.pack_records(bad, obs, act, rew, stored, term)


def test_pack_records_of_a_host_env_step():
    """a HostVecEnv step packed with the rollout's stored-next rule: what NativeVecEnv.step_records writes for the same step"""
    env = envs.HostVecEnv("cartpole", 5, seed=2, horizon=3)
    obs, _ = env.reset(seed=2)
    layout = LAYOUTS[(4, 1)]
    ends = 0
    for _ in range(7):
        act = env.action_space.sample()
        nobs, rew, term, trunc, infos = env.step(act)
        stored = nobs.copy()
        for k in np.flatnonzero(trunc):
            stored[k] = infos["final_observation"][k]
        rec = envs.pack_records(layout, obs, act, rew, stored, term)
        assert rec.tobytes() == per_row(layout, 4, 1, obs, act, rew, stored, term).tobytes()
        ends += int(trunc.sum())
        obs = nobs
    assert ends >= 5


def test_train_refuses_what_it_says():
    cfg = SimpleNamespace(seed=0, learning_starts=10, action_repeat=1, segment_len=1, num_envs=2, num_timesteps=10, eval_every=10, batch_size=4)
    agent = SimpleNamespace(rb=object(), timesteps_so_far=0, predict_begin=lambda *a, **k: None, predict_end=lambda: None)
    host_env = envs.HostVecEnv("pendulum", 2)
    with pytest.raises(ValueError, match="device_env"):
        loop.train(cfg, host_env, agent, native_rollout=True)
    with pytest.raises(ValueError, match="overlap"):
        loop.train(cfg, host_env, agent, native_rollout=True, overlap=True)
    with pytest.raises(ValueError, match="overlap"):
        loop.train(cfg, host_env, agent, native_rollout=True, overlap=True, device_env=True)
    with pytest.raises(TypeError, match="step_records"):
        loop.train(cfg, host_env, agent, native_rollout=True, device_env=True)               # no env that emits records
    with pytest.raises(TypeError, match="step_records"):
        loop.NativeRollout(host_env, agent, 0, 10, 1)
    assert callable(envs.NativeVecEnv.step_records)


def test_launcher_plans_and_refuses_the_native_rollout():
    assert launcher.env_plan("CartPole-native", True, native_rollout=True) == dict(train="NativeVecEnv", eval="NativeVecEnv", rollout="NativeRollout")
    assert launcher.env_plan("CartPole-native", True, native_rollout=False)["rollout"] == "DeviceRollout"      # the default stays
    assert launcher.env_plan("Hopper-v4", True, native_rollout=False)["rollout"] == "DeviceRollout"
    assert launcher.env_plan("Hopper-v4", False, native_rollout=False)["rollout"] == "Rollout"
    assert launcher.env_plan("CartPole-native", True) == dict(train="NativeVecEnv", eval="NativeVecEnv")       # not asked: the plan it was
    with pytest.raises(ValueError, match="--device_env"):
        launcher.env_plan("CartPole-native", False, native_rollout=True)
    with pytest.raises(ValueError, match="-native"):
        launcher.env_plan("Hopper-v4", True, native_rollout=True)
    with pytest.raises(ValueError, match="-native"):
        launcher.env_plan("Pendulum-native", True, has_factory=True, native_rollout=True)
    with pytest.raises(ValueError):
        launcher.run_job("sac", "Hopper-v4", 0, 0, "unused", device_env=True, native_rollout=True)            # before anything is built
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "sac_td3_cudagraphs_pytorch_amd.launcher", "--num_seeds", "1", "--dry-run"]

    def run(*more):
        return subprocess.run(base + list(more), capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
    out = run("--env_bundle", "native", "--device_env", "--native_rollout")
    assert out.returncode == 0, out.stderr[-2000:]
    jobs = [json.loads(ln[4:]) for ln in out.stdout.splitlines() if ln.startswith("JOB ")]
    assert [j["env_id"] for j in jobs] == ["Pendulum-native", "CartPole-native"] and all(j["rollout"] == "NativeRollout" and j["dry_run"] for j in jobs)
    out = run("--env_bundle", "native", "--device_env")
    assert out.returncode == 0 and all(json.loads(ln[4:])["rollout"] == "DeviceRollout" for ln in out.stdout.splitlines() if ln.startswith("JOB "))
    out = run("--env_bundle", "native", "--native_rollout")
    assert out.returncode == 2 and "--device_env" in out.stderr and "JOB " not in out.stdout
    out = run("--env_bundle", "debug", "--device_env", "--native_rollout")
    assert out.returncode == 2 and "-native" in out.stderr and "JOB " not in out.stdout


def test_engine_kernels_are_the_recorded_machine_code(tmp_path):
    """`make asm` of engine.hip against tests/golden/engine_kernels_sha256.json (tools/asm_same.py --record, taken from the commit in front
    of the native rollout): the same kernel symbols, each with the same body -- the rollout added host code to engine.hip and no kernel.
    A change that means to alter a kernel renews the record and says so in DESIGN.md section 4."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import asm_same
    path = tmp_path / "sactd3_engine.s"
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "sac-td3-cudagraphs-pytorch_amd", "csrc"), "asm", f"ASM_OUT={path}"],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    with open(asm_same.RECORD) as f:
        recorded = json.load(f)["kernels"]
    got = asm_same.digests(str(path))
    assert len(recorded) >= 115 and sorted(got) == sorted(recorded)
    assert not [name for name in recorded if got[name] != recorded[name]]
