"""Three real continuous-control tasks for the engine to train on, on the GPU and on the host (include/sactd3_env.h):

  NativeVecEnv    the vector env that lives on the GPU (csrc/env_kernels.h): `step` is ONE kernel launch on the current torch stream,
                  every array a device tensor, no host draw, no host wait, no torch arithmetic -- the protocol `loop.DeviceRollout`
                  consumes (`loop.train(device_env=True)`); `step_records` is the same step writing its transitions as ring records
                  into the caller's slab (include/sactd3_rollout.h), which `loop.NativeRollout` drives (`native_rollout=True`)
  pack_records    the ring's record layout in numpy: what `step_records` writes, for the host twin's users and for tests
  HostVecEnv      the same tasks in numpy float32, in the kernel's operation order and with the same Philox resets, with the
                  gymnasium-0.29 protocol of `loop.SyntheticVecEnv` -- for `loop.Rollout`, `loop.Evaluator` and `loop.evaluate`
  greedy_returns  evaluation with one host wait: a vector env stepped in lock-step with the agent's greedy action for one horizon
  device_episodes the same as an episode generator, to stand in for `loop.Evaluator.ep_gen`
  policy_rollout  on-policy episodes of a NativeVecEnv in ONE kernel launch (include/sactd3_eval.h): summaries, and on request the
                  trajectories with their returns-to-go; `greedy_returns(one_launch=True)` goes through the same launch
  q_bias          the normalised Q-bias of the current policy: Q(s, a) against its Monte-Carlo return on fresh episodes

The tasks (textbook physics: the torque-limited pendulum swing-up; the cart-pole of Barto, Sutton & Anderson 1983 with a continuous
force; a 2-D point mass that has to reach a goal drawn per episode, with a sparse reward) and the random streams are stated in
include/sactd3_env.h.  The host twin computes, bit for bit, what the kernel computes except through sin / cos: the reset states, the
random actions, the flags' rules and the fp32 accumulation of the returns are the same bits -- and the point mass, which calls no
libm function, is the same bits throughout."""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Generator, Optional

import numpy as np

from . import _lib

KINDS = {"pendulum": _lib.ENV_PENDULUM, "cartpole": _lib.ENV_CARTPOLE, "pointgoal": _lib.ENV_POINTGOAL}
#        kind -> (ob_dim, ac_dim, action bound, default horizon, floats of physical state)
SPECS = {_lib.ENV_PENDULUM: (3, 1, 2.0, 200, 2), _lib.ENV_CARTPOLE: (4, 1, 1.0, 200, 4), _lib.ENV_POINTGOAL: (6, 2, 1.0, 50, 4)}
# where a goal-conditioned task keeps its goals in an observation, and when it counts as reached (include/sactd3_env.h)
GOAL_LAYOUTS = {_lib.ENV_POINTGOAL: dict(achieved=0, desired=4, dim=2, threshold=0.1)}
STREAM_ENV = 0x500          # csrc/env_kernels.h: SACTD3_STREAM_ENV
F = np.float32
GOAL_THR = F(0.1)           # csrc/env_kernels.h: ENV_GOAL_THR
PI, TWO_PI, INV_2PI = F(3.14159274), F(6.28318548), F(0.159154937)       # csrc/env_kernels.h: ENV_PI, ENV_TWO_PI, ENV_INV_2PI
X_LIMIT, THETA_LIMIT = F(2.4), F(0.20943951)


def kind_of(kind) -> int:
    if isinstance(kind, str):
        if kind.lower() not in KINDS:
            raise ValueError(f"unknown env kind {kind!r} (one of {sorted(KINDS)})")
        return KINDS[kind.lower()]
    if int(kind) not in SPECS:
        raise ValueError(f"unknown env kind {kind!r}")
    return int(kind)


# ---------------------------------------------------------------------------------------------------- Philox4x32-10 in numpy
def philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """csrc/philox.h: philox4x32_10, vectorised over the counter words -> four uint32 arrays"""
    m = np.uint64(0xFFFFFFFF)
    c = [np.asarray(x, np.uint64) & m for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        n0 = (p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)
        c = [n0, p1 & m, n2, p0 & m]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def u01(x):
    """csrc/philox.h: philox_u01 in numpy float32"""
    return ((np.asarray(x, np.uint32) >> np.uint32(8)).astype(F) + F(0.5)) * F(1.0 / 16777216.0)


def _words(seed: int, first, env_index, which: int):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10(first, env_index, STREAM_ENV, which, seed & 0xFFFFFFFF, seed >> 32)


def first_states(kind: int, seed: int, env_index, episode) -> np.ndarray:
    """[n, 4] float32: the state in which episode `episode[k]` of env `env_index[k]` starts -- a pure function of (seed, env, episode)"""
    u = np.stack([u01(w) for w in _words(seed, np.asarray(episode), np.asarray(env_index), 0)], 1)
    s = np.zeros(u.shape, F)
    if kind == _lib.ENV_PENDULUM:
        s[:, 0] = -PI + TWO_PI * u[:, 0]
        s[:, 1] = F(-1.0) + F(2.0) * u[:, 1]
    elif kind == _lib.ENV_CARTPOLE:
        s[:] = F(-0.05) + F(0.1) * u
    else:
        s[:, :2] = F(-1.0) + F(2.0) * u[:, :2]
    return s


def goals(kind: int, seed: int, env_index, episode) -> np.ndarray:
    """[n, 2] float32: the goal of episode `episode[k]` of env `env_index[k]` -- a pure function of (seed, env, episode); zeros for a
    task without one"""
    w = _words(seed, np.asarray(episode), np.asarray(env_index), 2)
    if kind != _lib.ENV_POINTGOAL:
        return np.zeros((len(w[0]), 2), F)
    return np.stack([F(-1.0) + F(2.0) * u01(w[0]), F(-1.0) + F(2.0) * u01(w[1])], 1).astype(F)


def random_actions(kind: int, seed: int, env_index, draw) -> np.ndarray:
    """[n, ac_dim] float32: random action number `draw[k]` of env `env_index[k]`, uniform inside the bounds; dimension j takes word j"""
    bound = F(SPECS[kind][2])
    w = _words(seed, np.asarray(draw), np.asarray(env_index), 1)
    return np.stack([(-bound + (bound - (-bound)) * u01(w[j])).astype(F) for j in range(SPECS[kind][1])], 1)


# ---------------------------------------------------------------------------------------------------- the physics, float32
def _angnorm(x):
    return x - TWO_PI * np.floor((x + PI) * INV_2PI)


def goal_reward(achieved: np.ndarray, goal: np.ndarray) -> np.ndarray:
    """csrc/env_kernels.h: env_goal_reward in numpy float32: [n, 2] against [n, 2] -> [n], 0 on the goal and -1 off it"""
    assert achieved.dtype == F and goal.dtype == F
    dx, dy = achieved[:, 0] - goal[:, 0], achieved[:, 1] - goal[:, 1]
    d2 = (dx * dx) + (dy * dy)
    return np.where(d2 <= (GOAL_THR * GOAL_THR), F(0.0), F(-1.0)).astype(F)


def physics(kind: int, s: np.ndarray, u: np.ndarray, goal: Optional[np.ndarray] = None):
    """csrc/env_kernels.h: env_physics line for line in numpy float32.  s [n, 4], u [n] ([n, 2] for the point mass) clamped and finite,
    goal [n, 2] of the running episodes (the point mass only) -> (s2 [n, 4], reward [n], terminal [n])"""
    assert s.dtype == F and u.dtype == F
    s2 = np.zeros_like(s)
    if kind == _lib.ENV_POINTGOAL:
        v = (F(0.8) * s[:, 2:4]) + (F(0.2) * u)
        s2[:, 0:2] = np.minimum(np.maximum(s[:, 0:2] + (F(0.1) * v), F(-1.0)), F(1.0))
        s2[:, 2:4] = v
        assert s2.dtype == F
        return s2, goal_reward(s2[:, 0:2], np.asarray(goal, F)), np.zeros(len(s), bool)
    if kind == _lib.ENV_PENDULUM:
        th, w = s[:, 0], s[:, 1]
        thn = _angnorm(th)
        cost = ((thn * thn) + (F(0.1) * (w * w))) + (F(0.001) * (u * u))
        acc = (F(15.0) * np.sin(th)) + (F(3.0) * u)
        w2 = np.minimum(np.maximum(w + (acc * F(0.05)), F(-8.0)), F(8.0))
        s2[:, 0] = _angnorm(th + (F(0.05) * w2))
        s2[:, 1] = w2
        return s2, -cost, np.zeros(len(u), bool)
    x, xd, th, thd = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    f = F(10.0) * u
    c, sn = np.cos(th), np.sin(th)
    temp = (f + ((F(0.05) * (thd * thd)) * sn)) / F(1.1)
    den = F(0.5) * (F(1.33333337) - ((F(0.1) * (c * c)) / F(1.1)))
    thacc = ((F(9.8) * sn) - (c * temp)) / den
    xacc = temp - (((F(0.05) * thacc) * c) / F(1.1))
    s2[:, 0] = x + (F(0.02) * xd)
    s2[:, 1] = xd + (F(0.02) * xacc)
    s2[:, 2] = th + (F(0.02) * thd)
    s2[:, 3] = thd + (F(0.02) * thacc)
    assert s2.dtype == F
    return s2, np.ones(len(u), F), (np.abs(s2[:, 0]) > X_LIMIT) | (np.abs(s2[:, 2]) > THETA_LIMIT)


def observe(kind: int, s: np.ndarray, goal: Optional[np.ndarray] = None) -> np.ndarray:
    if kind == _lib.ENV_PENDULUM:
        return np.stack([np.cos(s[:, 0]), np.sin(s[:, 0]), s[:, 1]], 1).astype(F)
    if kind == _lib.ENV_POINTGOAL:
        return np.concatenate([s.astype(F), np.asarray(goal, F)], 1)
    return s.astype(F).copy()


def clean_actions(kind: int, actions, n: int):
    """-> (u [n] float32 clamped ([n, ac_dim] where ac_dim > 1), bad [n] bool): a NaN or infinite action component is replaced by 0;
    `bad` marks the steps with any such component"""
    ac = SPECS[kind][1]
    a = np.asarray(actions, F).reshape(n, -1)[:, :ac]
    nonfinite = ~np.isfinite(a)
    bound = F(SPECS[kind][2])
    u = np.minimum(np.maximum(np.where(nonfinite, F(0.0), a), -bound), bound).astype(F)
    return (u[:, 0] if ac == 1 else u), nonfinite.any(1)


# ---------------------------------------------------------------------------------------------------- the host twin
class _HostBox:
    def __init__(self, env):
        self._env = env
        bound = SPECS[env.kind][2]
        self.low, self.high = np.full(SPECS[env.kind][1], -bound, F), np.full(SPECS[env.kind][1], bound, F)

    def sample(self):
        e = self._env
        out = random_actions(e.kind, e.seed, np.arange(e.n), e.draws)
        e.draws = e.draws + np.uint32(1)
        return out


class HostVecEnv:
    """The tasks on the host, float32 numpy in the kernel's operation order, with gymnasium-0.29 autoreset semantics as
    `loop.SyntheticVecEnv` has them: on termination or truncation `infos["final_observation"][k]` (an object array) holds the
    observation the step arrived at, `infos["final_info"][k]["episode"]` its length `l` and return `r`, and the returned observation
    is the next episode's first one.  Episode k of env i starts where it starts on the GPU (the same Philox draw)."""

    def __init__(self, kind, num_envs: int, seed: int = 0, horizon: Optional[int] = None):
        self.kind = kind_of(kind)
        self.o, self.a, self.bound, default_horizon, _ = SPECS[self.kind]
        self.goal_layout = dict(GOAL_LAYOUTS[self.kind]) if self.kind in GOAL_LAYOUTS else None
        self.n = self.num_envs = int(num_envs)
        if self.n < 1:
            raise ValueError("num_envs must be >= 1")
        self.horizon = int(horizon) if horizon else default_horizon
        self.seed = int(seed)
        self.action_space = _HostBox(self)
        self.reset(seed=self.seed)

    def reset(self, seed=None):
        if seed is not None:
            self.seed = int(seed)
        n = self.n
        self.s = first_states(self.kind, self.seed, np.arange(n), np.zeros(n, np.uint32))
        self.goal = goals(self.kind, self.seed, np.arange(n), np.zeros(n, np.uint32))
        self.t = np.zeros(n, np.int32)
        self.ep = np.zeros(n, np.uint32)
        self.ret = np.zeros(n, F)
        self.draws = np.zeros(n, np.uint32)
        self._done, self._bad = np.zeros(n, np.int64), 0
        self._ret_sum, self._len_sum = 0.0, 0
        self._last_ret, self._last_len = np.zeros(n, F), np.zeros(n, np.int32)
        self._first_ret, self._first_len = np.zeros(n, F), np.zeros(n, np.int32)
        return observe(self.kind, self.s, self.goal), {}

    def step(self, actions):
        n = self.n
        u, bad = clean_actions(self.kind, actions, n)
        self._bad += int(bad.sum())
        s2, rew, term = physics(self.kind, self.s, u, self.goal)
        self.t = self.t + np.int32(1)
        self.ret = (self.ret + rew).astype(F)
        trunc = (self.t >= self.horizon) & ~term
        ended = term | trunc
        infos: Dict[str, Any] = {}
        if ended.any():
            final = observe(self.kind, s2, self.goal)      # (against the goal of the episode that ends)
            infos["final_observation"] = np.array([final[k].copy() if ended[k] else None for k in range(n)], dtype=object)
            infos["final_info"] = np.array([{"episode": {"l": np.array([self.t[k]]), "r": np.array([self.ret[k]])}} if ended[k] else None
                                            for k in range(n)], dtype=object)
            at = np.flatnonzero(ended)
            new = at[self._done[at] == 0]                     # the first episode an env finishes since the reset
            self._first_ret[new], self._first_len[new] = self.ret[new], self.t[new]
            self._done[at] += 1
            self._ret_sum += float(self.ret[at].astype(np.float64).sum())
            self._len_sum += int(self.t[at].sum())
            self._last_ret[at], self._last_len[at] = self.ret[at], self.t[at]
            self.ep[at] += np.uint32(1)
            s2[at] = first_states(self.kind, self.seed, at, self.ep[at])
            self.goal[at] = goals(self.kind, self.seed, at, self.ep[at])
            self.t[at] = 0
            self.ret[at] = 0.0
        self.s = s2
        return observe(self.kind, self.s, self.goal), rew.astype(F), term, trunc, infos

    def episode_stats(self) -> Dict[str, Any]:
        return {"episodes": int(self._done.sum()), "return_sum": self._ret_sum, "length_sum": self._len_sum, "bad_actions": self._bad,
                "last_return": self._last_ret.copy(), "last_length": self._last_len.copy(), "env_episodes": self._done.copy(),
                "first_return": self._first_ret.copy(), "first_length": self._first_len.copy()}

    def state(self) -> Dict[str, np.ndarray]:
        return {"phys": self.s.copy(), "steps": self.t.copy(), "episode": self.ep.copy(), "returns": self.ret.copy(), "draws": self.draws.copy()}

    def set_state(self, state) -> None:
        _check_state(state, self.n)
        for key, name, dt in (("phys", "s", F), ("steps", "t", np.int32), ("episode", "ep", np.uint32), ("returns", "ret", F), ("draws", "draws", np.uint32)):
            if key in state:
                setattr(self, name, np.array(state[key], dt).reshape(getattr(self, name).shape))
        self.goal = goals(self.kind, self.seed, np.arange(self.n), self.ep)      # (not state: a function of the episode index)


_STATE_KEYS = {"phys": (F, _lib.ENV_STATE_DIM), "steps": (np.int32, 1), "episode": (np.uint32, 1), "returns": (F, 1), "draws": (np.uint32, 1)}


def _check_state(state, n: int) -> None:
    unknown = set(state) - set(_STATE_KEYS)
    if unknown:
        raise ValueError(f"set_state: unknown keys {sorted(unknown)}")
    for k, v in state.items():
        if np.asarray(v).size != n * _STATE_KEYS[k][1]:
            raise ValueError(f"set_state: {k} must have {n} x {_STATE_KEYS[k][1]} elements")
    if "phys" in state and not np.isfinite(np.asarray(state["phys"], np.float64)).all():
        raise ValueError("set_state: a physical state is not finite")
    if "steps" in state and (np.asarray(state["steps"]) < 0).any():
        raise ValueError("set_state: a step count is negative")


# ---------------------------------------------------------------------------------------------------- transitions as ring records
def _layout_triple(layout):
    """(record_floats, next_obs_offset, next_obs_width) of Engine.rb_layout()'s dict, or of a triple given as such"""
    if isinstance(layout, dict):
        return int(layout["record_floats"]), int(layout["next_obs_offset"]), int(layout["next_obs_width"])
    rec, off, width = layout
    return int(rec), int(off), int(width)


def pack_records(layout, obs, actions, rewards, next_obs, dones) -> np.ndarray:
    """[n, record_floats] float32: n transitions as records of the engine's replay ring (include/sactd3.h: sactd3_rb_layout) --
        [s (ob_dim) | a (ac_dim) | 0-pad to next_obs_offset][s' (ob_dim) | 0-pad to next_obs_width][r, d (0 / 1)][0-pad]
    every value copied bit for bit, every pad float +0.  `next_obs` is the STORED next observation: for a `HostVecEnv` step the
    arrival observation where the step was truncated (infos["final_observation"]), otherwise the one returned -- which is what
    `NativeVecEnv.step_records` writes on the device.  With a host env, `agent.rb.extend_records(torch.as_tensor(rows, device=...))`
    appends the rows."""
    rec, off, width = _layout_triple(layout)
    obs, next_obs = np.asarray(obs, F), np.asarray(next_obs, F)
    n = obs.shape[0]
    obs, next_obs, actions = obs.reshape(n, -1), next_obs.reshape(n, -1), np.asarray(actions, F).reshape(n, -1)
    o, a = obs.shape[1], actions.shape[1]
    if off < o + a or width < o or rec < off + width + 2 or next_obs.shape != obs.shape:
        raise ValueError(f"pack_records: layout {(rec, off, width)} does not hold observations [{n}, {o}] and actions [{n}, {a}]")
    out = np.zeros((n, rec), F)
    out[:, :o], out[:, o:o + a], out[:, off:off + o] = obs, actions, next_obs
    out[:, off + width] = np.asarray(rewards, F).reshape(n)
    out[:, off + width + 1] = (np.asarray(dones).reshape(n) != 0).astype(F)
    return out


# ---------------------------------------------------------------------------------------------------- the env on the GPU
class _DeviceBox:
    def __init__(self, env):
        self._env = env
        self.low, self.high = np.full(env.a, -env.bound, F), np.full(env.a, env.bound, F)

    def sample(self):
        """[n, ac_dim] device tensor drawn by the device (sactd3_env_sample_actions): no host draw, no upload"""
        e = self._env
        out = e._empty((e.n, e.a), e._t.float32)
        e._call("sactd3_env_sample_actions", out.data_ptr(), out.stride(0), e._stream())
        return out


class NativeVecEnv:
    """The vector env on the GPU (include/sactd3_env.h), with the protocol `loop.DeviceRollout` consumes:
      reset(seed) -> (obs [n, o], {});   step(actions [n, a]) -> (obs, rewards [n], terminations [n], truncations [n], infos)
      infos["final_observation"]: [n, o], what the step arrived at BEFORE any reset, for every env; infos["_final_observation"]: [n]
      bool, the envs that ended;   action_space.sample() -> [n, a] drawn on the device.
    A step is one kernel launch on the current torch stream of the env's device.  Its outputs are FRESH tensors of torch's caching
    allocator on that stream -- never a buffer an earlier step handed out: `DeviceRollout.advance` still holds the previous
    observations while the next step runs and `rb.extend` reads them afterwards.  Nothing here reads a device value on the host;
    `episode_stats()`, `state()` and `set_state()` do, and wait."""

    def __init__(self, kind, num_envs: int, seed: int = 0, device: Any = None, horizon: Optional[int] = None):
        import torch
        self._t = torch
        self.kind = kind_of(kind)
        self.n = self.num_envs = int(num_envs)
        self.seed = int(seed)
        self.lib = _lib.load_library()
        if device is not None:
            self.device = torch.device(device)
            if self.device.type != "cuda":
                raise ValueError(f"NativeVecEnv lives on a GPU, not on {self.device} (HostVecEnv is the host twin)")
            if self.device.index is None:
                self.device = torch.device("cuda", torch.cuda.current_device())
        else:
            self.device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        cfg = _lib.CEnvConfig(self.kind, self.n, int(horizon or 0), int(self.device.index), self.seed & 0xFFFFFFFFFFFFFFFF)
        h = C.c_void_p()
        rc = self.lib.sactd3_env_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise _lib.EngineError(f"sactd3_env_create failed ({rc}): {self.lib.sactd3_env_last_error(None).decode()}")
        self._h = h
        info = _lib.CEnvInfo()
        self._call("sactd3_env_spec", C.byref(info))
        self.o, self.a, self.horizon, self.bound = int(info.ob_dim), int(info.ac_dim), int(info.horizon), float(info.max_ac)
        self.goal_layout = dict(GOAL_LAYOUTS[self.kind]) if self.kind in GOAL_LAYOUTS else None
        self.action_space = _DeviceBox(self)

    # -- plumbing
    def _call(self, name, *args):
        if self._h is None:
            raise _lib.EngineError(f"{name}: the env is closed")
        rc = getattr(self.lib, name)(self._h, *args)
        if rc != 0:
            raise _lib.EngineError(f"{name} failed ({rc}): {self.lib.sactd3_env_last_error(self._h).decode()}")

    def _stream(self) -> int:
        return int(self._t.cuda.current_stream(self.device).cuda_stream)

    def _empty(self, shape, dtype):
        return self._t.empty(shape, dtype=dtype, device=self.device)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            self.lib.sactd3_env_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001 -- interpreter shutdown
            pass

    # -- the protocol
    def reset(self, seed=None):
        if seed is not None:
            self.seed = int(seed)
        obs = self._empty((self.n, self.o), self._t.float32)
        self._call("sactd3_env_reset", self.seed & 0xFFFFFFFFFFFFFFFF, obs.data_ptr(), obs.stride(0), self._stream())
        return obs, {}

    def step(self, actions):
        t, n = self._t, self.n
        a = actions
        if not (t.is_tensor(a) and a.device == self.device and a.dtype == t.float32 and a.dim() == 2 and a.shape == (n, self.a)
                and a.stride(1) == 1 and a.stride(0) >= self.a):
            a = t.as_tensor(a, dtype=t.float32, device=self.device).reshape(n, self.a).contiguous()
        obs, final = self._empty((n, self.o), t.float32), self._empty((n, self.o), t.float32)
        rew = self._empty((n,), t.float32)
        flags = self._empty((3, n), t.bool)                   # one byte each: the kernel writes 0 / 1
        out = _lib.CEnvOut(obs.data_ptr(), obs.stride(0), final.data_ptr(), final.stride(0), rew.data_ptr(), 1,
                           flags[0].data_ptr(), 1, flags[1].data_ptr(), 1, flags[2].data_ptr(), 1)
        self._call("sactd3_env_step", a.data_ptr(), a.stride(0), C.byref(out), self._stream())
        return obs, rew, flags[0], flags[1], {"final_observation": final, "_final_observation": flags[2]}

    def step_records(self, actions, layout, records, obs) -> None:
        """One vector step that writes env i's transition as row i of `records`, in the engine's ring layout, and the observations to
        act on next into `obs` -- both the CALLER's tensors, nothing is allocated (include/sactd3_rollout.h: sactd3_rollout_env_step;
        one launch of k_env_step_rec on the current torch stream).  State, books and `obs` are those of step().  `layout`:
        Engine.rb_layout() (or a (record_floats, next_obs_offset, next_obs_width) triple); `records`: float32 [n, record_floats],
        contiguous, 16-byte aligned -- what `ReplayBuffer.extend_records` appends; `pack_records` states what a row holds."""
        lay = _lib.CRecordLayout(*_layout_triple(layout))
        self._call("sactd3_rollout_env_step", actions.data_ptr(), actions.stride(0), C.byref(lay), records.data_ptr(), obs.data_ptr(),
                   obs.stride(0), self._stream())

    # -- bookkeeping: these wait for the device
    def episode_stats(self) -> Dict[str, Any]:
        last_ret, last_len, eps = np.zeros(self.n, F), np.zeros(self.n, np.int32), np.zeros(self.n, np.int64)
        first_ret, first_len = np.zeros(self.n, F), np.zeros(self.n, np.int32)
        st = _lib.CEnvStats(0, 0.0, 0, 0, last_ret.ctypes.data, last_len.ctypes.data, eps.ctypes.data, first_ret.ctypes.data, first_len.ctypes.data)
        self._call("sactd3_env_episode_stats", C.byref(st), self._stream())
        return {"episodes": int(st.episodes), "return_sum": float(st.return_sum), "length_sum": int(st.length_sum),
                "bad_actions": int(st.bad_actions), "last_return": last_ret, "last_length": last_len, "env_episodes": eps,
                "first_return": first_ret, "first_length": first_len}

    def state(self) -> Dict[str, np.ndarray]:
        out = {k: np.zeros((self.n, w) if w > 1 else self.n, dt) for k, (dt, w) in _STATE_KEYS.items()}
        st = _lib.CEnvState(*[out[k].ctypes.data for k in ("phys", "steps", "episode", "returns", "draws")])
        self._call("sactd3_env_get_state", C.byref(st), self._stream())
        return out

    def set_state(self, state) -> None:
        _check_state(state, self.n)
        keep = {k: np.ascontiguousarray(np.asarray(v, _STATE_KEYS[k][0]).reshape(-1)) for k, v in state.items()}
        st = _lib.CEnvState(*[keep[k].ctypes.data if k in keep else None for k in ("phys", "steps", "episode", "returns", "draws")])
        self._call("sactd3_env_set_state", C.byref(st), self._stream())


# ---------------------------------------------------------------------------------------------------- evaluation with one host wait
def _greedy_actions(env, agent, obs):
    """the agent's greedy action for every row of `obs`, in calls of at most the engine's max_envs rows"""
    n = env.num_envs
    limit = int(getattr(getattr(getattr(agent, "engine", None), "cfg", None), "max_envs", n)) or n
    if isinstance(env, NativeVecEnv):
        if n <= limit:
            return agent.predict_device({"observations": obs}, explore=False)
        out = env._empty((n, env.a), env._t.float32)
        for lo in range(0, n, limit):
            agent.predict_device({"observations": obs[lo:lo + limit]}, explore=False, out=out[lo:lo + limit])
        return out
    return np.concatenate([np.asarray(agent.predict({"observations": obs[lo:lo + limit]}, explore=False), F).reshape(-1, env.a)
                           for lo in range(0, n, limit)])


def _native_for_rollout(env, agent, what: str):
    """the engine of `agent`, after the refusals of everything that goes through sactd3_eval_rollout"""
    if not isinstance(env, NativeVecEnv):
        raise TypeError(f"{what}: the one-launch rollout needs a NativeVecEnv -- the env's physics runs inside the kernel; a host env "
                        f"({type(env).__name__}) is stepped by greedy_returns' default loop")
    eng = getattr(agent, "engine", None)
    if eng is None or not hasattr(eng, "eval_rollout"):
        raise TypeError(f"{what}: the agent has no engine to roll the env with")
    return eng


def _rollout_launch(env, agent, what: str, steps, mode, seed, gamma, soft, trajectories, reset):
    """the launch of policy_rollout, nothing read: -> (T, summary: one uint8 device buffer, its views {name: tensor}, trajectories {name: tensor})"""
    eng = _native_for_rollout(env, agent, what)
    if mode not in ("greedy", "sample"):
        raise ValueError(f"{what}: mode must be 'greedy' or 'sample', not {mode!r}")
    t, n = env._t, env.n
    T = int(env.horizon if steps is None else steps)
    if not 1 <= T <= _lib.EVAL_MAX_STEPS:
        raise ValueError(f"{what}: steps must be in [1, {_lib.EVAL_MAX_STEPS}], not {T}")
    if seed is not None and not reset:
        raise ValueError(f"{what}: a seed is for reset=True")
    # the summary as ONE device buffer, so that one copy reads it: three [n] word arrays, alpha, then the [n] bytes
    summary = env._empty((4 * (3 * n + 1) + n,), t.uint8)
    words = summary[:4 * (3 * n + 1)]
    views = {"ep_return": words[:4 * n].view(t.float32), "g0": words[4 * n:8 * n].view(t.float32), "ep_length": words[8 * n:12 * n].view(t.int32),
             "alpha": words[12 * n:].view(t.float32), "ep_terminated": summary[4 * (3 * n + 1):]}
    traj = {}
    if trajectories:
        traj = {"obs": env._empty((T, n, env.o), t.float32), "actions": env._empty((T, n, env.a), t.float32),
                "eps": env._empty((T, n, env.a), t.float32), "reward": env._empty((T, n), t.float32), "logp": env._empty((T, n), t.float32),
                "rtg": env._empty((T, n), t.float32), "live": env._empty((T, n), t.uint8)}
    if reset and seed is not None:
        env.seed = int(seed)
    eng.eval_rollout(env._h, {k: v.data_ptr() for k, v in {**views, **traj}.items()}, steps=T, sample=mode == "sample", reset=reset, soft=soft,
                     gamma=gamma, seed=env.seed & 0xFFFFFFFFFFFFFFFF, stream=env._stream())
    return T, summary, views, traj


def policy_rollout(env, agent, *, steps: Optional[int] = None, mode: str = "greedy", seed: Optional[int] = None, gamma: Optional[float] = None,
                   soft: bool = False, trajectories: bool = False, reset: bool = True) -> Dict[str, Any]:
    """On-policy episodes in ONE kernel launch (include/sactd3_eval.h): the envs of a NativeVecEnv rolled for `steps` steps (None: one
    horizon) under the agent's online actor -- `mode` "greedy" (the exploit action) or "sample" (SAC: a sampled action with its
    log-prob) -- on the engine's stream, ordered against the current torch stream on the GPU.  `reset`: the env is reset first (`seed`:
    its own if None); otherwise it goes on from where it is.  `gamma` None: the engine's.  `soft`: entropy terms in the returns-to-go.
    -> {"ep_return", "ep_length", "ep_terminated", "g0": numpy [n], about the episode each env was in at the call's first step (length 0:
    still open at the end); "alpha"; "steps"} -- read with one host wait; with `trajectories` also the device tensors "obs" [T, n, o],
    "actions", "eps" [T, n, a], "reward", "logp", "rtg" [T, n] float32 and "live" [T, n] uint8, which that wait covers too."""
    T, summary, _, traj = _rollout_launch(env, agent, "policy_rollout", steps, mode, seed, gamma, soft, trajectories, reset)
    n = env.n
    host = summary.cpu().numpy()                              # the call's one host wait
    w = host[:4 * (3 * n + 1)]
    out = {"ep_return": w[:4 * n].view(F).copy(), "g0": w[4 * n:8 * n].view(F).copy(), "ep_length": w[8 * n:12 * n].view(np.int32).copy(),
           "alpha": float(w[12 * n:].view(F)[0]), "ep_terminated": host[4 * (3 * n + 1):].astype(bool), "steps": T}
    out.update(traj)
    return out


def q_bias(env, agent, *, seed: int, gamma: Optional[float] = None, mode: Optional[str] = None, tail_tol: float = 0.05) -> Dict[str, Any]:
    """The normalised Q-bias of the REDQ / DroQ / reset papers: Q(s, a) against the discounted Monte-Carlo return of the CURRENT policy
    from (s, a), on fresh on-policy episodes.  One policy_rollout with trajectories (reset to `seed`, one horizon), then agent.q_values
    on the recorded (o_t, a_t) rows; nothing leaves the device until the final statistics.  q_t = min_k Q_k, bias_t = q_t - G_t.
    Rows counted: every live row of an episode that terminated; of a truncated episode only those with gamma^(L - t) <= tail_tol,
    because its return lacks the tail behind the time limit.  `mode` None: "sample" with entropy terms for SAC (the soft return the
    critics are trained towards), "greedy" for TD3.
    -> {"mean", "std": of bias / |mean G| over the counted rows, "bias_mean", "bias_std", "return_mean", "rows"}"""
    eng = _native_for_rollout(env, agent, "q_bias")
    t = env._t
    sac = not bool(eng.cfg.prefer_td3_over_sac)
    mode = ("sample" if sac else "greedy") if mode is None else mode
    g = float(np.float32(eng.cfg.gamma if gamma is None else gamma))
    if not 0.0 < float(tail_tol) <= 1.0:
        raise ValueError("q_bias: tail_tol must be in (0, 1]")
    T, _, views, got = _rollout_launch(env, agent, "q_bias", None, mode, seed, g, sac and mode == "sample", True, True)
    n = env.n
    q = agent.q_values({"observations": got["obs"].view(T * n, env.o), "actions": got["actions"].view(T * n, env.a)})
    qmin = q.view(2, T, n).min(0).values.double()
    G = got["rtg"].double()
    L, terminated = views["ep_length"].long(), views["ep_terminated"] != 0
    left = (L.view(1, n) - t.arange(T, device=env.device).view(T, 1)).clamp(min=0).double()      # L - t of every row
    counted = (got["live"] != 0) & (L.view(1, n) > 0) & (terminated.view(1, n) | (t.full_like(left, g) ** left <= float(tail_tol)))
    m = counted.double()
    bias = (qmin - G) * m
    sums = t.stack([m.sum(), bias.sum(), (bias * bias).sum(), (G * m).sum()]).cpu().numpy()      # the final statistics: the one transfer
    rows = int(sums[0])
    if rows == 0:
        raise ValueError(f"q_bias: no row counts -- no episode terminated and none is long enough for gamma^(L - t) <= {tail_tol} "
                         f"(gamma {g}, horizon {env.horizon}): use an eval env with a longer horizon")
    mean, g_mean = sums[1] / rows, sums[3] / rows
    std = float(np.sqrt(max(sums[2] / rows - mean * mean, 0.0)))
    scale = abs(g_mean)
    return {"mean": float(mean / scale) if scale > 0 else float("nan"), "std": std / scale if scale > 0 else float("nan"),
            "bias_mean": float(mean), "bias_std": std, "return_mean": float(g_mean), "rows": rows}


def greedy_returns(env, agent, episodes: int, seed: Optional[int] = None, one_launch: bool = False) -> Dict[str, Any]:
    """Greedy evaluation on `episodes` envs in lock-step: `env` (a NativeVecEnv or a HostVecEnv with num_envs == episodes) is reset
    (`seed`: its own if None) and stepped for one horizon with `agent.predict_device(explore=False)` (`agent.predict` on the host
    twin); `episode_stats()` is read once at the end -- on the GPU that is the evaluation's only host wait.  Every env finishes its
    FIRST episode inside that window (the time limit at the latest), and that one counts: one episode per env, whatever their lengths,
    which is the statistic `loop.episode` reports one env at a time.  An env that terminates early goes on with further episodes;
    they are not counted.
    `one_launch` (a NativeVecEnv only): the reset and the whole horizon are ONE kernel launch (include/sactd3_eval.h) instead of one loop
    body per step; the env's books are read the same way afterwards, so the keys and their meaning are the same.  The actions are the
    actor's greedy ones in another summation order: float32-close to the loop's, not its bits.
    -> {"return", "length": the means over the envs' first episodes (float64 of the fp32 figures, in env order), "episodes": how many,
    "returns", "lengths": per env, "bad_actions"}"""
    if int(episodes) != env.num_envs:
        raise ValueError(f"greedy_returns: the env has {env.num_envs} envs, {episodes} episodes were asked for")
    if one_launch:
        eng = _native_for_rollout(env, agent, "greedy_returns(one_launch=True)")
        if env.horizon > _lib.EVAL_MAX_STEPS:
            raise ValueError(f"greedy_returns(one_launch=True): the horizon ({env.horizon}) is above {_lib.EVAL_MAX_STEPS} steps")
        if seed is not None:
            env.seed = int(seed)
        eng.eval_rollout(env._h, {}, steps=env.horizon, reset=True, seed=env.seed & 0xFFFFFFFFFFFFFFFF, stream=env._stream())
    else:
        obs, _ = env.reset(seed=env.seed if seed is None else seed)
        for _ in range(env.horizon):
            obs = env.step(_greedy_actions(env, agent, obs))[0]
    st = env.episode_stats()
    if not (st["env_episodes"] >= 1).all():
        raise RuntimeError("greedy_returns: an env finished no episode within one horizon")      # (the time limit makes this impossible)
    return {"return": float(st["first_return"].astype(np.float64).mean()), "length": float(st["first_length"].astype(np.float64).mean()),
            "episodes": env.num_envs, "returns": st["first_return"], "lengths": st["first_length"], "bad_actions": st["bad_actions"]}


def device_episodes(env, agent, seed: int, one_launch: bool = False) -> Generator[Dict[str, np.ndarray], None, None]:
    """An episode generator with the yield of `loop.episode` ({"length", "return"} per `next()`), served by `greedy_returns`: one
    window of env.num_envs episodes per refill, re-seeded as `loop.episode` re-seeds.  Assign it to `loop.Evaluator.ep_gen` (sized
    num_envs == cfg.eval_steps: one window per evaluation) to evaluate without a host env step.  `one_launch`: as for greedy_returns."""
    if one_launch:
        _native_for_rollout(env, agent, "device_episodes(one_launch=True)")      # (refused here, not at the first next())
    rng = np.random.default_rng(seed)
    while True:
        got = greedy_returns(env, agent, env.num_envs, seed=seed + rng.integers(2 ** 32 - 1, size=1).item(), one_launch=one_launch)
        for k in range(env.num_envs):
            yield {"length": np.array(float(got["lengths"][k])), "return": np.array(float(got["returns"][k]))}
