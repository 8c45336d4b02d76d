"""The callers on either side of the update path, mirrored from the reference's orchestrator.py so that the engine can
be driven end to end without tensordict / torchrl / gymnasium being importable:

  Rollout / segment()   the acting side + its generator  orchestrator.py:42-118   
  DeviceRollout         the same acting side for a vector env that lives on the GPU: every array a device tensor, no host wait
  NativeRollout         ... for an env that emits ring records itself (envs.NativeVecEnv): choose / advance are one library call each
  train()       the training loop's control flow       orchestrator.py:317-352 (+ counters :326,342,349)
  update_plan() / rollout_for()   what train() decides ONCE before its loop: which update it issues (and every rule about the update
                keywords), which rollout drives the env -- both without touching an agent or a GPU
  load_dataset() / train_offline()   training on a FIXED dataset (not in the reference): the ring filled once, then runs of whole
                periods through Engine.run_iterations -- the workload of TD3+BC (hps.bc_alpha > 0)
  ProportionalSampler   proportional prioritised replay (not in the reference): a priority array on the device for train(sampler=...)
  episode()     evaluation-episode generator           orchestrator.py:121-246 (lengths / returns, trajectories with need_lists; no pixels)
  evaluate()    offline evaluation of a checkpoint     orchestrator.py:415-481 (trajectory files as .npz)
  Evaluator     the eval block of the loop             orchestrator.py:303-305,354-403 (rolling window, best model, speed)
  Tabular       key/value progress files               helpers/logger.py:93-150 (progress.json lines, progress.csv, text table)

`env` is anything with gymnasium's vector-env protocol as the reference uses it: `reset(seed=) -> (obs[n, o], info)`,
`step(actions[n, a]) -> (next_obs, rewards[n], terminations[n], truncations[n], infos)` with autoreset and
`infos["final_observation"][k]` holding the true last observation of an env that just ended, and
`action_space.sample() -> actions[n, a]`.  `SyntheticVecEnv` below is a dependency-free stand-in of that protocol
(the image has no gymnasium / MuJoCo); it is a test double, not a port of any environment.  `SyntheticDeviceVecEnv` is the same
env on torch tensors of one device, for `DeviceRollout`.
"""
from __future__ import annotations

import json
import time
from collections import deque
from pathlib import Path
from types import SimpleNamespace
from typing import Any, Callable, Dict, Generator, Optional, TextIO

import numpy as np


class Rollout:
    """The acting side of one learner: the current observations of the vector env, the action in force and the write path
    into the replay ring.  Two half-steps, because the reference chooses the next action BEFORE it hands control to the learner
    and steps the env only afterwards (orchestrator.py:62-78): `choose()` then `advance()`.

    Reference behaviour kept (orchestrator.py:42-118): one seeded reset, never again (:53); uniformly random actions while
    `agent.timesteps_so_far < learning_starts` (:64-65), the policy's exploring action afterwards; an action stays in force for
    `action_repeat` steps (:62); a truncated env stores its true final observation as the transition's next observation while
    the rollout continues from the auto-reset one, terminated envs keep the auto-reset one (:86-89); the stored `dones` ARE the
    terminations (:107-108); every stored field is float32 / bool with `[n, 1]` rewards and flags (:83,91-93,104-105).

    `overlap=True`: `choose()` only BEGINS the policy's action (`agent.predict_begin`) and `advance()` starts by collecting it
    (`agent.predict_end`), so whatever the caller issues in between -- the iteration's update -- runs while the action is being
    computed.  The order of the reference is kept: the action was begun before that update.  A repeated action and the random
    phase begin nothing.  Anything else that acts with the agent in between must call `resolve()` first."""

    def __init__(self, env, agent, seed: int, learning_starts: int, action_repeat: int, overlap: bool = False):
        assert agent.rb is not None
        if overlap:
            for name in ("predict_begin", "predict_end"):
                if not callable(getattr(agent, name, None)):
                    raise TypeError(f"overlap=True needs an agent with {name}(); {type(agent).__name__} has none")
        self.overlap, self.pending = overlap, False
        self.env, self.agent = env, agent
        self.learning_starts, self.action_repeat = learning_starts, action_repeat
        first, _ = env.reset(seed=seed)
        self.obs = np.asarray(first, np.float32)
        self.actions = None
        self.steps = 0

    def choose(self) -> None:
        if self.steps % self.action_repeat:
            return                                                   # the action in force is repeated
        if self.agent.timesteps_so_far < self.learning_starts:
            self.actions = self.env.action_space.sample()
        elif self.overlap:
            self.agent.predict_begin({"observations": self.obs}, explore=True)
            self.pending = True
        else:
            self.actions = self.agent.predict({"observations": self.obs}, explore=True)

    def resolve(self) -> None:
        """collect the action begun by `choose()`, if one is pending, and keep it for `advance()`"""
        if self.pending:
            self.actions = self.agent.predict_end()
            self.pending = False

    def advance(self) -> None:
        self.resolve()
        arrived, rewards, terminations, truncations, infos = self.env.step(self.actions)
        arrived = np.asarray(arrived, np.float32)
        stored_next = arrived
        cut = np.flatnonzero(np.asarray(truncations))
        if cut.size:                                                 # time-limit cuts: the episode's own last observation is stored
            stored_next = arrived.copy()
            for k in cut:
                stored_next[k] = np.asarray(infos["final_observation"][k], np.float32)
        ended = np.asarray(terminations, bool).reshape(-1, 1)
        self.agent.rb.extend({"observations": self.obs, "next_observations": stored_next,
                              "actions": np.asarray(self.actions, np.float32),
                              "rewards": np.asarray(rewards, np.float32).reshape(-1, 1),
                              "terminations": ended, "dones": ended})
        self.obs = arrived
        self.steps += 1


class DeviceRollout:
    """`Rollout` for a vector env that lives on the GPU: observations, actions, rewards and flags are tensors of the engine's device
    from `env.reset` to `rb.extend`, the action comes from `agent.predict_device`, and nothing in `choose()` / `advance()` copies to
    the host or waits for the device -- the env's kernels, the acting kernels and the ring append are ordered on the GPU
    (what the env does inside its own `step` / `action_space.sample()` is the env's business: see SyntheticDeviceVecEnv).
    Same two half-steps and the same reference behaviour as `Rollout` (orchestrator.py:42-118): one seeded reset; random actions
    while `agent.timesteps_so_far < learning_starts`, exploring actions afterwards; `action_repeat`; a truncated env stores its
    true final observation (a select over the truncation mask: `infos["final_observation"]` is an [n, o] tensor here); `dones`
    are the terminations; [n, 1] float32 / bool fields."""

    def __init__(self, env, agent, seed: int, learning_starts: int, action_repeat: int):
        assert agent.rb is not None
        if not callable(getattr(agent, "predict_device", None)):
            raise TypeError(f"a device env needs an agent with predict_device(); {type(agent).__name__} has none")
        import torch
        self._where = torch.where
        self.env, self.agent = env, agent
        self.learning_starts, self.action_repeat = learning_starts, action_repeat
        self.obs, _ = env.reset(seed=seed)
        self.actions = None
        self.steps = 0

    def choose(self) -> None:
        if self.steps % self.action_repeat:
            return
        if self.agent.timesteps_so_far < self.learning_starts:
            self.actions = self.env.action_space.sample()
        else:
            self.actions = self.agent.predict_device({"observations": self.obs}, explore=True)

    def resolve(self) -> None:
        """nothing is ever pending here (the protocol of `Rollout`, for `segment` / `train`)"""

    def advance(self) -> None:
        arrived, rewards, terminations, truncations, infos = self.env.step(self.actions)
        stored_next = self._where(truncations.reshape(-1, 1), infos["final_observation"], arrived)
        ended = terminations.reshape(-1, 1)
        self.agent.rb.extend({"observations": self.obs, "next_observations": stored_next, "actions": self.actions,
                              "rewards": rewards.reshape(-1, 1), "terminations": ended, "dones": ended})
        self.obs = arrived
        self.steps += 1


class NativeRollout:
    """`DeviceRollout` for an env that writes its transitions as ring records itself (`env.step_records`: envs.NativeVecEnv), through
    one handle of the library that knows the env and the engine (include/sactd3_rollout.h).  Three tensors -- `.obs` [n, o], `.actions`
    [n, a] and the record slab [n, record_floats] -- are allocated here, once; after that `choose()` and `advance()` are ONE ctypes
    call each and allocate nothing: the env's draw or the acting kernels write `.actions`, one launch of the env steps, writes the
    slab and overwrites `.obs`, one ingest launch appends the slab, all ordered on the GPU.  The kernels of the env run on the torch
    stream that is current at construction.  Same two half-steps and the same reference behaviour as `Rollout`
    (orchestrator.py:42-118); what stays in Python is what is host state: random or exploring actions by
    `agent.timesteps_so_far < learning_starts`, and `action_repeat`.  The ring, the env and the engine end bit for bit as
    `DeviceRollout` leaves them.  `.obs` and `.actions` are VIEWS of the bound buffers: the next call overwrites them."""

    def __init__(self, env, agent, seed: int, learning_starts: int, action_repeat: int):
        assert agent.rb is not None
        if not callable(getattr(env, "step_records", None)):
            raise TypeError(f"native_rollout=True needs an env with step_records(); {type(env).__name__} has none")
        import ctypes as C
        import torch
        from . import _lib
        eng = agent.engine
        self.env, self.agent = env, agent
        self.learning_starts, self.action_repeat = learning_starts, action_repeat
        dev = torch.device("cuda", int(eng.cfg.device_id))
        self.obs = torch.zeros((env.num_envs, eng.cfg.ob_dim), dtype=torch.float32, device=dev)
        self.actions = torch.zeros((env.num_envs, eng.cfg.ac_dim), dtype=torch.float32, device=dev)
        self.records = torch.zeros((env.num_envs, eng.rb_layout()["record_floats"]), dtype=torch.float32, device=dev)
        self._lib, self._error = eng.lib, _lib.EngineError
        buffers = _lib.CRolloutBuffers(self.obs.data_ptr(), self.obs.stride(0), self.actions.data_ptr(), self.actions.stride(0),
                                       self.records.data_ptr())
        self._h = C.c_void_p()
        stream = int(torch.cuda.current_stream(dev).cuda_stream)
        rc = self._lib.sactd3_rollout_create(eng._h, env._h, C.byref(buffers), C.c_void_p(stream or None), C.byref(self._h))
        if rc != 0:
            self._h = None
            raise self._error(f"sactd3_rollout_create failed ({rc}): {self._lib.sactd3_rollout_last_error(None).decode()}")
        self._choose, self._advance = self._lib.sactd3_rollout_choose, self._lib.sactd3_rollout_advance
        self._random, self._explore = _lib.ROLLOUT_RANDOM, _lib.ROLLOUT_EXPLORE
        self._slabs, self._max_steps = {}, _lib.COLLECT_MAX_STEPS     # collect(): steps -> (slab, eps or None), made at first use
        env.seed = int(seed)
        self._ck(self._lib.sactd3_rollout_reset(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF))
        self.steps = 0

    def _ck(self, rc: int) -> None:
        if rc != 0:
            raise self._error(f"native rollout call failed ({rc}): {self._lib.sactd3_rollout_last_error(self._h).decode()}")

    def close(self) -> None:
        """drop the handle (before the env or the engine is closed); the tensors stay the caller's"""
        if getattr(self, "_h", None):
            # (an engine closed first is gone: the handle's destroy would give it back the cycle graphs it no longer holds -- the few
            # bytes of the handle are left behind instead; the order the header asks for is rollout first)
            if getattr(self.agent.engine, "_h", None):
                self._lib.sactd3_rollout_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001 -- interpreter shutdown
            pass

    def stats(self) -> Dict[str, int]:
        """host counters of the handle (sactd3_rollout_stats)"""
        import ctypes as C
        out = (C.c_int64 * 4)()
        self._ck(self._lib.sactd3_rollout_stats(self._h, out))
        return dict(zip(("random_choices", "policy_choices", "steps", "rows_appended"), (int(v) for v in out)))

    def choose(self) -> None:
        if self.steps % self.action_repeat:
            return                                                   # the action in force is repeated
        rc = self._choose(self._h, self._random if self.agent.timesteps_so_far < self.learning_starts else self._explore)
        if rc:
            self._ck(rc)

    def resolve(self) -> None:
        """nothing is ever pending here (the protocol of `Rollout`, for `segment` / `train`)"""

    def advance(self) -> None:
        rc = self._advance(self._h)
        if rc:
            self._ck(rc)
        self.steps += 1

    def cycle(self, i: int) -> None:
        """`advance()`, `choose()` with the exploring policy and `agent.iteration(i)` as ONE ctypes call and one graph launch
        (include/sactd3_rollout_cycle.h: sactd3_rollout_cycle), with the counters the three keep: `steps`, the agent's
        `qnet_updates_so_far` / `actor_updates_so_far` (the actor updates run when i % (delay + 1) == 0); the batch generation is the
        engine's own.  Bit for bit the three calls.  For a body of the loop past `learning_starts` with `action_repeat` 1: the caller
        decides that (train(fused_rollout=True)); the engine refuses pinned rows, engine-owned priorities and an acting call in flight."""
        agent = self.agent
        delay = agent.engine.cfg.actor_update_delay
        do_actor = i % (delay + 1) == 0
        rc = self._lib.sactd3_rollout_cycle(self._h, self._explore, 1 if do_actor else 0)
        if rc:
            self._ck(rc)
        self.steps += 1
        agent.qnet_updates_so_far += 1
        if do_actor:
            agent.actor_updates_so_far += delay

    def collect(self, steps: int, mode: Optional[int] = None, eps: bool = False):
        """`steps` x (`choose()`, `advance()`) as ONE ctypes call and two launches (include/sactd3_rollout_collect.h:
        sactd3_rollout_collect): the collect kernel rolls all envs for `steps` steps under the current policy -- or, with the random
        phase's draw, bit for bit as the call sequence does -- and writes every transition as a ring record into a slab, time-major;
        the engine's own append takes the slab.  `mode` (None: random while `agent.timesteps_so_far < learning_starts`, else explore; or
        one of _lib.ROLLOUT_RANDOM / _EXPLORE / _EXPLOIT).  The slab [steps * n, record_floats] -- and with `eps=True` the draws
        [steps, n, a] -- are allocated once per `steps` and returned as VIEWS the next call of the same `steps` overwrites:
        -> records, or (records, eps).  For `action_repeat` 1 (the caller decides that: train(collected_rollout=True)).  ValueError for
        `steps` outside [1, 4096], before anything is allocated; the library's own refusals -- `steps * n` above the ring slots an append
        may use among them -- come as EngineError from the call."""
        steps = int(steps)
        if not 1 <= steps <= self._max_steps:
            raise ValueError(f"collect: steps must be in [1, {self._max_steps}], got {steps}")
        if mode is None:
            mode = self._random if self.agent.timesteps_so_far < self.learning_starts else self._explore
        slab = self._slabs.get(steps)
        if slab is None or (eps and slab[1] is None):
            import torch
            n, dev = self.env.num_envs, self.obs.device
            rec = slab[0] if slab is not None else torch.zeros((steps * n, self.records.shape[1]), dtype=torch.float32, device=dev)
            slab = self._slabs[steps] = (rec, torch.zeros((steps, n, self.actions.shape[1]), dtype=torch.float32, device=dev) if eps else None)
        rec, draws = slab
        rc = self._lib.sactd3_rollout_collect(self._h, int(mode), steps, rec.data_ptr(), draws.data_ptr() if eps else None)
        if rc:
            self._ck(rc)
        self.steps += steps
        return (rec, draws) if eps else rec

    def collect_stats(self) -> Dict[str, int]:
        """counters of the handle's collected segments (sactd3_rollout_collect_stats); `collect_ctr` is a device word: waits for the
        engine's stream"""
        import ctypes as C
        out = (C.c_int64 * 4)()
        self._ck(self._lib.sactd3_rollout_collect_stats(self._h, out))
        return dict(zip(("calls", "env_steps", "calls_that_drew", "collect_ctr"), (int(v) for v in out)))

    def cycle_stats(self) -> Dict[str, int]:
        """host counters of the handle's cycles (sactd3_rollout_cycle_stats), and `clamped`: appends that found a ring length or cursor
        outside the ring in device memory (sactd3_rollout_cycle_clamped: 0 in every sound run; waits for the engine's stream)"""
        import ctypes as C
        out, clamped = (C.c_int64 * 4)(), C.c_int64()
        self._ck(self._lib.sactd3_rollout_cycle_stats(self._h, out))
        self._ck(self._lib.sactd3_rollout_cycle_clamped(self._h, C.byref(clamped)))
        return dict(zip(("cycles", "graphs_captured", "graph_nodes", "eager_cycles"), (int(v) for v in out)), clamped=int(clamped.value))


def segment(env, agent, seed: int, segment_len: int, learning_starts: int, action_repeat: int, overlap: bool = False,
            rollout: Optional[Rollout] = None) -> Generator[None, None, None]:
    """orchestrator.py:42-118 as a generator over `Rollout`: control goes back to the caller every `segment_len` env steps, AFTER
    the next action has been chosen and BEFORE the env is stepped with it (:62-78) -- so the action that opens a segment was
    computed with the parameters of the previous one.  `overlap`: see Rollout (the action that opens a segment is then still being
    computed while the caller has control).  `rollout`: one the caller made itself, to `resolve()` it before it acts otherwise."""
    ro = rollout if rollout is not None else Rollout(env, agent, seed, learning_starts, action_repeat, overlap)
    while True:
        ro.choose()
        if ro.steps and ro.steps % segment_len == 0:
            yield
        ro.advance()


def collected_rollout_rules(*, overlap: bool, native_rollout: bool, fused_rollout: bool, action_repeat: int, segment_len: int) -> None:
    """What `collected_rollout=True` (a segment as one `NativeRollout.collect`) needs and excludes, looked at without an env: ValueError."""
    if not native_rollout:
        raise ValueError("collected_rollout=True needs native_rollout=True: the segment is a call of the native rollout's handle")
    if fused_rollout:
        raise ValueError("collected_rollout=True and fused_rollout=True exclude each other: a cycle is one env step, a collect a whole segment")
    if overlap:
        raise ValueError("collected_rollout=True and overlap=True exclude each other: the segment acts inside its own launch, on the learner stream")
    if int(action_repeat) != 1:
        raise ValueError("collected_rollout=True needs action_repeat == 1: the collect kernel chooses an action with every step")
    if int(segment_len) < 1:
        raise ValueError("collected_rollout=True needs segment_len >= 1")


def rollout_for(env, *, overlap: bool, device_env: bool, native_rollout: bool, fused_rollout: bool = False,
                collected_rollout: bool = False, action_repeat: int = 1, segment_len: int = 1):
    """Which of the three classes above drives `env` for train(): refuses what excludes each other, constructs nothing.  -> None for the
    plain host case (segment() makes its own `Rollout`), else what to call with (env, agent, seed, learning_starts, action_repeat).
    Both device rollouts act on the learner stream, so neither goes with `overlap`; the native one needs an env on the GPU that emits
    ring records (`step_records`: envs.NativeVecEnv).  `fused_rollout` (a loop body as one `NativeRollout.cycle`) needs the native
    rollout -- its two rules come first, before `env` is looked at; what it needs of the update keywords is `update_plan`'s.
    `collected_rollout` (a segment as one `NativeRollout.collect`) needs the native rollout and `action_repeat` 1, excludes
    `fused_rollout` and `overlap` and takes any `segment_len` >= 1 (`collected_rollout_rules`, in front of the env's as well)."""
    if collected_rollout:
        collected_rollout_rules(overlap=overlap, native_rollout=native_rollout, fused_rollout=fused_rollout, action_repeat=action_repeat,
                                segment_len=segment_len)
    if fused_rollout and not native_rollout:
        raise ValueError("fused_rollout=True needs native_rollout=True: the cycle is a call of the native rollout's handle")
    if fused_rollout and overlap:
        raise ValueError("fused_rollout=True and overlap=True exclude each other: the cycle acts inside its own graph, on the learner stream")
    if native_rollout and overlap:
        raise ValueError("native_rollout=True and overlap=True exclude each other: the native rollout acts on the learner stream")
    if native_rollout and not device_env:
        raise ValueError("native_rollout=True needs device_env=True: it drives an env that lives on the GPU")
    if native_rollout and not callable(getattr(env, "step_records", None)):
        raise TypeError(f"native_rollout=True needs an env with step_records(); {type(env).__name__} has none")
    if overlap and device_env:
        raise ValueError("overlap=True and device_env=True exclude each other: predict_device acts on the learner stream")
    if device_env:
        return NativeRollout if native_rollout else DeviceRollout
    return (lambda *to: Rollout(*to, overlap=True)) if overlap else None


class ProportionalSampler:
    """Proportional prioritised replay (Schaul et al. 2016) as a sampler the engine does not own: one float32 priority per ring slot in
    a torch tensor on `device`, nothing else -- no tree, no storage (the rows stay in the engine's ring).  Every method is torch ops on
    that device and never reads a device value on the host.
      extend(n)          the n rows the ring just received (its cursor is mirrored here, wrapping at `capacity`) enter at the current
                         maximum priority
      sample(B)          -> (index [B] int64, weights [B] float32): index ~ P(i) = p_i^alpha / sum_j p_j^alpha over the N rows held
                         (torch.multinomial, with replacement: N <= 2^24), weights = (N P(i))^-beta / the batch's largest
      update(index, td)  p_index = max over critics of |td| + eps, td = Agent.td_errors() ([2, B, 1]) of the update on those rows
    Meant for ReplayBuffer.sample_at(index, weights) -> Agent.update_qnets -> Agent.td_errors(): see train(sampler=...)."""

    def __init__(self, capacity: int, alpha: float = 0.6, beta: float = 0.4, eps: float = 1e-6, device: Any = None):
        import torch
        self._torch = torch
        self.capacity, self.alpha, self.beta, self.eps = int(capacity), float(alpha), float(beta), float(eps)
        self.priorities = torch.zeros(self.capacity, dtype=torch.float32, device=device)
        self.max_priority = torch.ones((), dtype=torch.float32, device=device)
        self.len, self.cursor = 0, 0                                  # host mirrors of the ring's length and write cursor

    def extend(self, n: int) -> None:
        torch = self._torch
        slots = (torch.arange(int(n), device=self.priorities.device) + self.cursor) % self.capacity
        self.priorities[slots] = self.max_priority
        self.cursor = (self.cursor + int(n)) % self.capacity
        self.len = min(self.capacity, self.len + int(n))

    def sample(self, batch_size: int):
        if self.len < 1:
            raise ValueError("ProportionalSampler.sample: no rows yet (extend() first)")
        torch = self._torch
        scaled = self.priorities[:self.len].pow(self.alpha)
        index = torch.multinomial(scaled, int(batch_size), replacement=True)
        weights = (scaled[index] * (self.len / scaled.sum())).pow(-self.beta)
        return index, weights / weights.max()

    def update(self, index, td) -> None:
        new = td.detach().abs().amax(dim=0).reshape(-1) + self.eps
        self.priorities[index] = new
        self.max_priority = self._torch.maximum(self.max_priority, new.max())


class PolicyStats:
    """`policy_stats=N` of train / train_offline: at every evaluation point N ring rows -- host-drawn slots from a generator of this
    object's own, read where they are (`rb.rows`) -- are put to the policy with their stored actions and a native sample
    (`agent.policy`).  -> vitals/replay_log_prob (mean log pi(a|s) of the stored actions: the behaviour-cloning diagnostic of a run on
    prior data), vitals/policy_entropy (mean -log pi of fresh samples) and vitals/log_std_mean.  SAC only: ValueError otherwise, at
    construction.  The query has a stream, a counter and a scratch of its own: the run's parameters, optimiser state, losses and
    counters are bit for bit those of the run without it."""
    KEYS = ("vitals/replay_log_prob", "vitals/policy_entropy", "vitals/log_std_mean")

    def __init__(self, agent, n: int, seed: int = 0):
        self.n = int(n)
        if self.n < 0:
            raise ValueError(f"policy_stats must be >= 0, got {n}")
        if self.n and bool(agent.engine.cfg.prefer_td3_over_sac):
            raise ValueError("policy_stats=... needs SAC: TD3's deterministic actor has no log-probability, entropy or log-std to report")
        self.agent, self.rng, self.last = agent, np.random.default_rng([int(seed), 0x706F6C]), {}

    def __call__(self, tabular: Optional["Tabular"] = None) -> Dict[str, float]:
        rows = len(self.agent.rb) if self.n else 0
        if rows == 0:
            return {}
        at = self.agent.rb.rows(self.rng.integers(0, rows, size=self.n, dtype=np.int64))
        got = self.agent.policy({"observations": at["observations"], "actions": at["actions"]}, sample=True)
        self.last = {"vitals/replay_log_prob": float(got["log_prob"].mean()), "vitals/policy_entropy": float(-got["sample_log_prob"].mean()),
                     "vitals/log_std_mean": float(got["log_std"].mean())}
        if tabular is not None:
            for k, v in self.last.items():
                tabular.record(k, v)
        return self.last


class QBias:
    """`q_bias=dict(env=, seed= [, gamma=, mode=, tail_tol=])` of train / train_offline: at every evaluation point `envs.q_bias` -- fresh
    on-policy episodes of `env` (an envs.NativeVecEnv of its own: never the training env, whose episodes it would cut) in one kernel
    launch, the critics' values of the recorded pairs against the Monte-Carlo returns.  -> vitals/q_bias_mean, vitals/q_bias_std (both
    divided by |mean return|: the REDQ definition) and vitals/q_bias_rows.  The rollout and the scoring have scratch and counters of their
    own: the run's parameters, optimiser state, losses and counters are bit for bit those of the run without it."""
    KEYS = ("vitals/q_bias_mean", "vitals/q_bias_std", "vitals/q_bias_rows")

    def __init__(self, agent, spec):
        from . import envs
        if not isinstance(spec, dict) or "env" not in spec or "seed" not in spec:
            raise ValueError("q_bias must be a dict with `env` (an evaluation envs.NativeVecEnv) and `seed`")
        unknown = set(spec) - {"env", "seed", "gamma", "mode", "tail_tol"}
        if unknown:
            raise ValueError(f"q_bias: unknown keys {sorted(unknown)}")
        envs._native_for_rollout(spec["env"], agent, "q_bias")             # (a host env, an agent without an engine: TypeError, before the run)
        self.agent, self.env, self.last = agent, spec["env"], {}
        self.kw = {k: v for k, v in spec.items() if k != "env"}
        self._q_bias = envs.q_bias

    def __call__(self, tabular: Optional["Tabular"] = None) -> Dict[str, float]:
        got = self._q_bias(self.env, self.agent, **self.kw)
        self.last = {"vitals/q_bias_mean": got["mean"], "vitals/q_bias_std": got["std"], "vitals/q_bias_rows": got["rows"]}
        if tabular is not None:
            for k, v in self.last.items():
                tabular.record(k, v)
        return self.last


class _Vitals:
    """the diagnostics of an evaluation point, in order, as one: what _eval_point calls and _last_metrics reads"""

    def __init__(self, parts):
        self.parts = parts

    def __call__(self, tabular: Optional["Tabular"] = None) -> Dict[str, float]:
        for part in self.parts:
            part(tabular)
        return self.last

    @property
    def last(self) -> Dict[str, float]:
        return {k: v for part in self.parts for k, v in part.last.items()}


def _vitals(agent, policy_stats: int, q_bias, cfg: Any):
    """PolicyStats and / or QBias as train / train_offline were asked for them; None: neither (and no call is made, no field of cfg read)"""
    parts = ([PolicyStats(agent, policy_stats, getattr(cfg, "seed", 0))] if policy_stats else []) + ([QBias(agent, q_bias)] if q_bias is not None else [])
    return None if not parts else parts[0] if len(parts) == 1 else _Vitals(parts)


RESET_ALL = ("actor", "critics", "alpha")      # the networks reset_networks / reset_every may name (a TD3 agent drops "alpha")


def update_plan(cfg: Any, *, fused: bool, sampler: Optional[ProportionalSampler], prioritized: Optional[Dict[str, float]], n_step: int,
                one_launch: bool, prior_fraction: Optional[float], updates_per_step: int,
                hindsight: Optional[Dict[str, Any]] = None, fused_rollout: bool = False,
                reset_every: Optional[int] = None, reset_what: Any = RESET_ALL, num_updates: Optional[int] = None) -> SimpleNamespace:
    """What train() does with one update, decided once from its keywords: touches no agent, env or GPU and imports nothing, so a process
    that never opens a GPU can ask whether a run would be refused.  `cfg` needs `batch_size` (with `prior_fraction`, and when an update is
    issued call by call), `num_envs` (with `n_step` > 1) and `actor_update_delay` (call by call).  Which keywords need or exclude each
    other is the table `refusals` below, one row per rule with its reason, the first row that applies raising ValueError: a new mode
    adds its rows there.  `prior_fraction` and `hindsight` count as reasons for `one_launch`.
    `reset_every` (None: never): the networks `reset_what` names (any of "actor", "critics", "alpha"; a sequence or one comma-separated
    string) start over, on the kept ring, whenever the update count reaches a multiple of it -- a call between two loop bodies, so it
    goes with every update form and every rollout.  `num_updates`: the length of a plan that is nothing but updates (train_offline); a
    `reset_every` above it would never be reached and is refused.
    `fused_rollout` (train's keyword: a loop body as one `NativeRollout.cycle`, whose update is the fused uniform iteration) needs
    `fused` and excludes every other draw; `cfg` then needs `segment_len` and `action_repeat`, which must both be 1.  Its rows stand first.
    -> a namespace of
      updates_per_step  as an int
      priorities        None, or dict(alpha=, eps=) for `agent.rb.enable_priorities` -- train() enables them once, before its loop
      hindsight         None, or the keywords of `agent.rb.configure_hindsight` (`hindsight` as given, `stride` defaulting to
                        cfg.num_envs) -- train() configures the buffer once, in the same place
      reset             None, or `reset(agent, before, first=None)`: to be called between two loop bodies with the update count the
                        previous call saw -- if the count has reached a further multiple of reset_every since then, `first()` and
                        `agent.reset_networks(reset_what)`, once; -> the count now
      update            `update(agent, i, tlog)`: iteration i, in ONE of three forms chosen here --
                          fused        agent.iteration(i)
                          one launch   agent.iteration(i, prior_rows=), agent.iteration(i, hindsight=True) or
                                       agent.iteration(i, beta=, n_step=, stride=), the values fixed here
                          call by call one draw (uniform `rb.sample`, `sampler` + `rb.sample_at`, `rb.sample_prioritized`, `rb.sample_mixed`,
                                       `rb.sample_hindsight`) ->
                                       update_qnets -> its write-back (`sampler.update` / `rb.update_priorities`) -> counters -> every
                                       delay + 1 iterations delay x update_actor -> update_targ_nets; losses go into `tlog`"""
    updates_per_step, n_step = int(updates_per_step), int(n_step)
    prior, prio, outside = prior_fraction is not None, prioritized is not None, sampler is not None
    unknown = sorted(set(prioritized or ()) - {"alpha", "beta", "eps"})
    hind = hindsight is not None
    hs_unknown = sorted(set(hindsight or ()) - {"achieved", "desired", "dim", "threshold", "ratio", "window", "stride"})
    hs_missing = sorted({"achieved", "desired", "dim", "threshold"} - set(hindsight or ())) if hind else []
    fr = bool(fused_rollout)
    rs = reset_every is not None
    rs_names = [w.strip() for w in reset_what.split(",")] if isinstance(reset_what, str) else list(reset_what)
    rs_unknown = sorted(set(rs_names) - set(RESET_ALL))
    refusals = (
        (rs and int(reset_every) < 1, f"reset_every must be >= 1, got {reset_every}"),
        (rs and bool(rs_unknown), f"reset_what: unknown networks {rs_unknown} (a choice of {list(RESET_ALL)})"),
        (rs and not rs_names, "reset_what names no network"),
        (rs and num_updates is not None and int(reset_every) > int(num_updates),
         f"reset_every={reset_every} is never reached by a plan of {num_updates} updates"),
        (fr and not fused, "fused_rollout=True needs fused=True: the update inside the cycle is the fused uniform iteration"),
        (fr and outside, "fused_rollout=True excludes sampler=...: the cycle draws uniformly inside its graph"),
        (fr and prio, "fused_rollout=True excludes prioritized=...: the cycle's append owes the priorities no launch, its draw is uniform"),
        (fr and n_step > 1, "fused_rollout=True excludes n_step > 1: the cycle's iteration samples single steps"),
        (fr and prior, "fused_rollout=True excludes prior_fraction=...: the cycle's append goes round the whole ring, pinned rows included"),
        (fr and hind, "fused_rollout=True excludes hindsight=...: the cycle's iteration relabels nothing"),
        (fr and one_launch, "fused_rollout=True excludes one_launch=True: that is the one-launch form of the other draws"),
        (fr and int(cfg.segment_len) != 1, "fused_rollout=True needs segment_len == 1: a cycle is one env step and one update"),
        (fr and int(cfg.action_repeat) != 1, "fused_rollout=True needs action_repeat == 1: a cycle chooses an action with every step"),
        (updates_per_step < 1, f"updates_per_step must be >= 1, got {updates_per_step}"),
        (prior and not 0.0 <= float(prior_fraction) <= 1.0, f"prior_fraction must be in [0, 1], got {prior_fraction}"),
        (prior and fused, "prior_fraction=... needs fused=False: the fused iteration samples uniformly inside its graph"),
        (prior and outside, "prior_fraction=... and sampler=... exclude each other: the mixed draw is the engine's own"),
        (prior and prio, "prior_fraction=... and prioritized=... exclude each other: a pinned ring has no priority table yet"),
        (prior and n_step > 1, "prior_fraction=... excludes n_step > 1: a pinned ring has no n-step chains yet"),
        (one_launch and fused, "one_launch=True needs fused=False: fused=True is the uniform 1-step iteration, already one launch"),
        (one_launch and outside, "one_launch=True excludes sampler=...: a sampler outside the engine cannot be part of its graph"),
        (one_launch and not (prio or n_step > 1 or prior or hind),
         "one_launch=True needs prioritized=... and / or n_step > 1: the uniform 1-step iteration is fused=True"),
        (not 1 <= n_step <= 16, f"n_step must be in [1, 16], got {n_step}"),
        (n_step > 1 and fused, "n_step=... needs fused=False: the fused iteration samples single steps uniformly inside its graph"),
        (outside and fused, "sampler=... needs fused=False: the fused iteration samples uniformly inside its graph"),
        (prio and fused, "prioritized=... needs fused=False: the fused iteration samples uniformly inside its graph"),
        (prio and outside, "prioritized=... and sampler=... exclude each other: one owner for the priorities"),
        (bool(unknown), f"prioritized: unknown keys {unknown}"),
        (hind and fused, "hindsight=... needs fused=False: the fused iteration samples uniformly inside its graph and relabels nothing"),
        (hind and outside, "hindsight=... and sampler=... exclude each other: the engine relabels the rows of its own draw"),
        (hind and prio, "hindsight=... and prioritized=... exclude each other: a relabelled row's TD error is not its record's priority"),
        (hind and n_step > 1, "hindsight=... excludes n_step > 1: a relabelled reward is a single step's, the chain's return is not"),
        (hind and prior, "hindsight=... and prior_fraction=... exclude each other: a pinned ring has no episode chains yet"),
        (bool(hs_unknown), f"hindsight: unknown keys {hs_unknown}"),
        (bool(hs_missing), f"hindsight: missing keys {hs_missing}"),
    )
    for applies, why in refusals:
        if applies:
            raise ValueError(why)
    prior_rows = int(round(float(prior_fraction) * int(cfg.batch_size))) if prior else None
    chain = dict(n_step=n_step, stride=int(cfg.num_envs)) if n_step > 1 else {}
    beta = float(prioritized.get("beta", 0.4)) if prio else None
    priorities = dict(alpha=float(prioritized.get("alpha", 0.6)), eps=float(prioritized.get("eps", 1e-6))) if prio else None
    hs_config = dict(hindsight, stride=int(hindsight["stride"]) if hindsight.get("stride") is not None else int(cfg.num_envs)) if hind else None
    if fused:
        update = lambda agent, i, tlog: agent.iteration(i)
    elif one_launch and prior:                                           # (a keyword the older signature lacks: only when used)
        update = lambda agent, i, tlog: agent.iteration(i, prior_rows=prior_rows)
    elif one_launch and hind:                                            # (the same: a keyword only when used)
        update = lambda agent, i, tlog: agent.iteration(i, hindsight=True)
    elif one_launch:
        stride = chain.get("stride")
        update = lambda agent, i, tlog: agent.iteration(i, beta=beta, n_step=n_step, stride=stride)
    else:
        write_back = lambda agent, index: None                           # the uniform and the mixed draw keep no priorities
        if prior:
            draw = lambda agent: (agent.rb.sample_mixed(cfg.batch_size, prior_rows), None)
        elif prio:
            draw = lambda agent: (agent.rb.sample_prioritized(cfg.batch_size, beta, **chain), None)
            write_back = lambda agent, index: agent.rb.update_priorities()
        elif hind:
            draw = lambda agent: (agent.rb.sample_hindsight(cfg.batch_size), None)
        elif not outside:
            draw = lambda agent: (agent.rb.sample(cfg.batch_size, **chain), None)
        else:
            def draw(agent):
                index, weights = sampler.sample(cfg.batch_size)
                return agent.rb.sample_at(index, weights, **chain), index
            write_back = lambda agent, index: sampler.update(index, agent.td_errors())

        def update(agent, i, tlog):
            batch, index = draw(agent)
            tlog.update(agent.update_qnets(batch))
            write_back(agent, index)
            agent.qnet_updates_so_far += 1
            if i % (cfg.actor_update_delay + 1) == 0:
                for _ in range(cfg.actor_update_delay):
                    tlog.update(agent.update_actor(batch))
                    agent.actor_updates_so_far += 1
            agent.update_targ_nets()
    reset = None
    if rs:
        every, names = int(reset_every), tuple(rs_names)

        def reset(agent, before, first=None):
            now = int(agent.qnet_updates_so_far)
            if now // every > before // every:
                if first is not None:
                    first()
                agent.reset_networks(names)
            return now
    return SimpleNamespace(updates_per_step=updates_per_step, priorities=priorities, hindsight=hs_config, update=update, reset=reset)


def _eval_point(agent, pstats: Optional[Any], evaluator: Optional["Evaluator"], on_eval, count: int, resets: bool = False) -> None:
    """the evaluation point of train / train_offline: policy stats, then the evaluator, then on_eval(agent, count); resets: the run
    resets its networks, and vitals/resets goes into the evaluator's table with them"""
    if pstats is not None:
        pstats(getattr(evaluator, "tabular", None))
    if resets and getattr(evaluator, "tabular", None) is not None:
        evaluator.tabular.record("vitals/resets", int(agent.resets_so_far))
    if evaluator is not None:
        evaluator(agent)
    if on_eval is not None:
        on_eval(agent, count)


def _last_metrics(agent, pstats: Optional[Any], resets: bool = False) -> Dict[str, float]:
    out = dict(agent.engine.read_metrics(), **(pstats.last if pstats is not None else {}))
    if resets:
        out["vitals/resets"] = int(agent.resets_so_far)
    return out


def train(cfg: Any, env, agent, *, fused: bool = True, on_eval: Optional[Callable[[Any, int], None]] = None,
          evaluator: Optional["Evaluator"] = None, overlap: bool = False, device_env: bool = False,
          sampler: Optional[ProportionalSampler] = None, prioritized: Optional[Dict[str, float]] = None,
          n_step: int = 1, one_launch: bool = False, prior_fraction: Optional[float] = None,
          updates_per_step: int = 1, policy_stats: int = 0, native_rollout: bool = False,
          hindsight: Optional[Dict[str, Any]] = None, fused_rollout: bool = False,
          reset_every: Optional[int] = None, reset_what: Any = RESET_ALL, q_bias: Optional[Dict[str, Any]] = None,
          collected_rollout: bool = False) -> Dict[str, float]:
    """Control flow of orchestrator.py:317-352 (no wandb / tqdm / checkpoint upload): interact, count, wait for
    `learning_starts`, then per iteration sample -> critic update -> (every delay+1 iterations) delay x actor
    update -> target update, with the reference's counters.  `fused=True` issues the whole iteration as one graph
    launch (Agent.iteration); `fused=False` makes the reference's individual calls.  Every `eval_every` timesteps
    `evaluator` (the reference's eval block, :354-403) and/or `on_eval` run.  Returns the last metrics.
    Which of the update keywords need or exclude each other is stated once, at `update_plan`; which rollout keywords do, at
    `rollout_for`.  Both are asked before anything else happens: a call that either refuses has not touched the agent -- in
    particular it has not enabled priorities in the engine, as a call refused for its rollout keywords once had.
    `overlap=True` (an agent with predict_begin / predict_end): the action that opens the next segment is computed on the engine's
    acting stream while this iteration's update runs; a pending action is collected before an evaluation acts with the agent.
    `device_env=True`: `env` lives on the GPU (device tensors in and out, e.g. SyntheticDeviceVecEnv) and is driven by `DeviceRollout`
    -- `agent.predict_device`, no host round trip per env step.
    `native_rollout=True` (an env with `step_records`, e.g. envs.NativeVecEnv): the env is driven by `NativeRollout` instead -- the env
    step writes the transitions as ring records and choose / advance are one library call each, with the ring, the env and the engine
    bit for bit as `DeviceRollout` leaves them.  Off by default.
    `fused_rollout=True` (needs native_rollout=True and fused=True, segment_len == 1 and action_repeat == 1; excludes every other draw):
    a loop body -- env step, ring append, next action, update -- is ONE library call and one graph launch (`NativeRollout.cycle`)
    wherever the step count in front of it is at or past `learning_starts`, so that its choice is an exploring one and an update
    follows; every other body -- the random phase, the step that crosses `learning_starts` -- goes through the call sequence, and
    with `updates_per_step` > 1 the further updates do.  The run ends bit for bit as the native_rollout=True run does.  Off by default.
    `collected_rollout=True` (needs native_rollout=True and action_repeat == 1; excludes fused_rollout and overlap; any segment_len >= 1):
    a segment -- segment_len steps of all envs, their actions, their ring records, the append -- is ONE library call and two launches
    (`NativeRollout.collect`) in place of segment_len choose / advance pairs; everything behind it in a loop body is unchanged, so every
    update form, `updates_per_step`, resets and the vitals work with it, pinned rows and engine-owned priorities included (the append
    is the engine's own).  One semantic difference: the action that opens a segment is chosen AFTER the update in front of it, with
    that update's parameters, not before it (`segment()` chooses, then yields) -- and a policy action comes from the collect kernel,
    which sums in another order than `predict`, with draws of a stream of its own.  So the run is not bit for bit the
    native_rollout=True run; its random phase is.  A segment must fit the ring slots an append may use (segment_len * num_envs <=
    rb_capacity minus the pinned rows): that is the engine's to know and is refused by the first `collect`, as an EngineError, not here.
    Off by default.
    `sampler` (a ProportionalSampler): prioritised replay, call by call on the device -- the sampler's rows and importance weights
    through `rb.sample_at`, the critic update weighted by them, its TD errors (`agent.td_errors`) back into the sampler's priorities;
    the actor updates train on the same rows, unweighted.
    `prioritized` (dict(alpha=, beta=, eps=), any subset): the same iteration with the priorities kept by the ENGINE --
    `rb.sample_prioritized` -> weighted critic update -> `rb.update_priorities()` -- with no torch arithmetic in between and nothing to
    mirror on the host: the engine sees its own appends.
    `n_step` (1 to 16): the critic trains on n-step returns chained by the engine out of consecutive ring rows of one env
    (`stride=cfg.num_envs`), cut at episode ends -- with the uniform, the `sampler` and the `prioritized` draw alike.
    `one_launch=True`: the `prioritized` / `n_step` / `prior_fraction` / `hindsight` iteration is issued as one graph launch --
    `agent.iteration(i, beta=, n_step=, stride=cfg.num_envs)`, `agent.iteration(i, prior_rows=)` or
    `agent.iteration(i, hindsight=True)` -- in place of the call sequence,
    with the same results bit for bit and the same counters.
    `prior_fraction` (in [0, 1]): learning online from prior data -- every batch takes round(prior_fraction * batch_size) rows from
    the rows `agent.rb.pin()` protects (`load_dataset(..., pin=True)`) and the others from the rows the run appends (`rb.sample_mixed`).
    `hindsight` (dict(achieved=, desired=, dim=, threshold= [, ratio=, window=, stride=]): the keywords of `rb.configure_hindsight`,
    `stride` defaulting to cfg.num_envs): a goal-conditioned task with a sparse reward -- every batch is drawn as `rb.sample` draws it
    and a `ratio` share of its rows is relabelled by the engine while it is staged, with a goal the row's own episode reached later
    (`rb.sample_hindsight`; fused=False: call by call, or with one_launch=True as one graph launch).  `envs.NativeVecEnv.goal_layout` gives the first four keys for a native task.
    `updates_per_step` (>= 1, every mode): the update-to-data ratio -- after each segment the update runs that many times, `i` and the
    update counters advancing per update; 1 is the reference's loop.
    `policy_stats=N` (default 0: off, and no call is made; SAC only): at every evaluation point N ring rows are put to the policy
    (PolicyStats) and vitals/replay_log_prob, vitals/policy_entropy and vitals/log_std_mean are recorded with the evaluator's table
    and returned with the last metrics; the run itself is bit for bit the run without it.
    `reset_every=N` (default None: never; `reset_what`: any of "actor", "critics", "alpha", default all): the periodic reset of high
    update-to-data training -- whenever `agent.qnet_updates_so_far` reaches a multiple of N, `agent.reset_networks(reset_what)` is
    issued between two loop bodies (behind the body's evaluation point): fresh networks from the engine's own initialiser, the replay
    ring kept.  One call on the engine's stream in every update form and every rollout, fused_rollout=True included: no graph is
    dropped.  vitals/resets (`agent.resets_so_far`) is recorded with the evaluator's table and returned with the last metrics.
    `q_bias=dict(env=, seed=)` (default None: off, and no call is made): at every evaluation point the normalised Q-bias of the current
    policy on fresh episodes of `env` (QBias; an envs.NativeVecEnv of its own) -- vitals/q_bias_mean, vitals/q_bias_std and
    vitals/q_bias_rows, recorded and returned like the policy stats; the run itself is bit for bit the run without it."""
    pstats = _vitals(agent, policy_stats, q_bias, cfg)
    plan = update_plan(cfg, fused=fused, sampler=sampler, prioritized=prioritized, n_step=n_step, one_launch=one_launch,
                       prior_fraction=prior_fraction, updates_per_step=updates_per_step, hindsight=hindsight, fused_rollout=fused_rollout,
                       reset_every=reset_every, reset_what=reset_what)
    resets = plan.reset is not None
    make_rollout = rollout_for(env, overlap=overlap, device_env=device_env, native_rollout=native_rollout, fused_rollout=fused_rollout,
                               **(dict(collected_rollout=True, action_repeat=cfg.action_repeat, segment_len=cfg.segment_len)
                                  if collected_rollout else {}))
    if plan.priorities is not None:                                       # (nothing above touched the agent's engine)
        agent.rb.enable_priorities(**plan.priorities)
    if plan.hindsight is not None:
        agent.rb.configure_hindsight(**plan.hindsight)
    ro = make_rollout(env, agent, cfg.seed, cfg.learning_starts, cfg.action_repeat) if make_rollout is not None else None
    resolve = ro.resolve if ro is not None else (lambda: None)            # (segment()'s own host rollout never has an action pending)
    seg_gen = segment(env, agent, cfg.seed, cfg.segment_len, cfg.learning_starts, cfg.action_repeat, rollout=ro)
    i = 0
    tlog: Dict[str, Any] = {}
    step_rows = cfg.segment_len * cfg.num_envs
    seen = int(agent.qnet_updates_so_far) if resets else 0               # the update count the reset rule last looked at
    try:
        while agent.timesteps_so_far <= cfg.num_timesteps:
            if evaluator is not None:
                evaluator.maybe_start_clock(agent.timesteps_so_far)       # orchestrator.py:319-322
            # a body past learning_starts chooses by the policy and is followed by an update: advance, choose and that update as one
            # call.  (ro.steps > 0: the generator has made the choice that opens the rollout, and waits between a choose and an advance.)
            cycled = fused_rollout and ro.steps > 0 and agent.timesteps_so_far >= cfg.learning_starts
            if cycled:
                ro.cycle(i)
                i += 1
            elif collected_rollout:
                ro.collect(cfg.segment_len)
            else:
                next(seg_gen)
            agent.timesteps_so_far += step_rows
            if sampler is not None:
                sampler.extend(step_rows)                                 # the rows the segment just appended
            if agent.timesteps_so_far <= cfg.learning_starts:
                i += 1
                continue
            for _ in range(plan.updates_per_step - (1 if cycled else 0)):   # (1: the reference's one update per segment)
                plan.update(agent, i, tlog)
                i += 1
            if agent.timesteps_so_far % cfg.eval_every == 0:
                resolve()                                                 # the evaluator / on_eval act (or load) with the same agent
                _eval_point(agent, pstats, evaluator, on_eval, agent.timesteps_so_far, resets)
            if resets:                                                    # between two bodies, whatever form they take; resolve: the
                seen = plan.reset(agent, seen, resolve)                   # engine refuses a reset under an acting call in flight
    finally:
        if fused_rollout and ro is not None:
            ro.close()                                                    # the engine holds graphs of this binding: dropped with it, here
    resolve()                                                             # leave no acting call in flight behind the loop
    return _last_metrics(agent, pstats, resets)


_DATASET_KEYS = ("observations", "actions", "rewards", "next_observations", "terminations")


def load_dataset(agent, data, chunk: int = 65536, pin: bool = False) -> int:
    """Append a whole offline dataset to the agent's replay ring, `chunk` rows per `rb.extend` call, in order.  `data`: a mapping with
    the keys of `rb.extend` -- observations [n, o], actions [n, a], rewards [n] or [n, 1], next_observations [n, o], terminations [n]
    or [n, 1], optionally dones (default: terminations) -- whose values are numpy arrays or CUDA tensors (device tensors are appended
    where they are, without a host round trip).  Raises ValueError if the rows do not fit into what is left of the ring's capacity:
    the ring would wrap and silently drop the oldest rows.  Normalising the states (as the TD3+BC paper does) is the caller's
    business, before this call: the engine trains on the rows it is given.  `pin=True`: the rows the ring then holds are pinned
    (`agent.rb.pin()`) -- an online run on top appends behind them and never evicts them (train(prior_fraction=...)).  Returns the
    number of rows appended."""
    missing = [k for k in _DATASET_KEYS if k not in data]
    if missing:
        raise ValueError(f"load_dataset: missing key(s) {missing}")
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"load_dataset: chunk must be >= 1, got {chunk}")
    cols = {k: data[k] for k in _DATASET_KEYS}
    cols["dones"] = data["dones"] if "dones" in data else data["terminations"]
    rows = {k: int(v.shape[0]) for k, v in cols.items()}
    n = rows["observations"]
    if len(set(rows.values())) != 1:
        raise ValueError(f"load_dataset: the fields disagree on the number of rows: {rows}")
    room = int(agent.rb.capacity) - len(agent.rb)
    if n > room:
        raise ValueError(f"load_dataset: {n} rows do not fit into the replay ring ({room} of {int(agent.rb.capacity)} rows free): "
                         "it would wrap and drop data; build the agent with a larger rb_capacity")
    for lo in range(0, n, chunk):
        agent.rb.extend({k: v[lo:lo + chunk] for k, v in cols.items()})
    if pin:
        agent.rb.pin()
    return n


def train_offline(cfg: Any, agent, *, num_updates: int, evaluator: Optional["Evaluator"] = None,
                  on_eval: Optional[Callable[[Any, int], None]] = None, eval_every_updates: Optional[int] = None,
                  policy_stats: int = 0, reset_every: Optional[int] = None, reset_what: Any = RESET_ALL,
                  q_bias: Optional[Dict[str, Any]] = None) -> Dict[str, float]:
    """`num_updates` iterations of orchestrator.py:337-352 on the ring as it stands (load_dataset), with no environment step in
    between: the iterations go out through `agent.engine.run_iterations` -- whole periods of the actor schedule as one graph launch,
    runs of periods as one launch where the engine has them -- in runs that end where an evaluation is due (every
    `eval_every_updates` iterations; None: none before the end) and at `num_updates`.  `evaluator` and / or `on_eval(agent, updates
    done)` run at those points.  Keeps `qnet_updates_so_far` and `actor_updates_so_far` as Agent.iteration does and leaves
    `timesteps_so_far` alone (no env step was taken).  With plain TD3 or SAC this diverges on most datasets -- the actor climbs Q where
    no data constrains it; TD3+BC (`hps.bc_alpha` > 0, e.g. 2.5) is the algorithm it is meant for.  `policy_stats=N` as for train (SAC
    only), `q_bias=dict(env=, seed=)` as for train.  `reset_every` / `reset_what` as for train: the runs also end where a reset is due, and a `reset_every` above `num_updates`
    is refused (update_plan's table).  Returns the last metrics."""
    num_updates = int(num_updates)
    if num_updates < 0:
        raise ValueError(f"train_offline: num_updates must be >= 0, got {num_updates}")
    reset = None
    if reset_every is not None:                                           # (before the agent is touched)
        reset = update_plan(cfg, fused=True, sampler=None, prioritized=None, n_step=1, one_launch=False, prior_fraction=None,
                            updates_per_step=1, reset_every=reset_every, reset_what=reset_what, num_updates=num_updates).reset
    pstats = _vitals(agent, policy_stats, q_bias, cfg)
    every = num_updates if eval_every_updates is None else int(eval_every_updates)
    if eval_every_updates is not None and every < 1:
        raise ValueError(f"train_offline: eval_every_updates must be >= 1, got {eval_every_updates}")
    eng = agent.engine
    period, delay = int(eng.cfg.actor_update_delay) + 1, int(eng.cfg.actor_update_delay)
    i = 0
    seen = int(agent.qnet_updates_so_far) if reset is not None else 0      # the update count the reset rule last looked at
    while i < num_updates:
        end = min(num_updates, (i // every + 1) * every) if every > 0 else num_updates
        if reset is not None:                                             # ... and where the update count reaches a multiple of reset_every
            end = min(end, i + int(reset_every) - seen % int(reset_every))
        eng.run_iterations(i, end - i)
        agent.qnet_updates_so_far += end - i
        agent.actor_updates_so_far += delay * len(range(-(-i // period) * period, end, period))      # the iterations with i % period == 0
        i = end
        if i % every == 0 or i == num_updates:
            _eval_point(agent, pstats, evaluator, on_eval, i, reset is not None)
        if reset is not None:
            seen = reset(agent, seen)
    return _last_metrics(agent, pstats, reset is not None)


class Tabular:
    """Key/value progress writer with the file formats of the reference's logger (helpers/logger.py:93-150):
    `progress.json` holds one JSON object per dump, `progress.csv` one row per dump under a header that grows when a
    new key appears (earlier rows are padded), and an optional text stream gets a boxed two-column table."""

    def __init__(self, directory: Optional[Path] = None, stream: Optional[TextIO] = None, suffix: str = ""):
        self._kv: Dict[str, Any] = {}
        self._keys: list = []
        self._rows: list = []
        self._stream = stream
        self._json = self._csv = None
        if directory is not None:
            directory = Path(directory)
            directory.mkdir(parents=True, exist_ok=True)
            self._json = (directory / f"progress{suffix}.json").open("wt")
            self._csv = directory / f"progress{suffix}.csv"

    def record(self, key: str, val: Any) -> None:
        self._kv[key] = val.item() if isinstance(val, np.ndarray) and val.ndim == 0 else (float(val) if isinstance(val, np.floating) else val)

    def dump(self) -> Dict[str, Any]:
        kv, self._kv = self._kv, {}
        if not kv:
            return kv
        if self._json is not None:
            self._json.write(json.dumps(kv) + "\n")
            self._json.flush()
        if self._csv is not None:
            self._keys += [k for k in kv if k not in self._keys]
            self._rows.append(kv)
            with self._csv.open("wt") as f:            # a new column rewrites the (small) file, as the reference's writer does
                f.write(",".join(self._keys) + "\n")
                for row in self._rows:
                    f.write(",".join("" if row.get(k) is None else str(row[k]) for k in self._keys) + "\n")
        if self._stream is not None:
            cells = {k[:40]: (f"{v:<8.3g}" if isinstance(v, float) else str(v))[:40] for k, v in kv.items()}
            kw, vw = max(map(len, cells)), max(map(len, cells.values()))
            bar = "-" * (kw + vw + 7)
            self._stream.write("\n".join([bar] + [f"| {k.ljust(kw)} | {v.ljust(vw)} |" for k, v in cells.items()] + [bar]) + "\n")
            self._stream.flush()
        return kv

    def close(self) -> None:
        if self._json is not None:
            self._json.close()


class Evaluator:
    """The evaluation block of the training loop (orchestrator.py:354-403): every call plays `eval_steps` greedy
    episodes, reports the mean length / return over a rolling window of the last 20 x eval_steps episodes (:303-305,
    :364-367), saves the model as `ckpt_best` when the windowed return improves (:376-380) and computes the training speed
    in env steps per second with evaluation time excluded and a burn-in before the clock starts (:319-322,:392-397)."""

    def __init__(self, cfg: Any, eval_env, agent, tabular: Optional[Tabular] = None, ckpt_dir: Optional[Path] = None,
                 clock: Callable[[], float] = time.time):
        self.cfg, self.tabular, self.ckpt_dir, self._clock = cfg, tabular, ckpt_dir, clock
        self.ep_gen = episode(eval_env, agent, cfg.seed)
        window = 20 * cfg.eval_steps
        self.len_buff, self.ret_buff = deque(maxlen=window), deque(maxlen=window)
        self.start_time: Optional[float] = None
        self.burnin_ts: Optional[int] = None
        self.time_spent_eval = 0.0
        self.history: list = []

    def maybe_start_clock(self, timesteps_so_far: int) -> None:
        burn = getattr(self.cfg, "measure_burnin", 0)
        if self.start_time is None and timesteps_so_far >= burn + self.cfg.learning_starts:
            self.start_time, self.burnin_ts = self._clock(), timesteps_so_far

    def __call__(self, agent) -> Dict[str, float]:
        t0 = self._clock()
        for _ in range(self.cfg.eval_steps):
            ep = next(self.ep_gen)
            self.len_buff.append(float(ep["length"]))
            self.ret_buff.append(float(ep["return"]))
        out = {"timestep": int(agent.timesteps_so_far), "length": float(np.mean(np.asarray(self.len_buff, np.float32))),
               "return": float(np.mean(np.asarray(self.ret_buff, np.float32)))}
        if self.tabular is not None:
            for k, v in out.items():
                self.tabular.record(k, v)
        if out["return"] > agent.best_eval_ep_ret:
            agent.best_eval_ep_ret = out["return"]
            if self.ckpt_dir is not None:
                Path(self.ckpt_dir).mkdir(parents=True, exist_ok=True)
                agent.save(self.ckpt_dir, sfx="best")
            out["new_best"] = True
        out["replay_buffer_numel"] = len(agent.rb) if getattr(agent, "rb", None) is not None else 0
        self.time_spent_eval += self._clock() - t0
        if self.start_time is not None:
            train_time = self._clock() - self.start_time - self.time_spent_eval
            out["speed"] = (agent.timesteps_so_far - self.burnin_ts) / max(train_time, 1e-9)
            if self.tabular is not None:
                self.tabular.record("speed", out["speed"])
        if self.tabular is not None:
            self.tabular.dump()
        self.history.append(out)
        return out


class _Trajectory:
    """The per-step record of one evaluation episode (`need_lists=True`, orchestrator.py:143-148,179-195).  Columns are
    plain Python lists while the episode runs and become numpy arrays when it ends (the reference's reason: list.append is
    cheap).  Layout quirks kept on purpose: every entry keeps the vector-env's leading axis of size 1; `observations` is
    the reset observation followed by every non-final `new_ob`, `next_observations` every `new_ob` -- so the last one is
    the auto-reset observation of the NEXT episode, not the final observation of this one."""

    KEYS = ("observations", "actions", "next_observations", "rewards", "terminations", "dones")

    def __init__(self):
        self.cols: Dict[str, list] = {k: [] for k in self.KEYS}

    def begin(self, ob) -> None:
        self.cols = {k: [] for k in self.KEYS}
        self.cols["observations"].append(ob)

    def step(self, action, new_ob, reward, termination, done) -> None:
        c = self.cols
        c["next_observations"].append(new_ob)
        c["actions"].append(action)
        c["rewards"].append(reward)
        c["terminations"].append(termination)
        c["dones"].append(done)
        if not done:
            c["observations"].append(new_ob)

    def arrays(self) -> Dict[str, np.ndarray]:
        return {k: np.array(v) for k, v in self.cols.items()}


def episode(env, agent, seed: int, *, need_lists: bool = False) -> Generator[Dict[str, np.ndarray], None, None]:
    """orchestrator.py:121-246 without pixels: one evaluation episode per `next()` on a ONE-env vector env, greedy actions
    (`explore=False`, :165-173), episode statistics taken from `infos["final_info"]` (:197-201), the env re-seeded before
    every episode from a generator seeded with `seed` (:136-140,152,238).  `need_lists=True` adds the trajectory (see
    _Trajectory) to the yielded dict, as `evaluate()` consumes it (:446-457)."""
    rng = np.random.default_rng(seed)

    def fresh_episode():
        ob, _ = env.reset(seed=seed + rng.integers(2 ** 32 - 1, size=1).item())
        return ob

    traj = _Trajectory() if need_lists else None
    ob = fresh_episode()
    if traj:
        traj.begin(ob)
    while True:
        action = agent.predict({"observations": np.asarray(ob, np.float32)}, explore=False)
        new_ob, reward, termination, truncation, infos = env.step(action)
        done = bool(np.asarray(termination).any() or np.asarray(truncation).any())
        if traj:
            traj.step(action, new_ob, reward, termination, np.asarray(done) if np.ndim(termination) == 0 else np.asarray(termination) | np.asarray(truncation), )
        ob = new_ob
        if "final_info" in infos:
            stats = [i["episode"] for i in infos["final_info"] if i is not None][-1]
            out = traj.arrays() if traj else {}
            out["length"] = np.array(float(np.asarray(stats["l"]).item()))
            out["return"] = np.array(float(np.asarray(stats["r"]).item()))
            yield out
            ob = fresh_episode()
            if traj:
                traj.begin(ob)


def evaluate(cfg: Any, env, agent, name: str = "eval", tabular: Optional[Tabular] = None) -> Dict[str, float]:
    """orchestrator.py:415-481 without wandb / pixels: optionally restore a checkpoint (`cfg.load_ckpt`: a local .pth path
    for `agent.load_from_disk`; the reference downloads it from wandb, :430), play `cfg.num_episodes` greedy episodes, and
    with `cfg.gather_trajectories` write each one under `cfg.trajectory_dir / name` as `{i:03d}_L{length}_R{return}.npz`
    (the reference writes the same arrays with TensorDict.to_h5, :446-457; h5py / tensordict are not in this image) after
    checking that every column has `length` rows (:450-451) and casting float64 columns to float32 (:454-456).  Returns the
    mean length / return (:473-476, float32 means) and records them in `tabular` (:478-481)."""
    traj_dir = None
    if getattr(cfg, "gather_trajectories", False):
        traj_dir = Path(cfg.trajectory_dir) / name
        traj_dir.mkdir(parents=True, exist_ok=True)
    ckpt = getattr(cfg, "load_ckpt", None)
    if ckpt:
        agent.load_from_disk(Path(ckpt))
    ep_gen = episode(env, agent, cfg.seed, need_lists=traj_dir is not None)
    lens, rets = [], []
    for i in range(cfg.num_episodes):
        ep = next(ep_gen)
        lens.append(ep["length"])
        rets.append(ep["return"])
        if traj_dir is not None:
            n = int(ep["length"])
            cols = {k: v for k, v in ep.items() if k not in ("length", "return")}
            for k, v in cols.items():
                assert v.shape[0] == n, f"wrong array length for {k=}"
            cols = {k: (v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in cols.items()}
            np.savez(traj_dir / f"{str(i).zfill(3)}_L{n}_R{int(ep['return'])}.npz", length=ep["length"], **{"return": ep["return"]}, **cols)
    out = {"length": float(np.asarray(lens, np.float32).mean()), "return": float(np.asarray(rets, np.float32).mean())}
    if tabular is not None:
        for k, v in out.items():
            tabular.record(k, v)
        tabular.dump()
    return out


def _fold_sum(x):
    """The sum over axis 1 of a numpy array or torch tensor `x` (which it overwrites) in ONE fixed order, by element-wise additions
    only: the upper half is folded onto the lower until one column is left.  A library reduction or matrix product adds in an order
    of its own choice; this one gives the same bits in numpy, in torch on the host and in torch on the GPU."""
    k = x.shape[1]
    while k > 1:
        h = k // 2
        x[:, :h] += x[:, k - h:k]
        k -= h
    return x[:, 0]


def _dynamics(s, actions, A, Bm, noise):
    """s' = s A + a B + 0.05 noise and reward = -|s|^2 / o - |a|^2 / a of the synthetic envs, float32, on numpy arrays or torch
    tensors alike: element-wise products and `_fold_sum`, so that both envs compute the same bits wherever they run."""
    s2 = _fold_sum(s[:, :, None] * A[None]) + _fold_sum(actions[:, :, None] * Bm[None]) + 0.05 * noise
    # (means as products with 1 / width: an array library may turn a division by a scalar into one, and then not divide as numpy does)
    rew = -(_fold_sum(s * s) * (1.0 / s.shape[1])) - (_fold_sum(actions * actions) * (1.0 / actions.shape[1]))
    return s2, rew


class _Box:
    def __init__(self, low, high, n, rng):
        self.low, self.high, self._n, self._rng = low, high, n, rng

    def seed(self, seed):
        self._rng = np.random.default_rng(seed)

    def sample(self):
        return self._rng.uniform(self.low, self.high, (self._n, len(self.low))).astype(np.float32)


class SyntheticVecEnv:
    """A deterministic, dependency-free vector env with gymnasium-0.29 autoreset semantics: linear dynamics
    s' = A s + B a + noise, reward = -|s|^2/o - |a|^2/a, termination when |s|_inf > `term_at`, truncation after
    `horizon` steps; on either, `infos["final_observation"][k]` / `infos["final_info"][k]` are set and the returned
    observation is the next episode's first one."""

    def __init__(self, ob_dim: int, ac_dim: int, num_envs: int, horizon: int = 50, term_at: float = 4.0, bound: float = 1.0):
        self.o, self.a, self.n, self.horizon, self.term_at = ob_dim, ac_dim, num_envs, horizon, term_at
        g = np.random.default_rng(12345)
        self.A = (0.95 * np.eye(ob_dim) + 0.05 * g.standard_normal((ob_dim, ob_dim)) / np.sqrt(ob_dim)).astype(np.float32)
        self.Bm = (0.3 * g.standard_normal((ac_dim, ob_dim))).astype(np.float32)
        self._rng = np.random.default_rng(0)
        self.action_space = _Box(np.full(ac_dim, -bound, np.float32), np.full(ac_dim, bound, np.float32), num_envs,
                                 np.random.default_rng(0))
        self.num_envs = num_envs

    def _fresh(self, k):
        return self._rng.standard_normal((k, self.o)).astype(np.float32)

    def reset(self, seed=None):
        if seed is not None:
            self._rng = np.random.default_rng(seed)
        self.s = self._fresh(self.n)
        self.t = np.zeros(self.n, int)
        self.ret = np.zeros(self.n)
        return self.s.copy(), {}

    def step(self, actions):
        actions = np.clip(np.asarray(actions, np.float32).reshape(self.n, self.a), self.action_space.low, self.action_space.high)
        noise = self._rng.standard_normal((self.n, self.o)).astype(np.float32)
        s2, rew = _dynamics(self.s, actions, self.A, self.Bm, noise)
        self.t += 1
        self.ret += rew
        term = np.abs(s2).max(1) > self.term_at
        trunc = (self.t >= self.horizon) & ~term
        infos: Dict[str, Any] = {}
        ended = term | trunc
        if ended.any():
            infos["final_observation"] = np.array([s2[k].copy() if ended[k] else None for k in range(self.n)], dtype=object)
            infos["final_info"] = np.array([{"episode": {"l": np.array([self.t[k]]), "r": np.array([self.ret[k]])}} if ended[k] else None
                                            for k in range(self.n)], dtype=object)
            s2 = s2.copy()
            s2[ended] = self._fresh(int(ended.sum()))
            self.t[ended] = 0
            self.ret[ended] = 0.0
        self.s = s2.astype(np.float32)
        return self.s.copy(), rew.astype(np.float32), term, trunc, infos


class _DeviceBox(_Box):
    """`_Box` whose samples are tensors of one device: the same host generator, so the same actions as the host env's space"""

    def __init__(self, low, high, n, rng, to_device):
        super().__init__(low, high, n, rng)
        self._to_device = to_device

    def sample(self):
        return self._to_device(super().sample())


class SyntheticDeviceVecEnv:
    """`SyntheticVecEnv` on torch tensors of one device (default: the current CUDA device) -- for `DeviceRollout`, and on
    torch.device("cpu") for tests: same dynamics (`_dynamics`), horizon, termination rule and auto-reset, and with the same seed the
    same observations, rewards and flags, bit for bit.  `step` takes an [n, a] tensor and returns tensors; nothing in it depends on
    the host knowing a value the device computed: envs are reset with selects over the `ended` mask, `infos` always holds
    `final_observation` -- an [n, o] tensor: the observation the step arrived at BEFORE any reset, for every env -- and its mask
    `_final_observation`; there is no `final_info` (evaluation episodes run on the host env).
    The host env draws its normals from one numpy generator, k x o fresh ones behind a step in which k envs ended.  The draws come
    from the same generator here, made on the host in blocks ahead of their use and kept in a device pool; the position in that
    sequence is a device scalar, advanced by n x o + k x o per step on the device.  The host only knows bounds of it (it grows by
    one to two times n x o per step): it draws up to the upper one and drops what lies below the lower one; the bounds are tightened
    from a copy of the device scalar that is requested now and then and used once it has arrived, never waited for.
    It is a test double: `action_space.sample()` (the random phase before `learning_starts`) and the block of normals drawn every few
    hundred steps are made by numpy on the host and uploaded from pageable memory, which holds the host for the length of that copy --
    the only host-side waits of a `DeviceRollout` step on this env, and neither waits for the device's queued work.  The fixed-order
    sums (`_dynamics`) cost an [n, o, o] temporary per step: at Humanoid's o = 376 the env, not the agent, is what a step of many
    envs spends its time on."""

    def __init__(self, ob_dim: int, ac_dim: int, num_envs: int, horizon: int = 50, term_at: float = 4.0, bound: float = 1.0,
                 device: Any = None):
        import torch
        self._t = torch
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.o, self.a, self.n, self.horizon, self.term_at = ob_dim, ac_dim, num_envs, horizon, term_at
        host = SyntheticVecEnv(ob_dim, ac_dim, num_envs, horizon, term_at, bound)           # the same matrices and bounds
        self.A, self.Bm = self._dev(host.A), self._dev(host.Bm)
        self.low, self.high = self._dev(host.action_space.low), self._dev(host.action_space.high)
        self.action_space = _DeviceBox(host.action_space.low, host.action_space.high, num_envs, np.random.default_rng(0), self._dev)
        self._rng = np.random.default_rng(0)
        self.num_envs = num_envs
        no = num_envs * ob_dim
        self._i_no = torch.arange(no, device=self.device)
        self._i_o = torch.arange(ob_dim, device=self.device).reshape(1, -1)
        self._block = max(64 * no, 1 << 16)        # normals drawn per host block
        self._refresh_every = 256

    def _dev(self, x):
        return self._t.from_numpy(np.ascontiguousarray(x)).to(self.device)

    def _draw_to(self, need: int) -> None:
        """make the pool hold the sequence of normals up to position `need`"""
        if self._drawn < need:
            k = max(need - self._drawn, self._block)
            self._pool = self._t.cat([self._pool, self._dev(self._rng.standard_normal(k).astype(np.float32))])
            self._drawn += k

    def _snapshot(self):
        """a copy of the position that the host may read later without waiting: -> (holder, arrived())"""
        if self.device.type == "cpu":
            return self._cur.clone(), lambda: True
        self._cur_host.copy_(self._cur, non_blocking=True)              # pinned: the copy is asynchronous
        ev = self._t.cuda.Event()
        ev.record(self._t.cuda.current_stream(self.device))
        return self._cur_host, ev.query

    def _tighten(self) -> None:
        """Every `_refresh_every` steps a copy of the position is requested; once it has arrived (asked, never waited for) the
        bounds restart from it, widened by the steps taken since.  Then the normals below the lower bound are dropped."""
        no = self.n * self.o
        if self._ask is None:
            if self._steps % self._refresh_every == 0:
                self._ask = self._snapshot() + (self._steps,)
        elif self._ask[1]():
            d, at = self._steps - self._ask[2], int(self._ask[0])
            self._lo, self._hi, self._ask = at + d * no, at + 2 * d * no, None
        if self._lo - self._base >= self._block:                 # no step can ask for these again
            self._pool = self._pool[self._lo - self._base:].clone()
            self._base = self._lo

    def reset(self, seed=None):
        t = self._t
        if seed is not None:
            self._rng = np.random.default_rng(seed)
        no = self.n * self.o
        self._pool, self._base, self._drawn = t.empty(0, dtype=t.float32, device=self.device), 0, 0
        self._draw_to(no)
        self.s = self._pool[:no].reshape(self.n, self.o).clone()
        self.t = t.zeros(self.n, dtype=t.int64, device=self.device)
        self._cur = t.full((), no, dtype=t.int64, device=self.device)         # position in the sequence of normals
        self._lo = self._hi = no
        self._steps, self._ask = 0, None
        if self.device.type != "cpu":
            self._cur_host = t.zeros((), dtype=t.int64).pin_memory()
        return self.s.clone(), {}

    def step(self, actions):
        t, n, o = self._t, self.n, self.o
        no = n * o
        self._tighten()
        self._draw_to(self._hi + 2 * no)
        actions = t.clamp(actions.to(t.float32).reshape(n, self.a), self.low, self.high)
        at = self._cur - self._base
        noise = self._pool[at + self._i_no].reshape(n, o)
        s2, rew = _dynamics(self.s, actions, self.A, self.Bm, noise)
        self.t = self.t + 1
        term = s2.abs().amax(1) > self.term_at
        trunc = (self.t >= self.horizon) & ~term
        ended = term | trunc
        rank = t.cumsum(ended.to(t.int64), 0) - 1                # the k-th env that ended takes the k-th row of fresh normals
        fresh = self._pool[(at + no + t.clamp(rank, min=0) * o).reshape(-1, 1) + self._i_o]
        self.s = t.where(ended.reshape(-1, 1), fresh, s2)
        self.t = t.where(ended, t.zeros_like(self.t), self.t)
        self._cur = self._cur + no + ended.sum() * o
        self._lo, self._hi, self._steps = self._lo + no, self._hi + 2 * no, self._steps + 1
        return self.s.clone(), rew, term, trunc, {"final_observation": s2, "_final_observation": ended}
