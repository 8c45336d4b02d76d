"""Seed-parallel runs: the reference's only "multi-GPU" mechanism is spawner.py emitting N independent
`python main.py train --seed k` jobs, one GPU each (spawner.py:147-178,210-211,291).  There is no exchange step on
the path, so the MI355X counterpart is replicas only: one process per GPU (torch.distributed.run), each owning an
independent learner for its share of the seeds; torch.distributed is used for the start barrier and for combining
the timings, never on the data path.
"""
from __future__ import annotations

import os
from typing import List, Optional, Tuple

from . import loop      # (numpy only: the parent process still opens no GPU)


def rank_info() -> Tuple[int, int, int]:
    """(rank, world_size, local_rank) from the torch.distributed.run environment (1 process: 0, 1, 0)."""
    return int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))


def shard_seeds(num_seeds: int, world_size: int, rank: int, first_seed: int = 0) -> List[int]:
    """Seeds first_seed .. first_seed+num_seeds-1 dealt round-robin over the ranks (spawner.py:166-178 numbers
    its jobs the same way: one job per (env, seed))."""
    assert 0 <= rank < world_size
    return [first_seed + s for s in range(num_seeds) if s % world_size == rank]


# The reference's sweep unit (spawner.py:21-38,147-178): an "environment bundle" names a list of tasks and a run is one job
# per (task, seed), tasks outermost.  The cluster side of spawner.py (SLURM / tmux scripts, wandb) is out of scope; `main()`
# below runs the sweep on this node, one learner process per GPU.
ENV_BUNDLES = {
    "debug": ["Hopper-v4"],
    "low": ["Hopper-v4", "Pusher-v4"],
    "medium": ["HalfCheetah-v4", "Walker2d-v4", "Ant-v4"],
    "high": ["Humanoid-v4", "HumanoidStandup-v4"],
    "native": ["Pendulum-native", "CartPole-native"],      # the two dense-reward tasks this package simulates itself (envs.py)
    "native_goal": ["PointGoal-native"],                   # ... and its goal-conditioned, sparse-reward one
}
NATIVE_ENVS = {"Pendulum-native": "pendulum", "CartPole-native": "cartpole", "PointGoal-native": "pointgoal"}      # env id -> envs.py kind


def sweep_jobs(env_bundle: str, num_seeds: int) -> List[Tuple[str, int]]:
    """[(env_id, seed)] in the reference's job order: for env in bundle: for seed in range(num_seeds)."""
    if env_bundle not in ENV_BUNDLES:
        raise ValueError(f"unknown env bundle {env_bundle!r} (one of {sorted(ENV_BUNDLES)})")
    if num_seeds < 1:
        raise ValueError("num_seeds must be positive")
    return [(env, seed) for env in ENV_BUNDLES[env_bundle] for seed in range(num_seeds)]


def shard_jobs(jobs: List[Tuple[str, int]], world_size: int, rank: int) -> List[Tuple[str, int]]:
    """This rank's share of a sweep: job k runs on GPU k mod world_size (one learner per GPU at a time, in order)."""
    assert 0 <= rank < world_size
    return [j for k, j in enumerate(jobs) if k % world_size == rank]


def init_process_group(backend: str = "nccl"):
    """Join the job's process group (nccl == RCCL on ROCm; gloo for CPU rehearsals).  Returns the module or None."""
    rank, world, local = rank_info()
    if world <= 1:
        return None
    import torch
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if backend == "nccl":
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    else:
        dist.init_process_group(backend)
    return dist


def aggregate(dist, local_units: float, local_seconds: float, device=None) -> Tuple[float, float]:
    """Whole-job figures: units summed over ranks, time = the slowest rank's.  Returns (total_units, seconds)."""
    if dist is None:
        return float(local_units), float(local_seconds)
    import torch
    t = torch.tensor([local_seconds], dtype=torch.float64, device=device)
    u = torch.tensor([local_units], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dist.all_reduce(u, op=dist.ReduceOp.SUM)
    return float(u.item()), float(t.item())


class SharedReplay:
    """Optional shared-replay variant (BASELINE.json north_star; not in the reference): every rank appends the new
    transitions of ALL ranks, so each GPU's ring holds every seed's data, in rank order (all rings stay identical).  The
    exchange is the only collective on the data path, and only in this variant; it is latency-bound (num_envs x ~100 B per
    rank and env step), so `every=K` batches K env steps into one exchange.

    Two paths, chosen by what `rb` is:
      * device path (`rb` is this package's ReplayBuffer bound to an engine, `device` a cuda device): the rank's rows are packed
        into the ring's record layout, ONE all_gather_into_tensor (RCCL over xGMI when the backend is nccl) fills a device slab
        [world x rows, record] and the engine appends the slab with one kernel (`sactd3_rb_extend_device`): no device -> host
        copy, no per-key collectives;
      * host path (any buffer with the reference's `extend(td)` / `sample(B)` / `len()`; gloo rehearsals): one all_gather per
        key, rows appended through `rb.extend`."""

    KEYS = ("observations", "next_observations", "actions", "rewards", "terminations", "dones")

    def __init__(self, dist, rb, device=None, every: int = 1, force_device_path: bool = False):
        self.dist, self.rb, self.device, self.every = dist, rb, device, max(int(every), 1)
        self._pending: list = []
        eng = getattr(rb, "_engine", None)
        self._engine = eng if (eng is not None and device is not None and str(device).startswith("cuda")
                               and (force_device_path or dist is not None)) else None
        self._slab = None                         # kept alive until the engine has consumed it

    # -- device path
    def _exchange_device(self, td_list) -> None:
        import numpy as np
        import torch
        eng = self._engine
        rec = np.concatenate([eng.pack_records(_host(td["observations"]), _host(td["actions"]), _host(td["rewards"]),
                                               _host(td["next_observations"]), _host(td["dones"] if "dones" in td else td["terminations"]))
                              for td in td_list])
        world = self.dist.get_world_size() if self.dist is not None else 1
        eng.sync()                                # the previous slab has been read by now: its memory may be reused
        mine = torch.from_numpy(rec).to(self.device, non_blocking=False)
        if self.dist is not None and world > 1:
            slab = torch.empty((world * rec.shape[0], rec.shape[1]), dtype=torch.float32, device=self.device)
            self.dist.all_gather_into_tensor(slab, mine)
        else:
            slab = mine
        torch.cuda.current_stream(slab.device).synchronize()      # the collective ran on torch's stream, the ingest runs on the engine's
        self._slab = slab
        eng.rb_extend_device(slab.data_ptr(), slab.shape[0])

    # -- host path
    def _exchange_host(self, td) -> None:
        import numpy as np
        import torch
        world = self.dist.get_world_size()
        out = {}
        for k in self.KEYS:
            if k not in td:
                continue
            x = td[k]
            x = x.detach() if hasattr(x, "detach") else torch.as_tensor(np.asarray(x))
            x = x.to(torch.float32).reshape(x.shape[0], -1).contiguous()
            if self.device is not None:
                x = x.to(self.device)
            buf = [torch.empty_like(x) for _ in range(world)]
            self.dist.all_gather(buf, x)
            out[k] = torch.cat(buf, 0).cpu().numpy()
        for k in ("terminations", "dones"):
            if k in out:
                out[k] = out[k] != 0
        self.rb.extend(out)

    def extend(self, td) -> None:
        if self._engine is not None:
            self._pending.append(td)
            if len(self._pending) >= self.every:
                pend, self._pending = self._pending, []
                self._exchange_device(pend)
            return
        if self.dist is None:
            return self.rb.extend(td)
        self._exchange_host(td)

    def flush(self) -> None:
        if self._engine is not None and self._pending:
            pend, self._pending = self._pending, []
            self._exchange_device(pend)

    def sample(self, batch_size):
        return self.rb.sample(batch_size)

    def __len__(self):
        return len(self.rb)


def _host(x):
    import numpy as np
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


# ------------------------------------------------------------------------------------------------ the sweep runner
# spawner.py:147-178,240-349 turns (env bundle x seeds) into one `python main.py train --env_id .. --seed ..` job per pair and
# hands each to Slurm with --gres=gpu:1 (or to a tmux window).  Here the node IS the scheduler: the parent process (which
# never touches a GPU) starts one worker process per GPU, worker r runs jobs r, r + N, r + 2N, ... one after the other with
# `loop.train`, each job with its own engine, replay ring, seed and output directory, and prints one JSON line per job;
# the parent relays them and ends with a summary line.  No collective, no shared state: replicas only.
ENV_DIMS = {   # (ob_dim, ac_dim, action bound) of the Gymnasium MuJoCo -v4 tasks named by the bundles (public task specs)
    "Hopper-v4": (11, 3, 1.0), "Pusher-v4": (23, 7, 2.0), "HalfCheetah-v4": (17, 6, 1.0), "Walker2d-v4": (17, 6, 1.0),
    "Ant-v4": (27, 8, 1.0), "Humanoid-v4": (376, 17, 0.4), "HumanoidStandup-v4": (376, 17, 0.4),
    "Pendulum-native": (3, 1, 2.0), "CartPole-native": (4, 1, 1.0), "PointGoal-native": (6, 2, 1.0),      # include/sactd3_env.h
}


def env_plan(env_id: str, device_env: bool, has_factory: bool = False, native_rollout: Optional[bool] = None):
    """Which env classes a job uses, decided without touching a GPU: -> dict(train=, eval=) of class names.  The -native ids are
    simulated by this package: `envs.HostVecEnv` trains and evaluates on the host, and with --device_env `envs.NativeVecEnv` does both
    on the GPU (evaluation through `envs.device_episodes`: no host env step anywhere in the job).  Every other id is what it was: the
    caller's factory or the synthetic stand-in, and the synthetic device env for training with --device_env.
    `native_rollout` (True / False; None: the question is not asked and the plan has no such key) adds rollout=: the class of `loop`
    that drives the training env -- "NativeRollout" with --native_rollout, which needs --device_env and a -native id without a
    factory (ValueError otherwise), else "DeviceRollout" with --device_env and "Rollout" without."""
    if env_id in NATIVE_ENVS and not has_factory:
        plan = dict(train="NativeVecEnv", eval="NativeVecEnv") if device_env else dict(train="HostVecEnv", eval="HostVecEnv")
    else:
        base = "factory" if has_factory else "SyntheticVecEnv"
        plan = dict(train="SyntheticDeviceVecEnv" if device_env else base, eval=base)
    if native_rollout is not None:
        if native_rollout and not device_env:
            raise ValueError("--native_rollout needs --device_env: it drives an env that lives on the GPU")
        if native_rollout and plan["train"] != "NativeVecEnv":
            raise ValueError(f"--native_rollout needs a -native env id ({', '.join(NATIVE_ENVS)}) without --env_factory: {env_id} "
                             "has no env that emits ring records")
        plan["rollout"] = "NativeRollout" if native_rollout else ("DeviceRollout" if device_env else "Rollout")
    return plan
DEFAULTS = {   # tasks/defaults/sac.yml:1-48 (td3.yml differs in the keys listed under "td3")
    "sac": dict(num_envs=4, action_repeat=1, measure_burnin=3, num_timesteps=10_000_000, learning_starts=5000, eval_steps=10,
                eval_every=10_000, layer_norm=True, actor_lr=3e-4, qnets_lr=1e-3, clip_norm=0.0, segment_len=1, batch_size=256,
                gamma=0.99, rb_capacity=1_000_000, polyak=0.005, prefer_td3_over_sac=False, bcq_style_targ_mix=False,
                actor_update_delay=2, crit_targ_update_freq=1, alpha_init=0.2, autotune=True, log_alpha_lr=1e-3),
    "td3": dict(prefer_td3_over_sac=True, bcq_style_targ_mix=True, qnets_lr=3e-4, actor_noise_std=0.1, targ_actor_smoothing=True,
                td3_std=0.2, td3_c=0.5),
}


def job_config(algo: str, env_id: str, seed: int, **over):
    from types import SimpleNamespace
    cfg = dict(DEFAULTS["sac"])
    if algo == "td3":
        cfg.update(DEFAULTS["td3"])
    cfg.update(env_id=env_id, seed=seed, cudagraphs=False, compile=False)
    cfg.update({k: v for k, v in over.items() if v is not None})
    return SimpleNamespace(**cfg)


def offline_plan(args):
    """What --offline_dataset / --bc_alpha / --num_updates ask for, checked without touching a GPU.  -> None for an online run, else
    dict(dataset=, num_updates=, bc_alpha=).  ValueError: --bc_alpha with --algo sac (the behaviour-cloning term exists in the TD3
    engine only), a negative or non-finite --bc_alpha, --num_updates without a dataset or below 1, or an online-only switch
    (--overlap_acting, --device_env, --prioritized, --n_step, --one_launch: they shape the env loop) beside a dataset.  A dataset
    WITHOUT --bc_alpha is accepted for either algorithm -- plain TD3 / SAC on a fixed ring, the baseline that usually diverges -- and
    flagged in the plan (`plain=True`) so that the caller can say so."""
    import math
    bc_alpha = 0.0 if args.bc_alpha is None else float(args.bc_alpha)
    if not math.isfinite(bc_alpha) or bc_alpha < 0.0:
        raise ValueError("--bc_alpha must be finite and >= 0")
    if bc_alpha > 0.0 and args.algo != "td3":
        raise ValueError("--bc_alpha needs --algo td3: the behaviour-cloning actor term (TD3+BC) exists in the TD3 engine only")
    # --prior_fraction F beside a dataset: an ONLINE run on top of the pinned dataset (load, pin, loop.train) -- the plan says so with
    # two more keys; --updates_per_step G: any online run.  Without the two flags the plan is what it always was.
    prior, utd = getattr(args, "prior_fraction", None), getattr(args, "updates_per_step", None)
    if utd is not None and int(utd) < 1:
        raise ValueError("--updates_per_step must be >= 1")
    if prior is not None and not 0.0 <= float(prior) <= 1.0:                               # (false for NaN)
        raise ValueError("--prior_fraction must be in [0, 1]")
    if args.offline_dataset is None:
        if args.num_updates is not None:
            raise ValueError("--num_updates needs --offline_dataset (an online run is sized by --num_timesteps)")
        if prior is not None:
            raise ValueError("--prior_fraction needs --offline_dataset: the prior data the batches take their share from")
        return None
    if prior is not None:
        excluded = (["prioritized"] if args.prioritized else []) + (["n_step"] if args.n_step != 1 else []) + \
                   (["num_updates"] if args.num_updates is not None else [])
        if excluded:
            raise ValueError("--prior_fraction excludes " + ", ".join("--" + k for k in excluded) +
                             ": a pinned ring has no priorities and no n-step chains yet, and the run is sized by --num_timesteps")
        return dict(dataset=args.offline_dataset, num_updates=None, bc_alpha=bc_alpha, plain=bc_alpha == 0.0,
                    prior_fraction=float(prior), updates_per_step=1 if utd is None else int(utd))
    if utd is not None:
        raise ValueError("--updates_per_step needs an env loop: with --offline_dataset add --prior_fraction (the number of updates is --num_updates)")
    online_only = [k for k in ("overlap_acting", "device_env", "prioritized", "one_launch") if getattr(args, k)] + (["n_step"] if args.n_step != 1 else [])
    if online_only:
        raise ValueError("--offline_dataset excludes " + ", ".join("--" + k for k in online_only) + ": there is no env loop to shape")
    if args.num_updates is not None and args.num_updates < 1:
        raise ValueError("--num_updates must be >= 1")
    return dict(dataset=args.offline_dataset, num_updates=args.num_updates, bc_alpha=bc_alpha, plain=bc_alpha == 0.0)


def policy_stats_plan(args) -> int:
    """What --policy_stats N asks for, checked without touching a GPU.  -> N (0: off).  ValueError: a negative N, or N > 0 with --algo td3
    (there is no SAC policy to ask: TD3's actor has no log-probability, entropy or log-std)."""
    n = int(getattr(args, "policy_stats", 0) or 0)
    if n < 0:
        raise ValueError("--policy_stats must be >= 0")
    if n > 0 and args.algo != "sac":
        raise ValueError("--policy_stats needs --algo sac: TD3's deterministic actor has no log-probability, entropy or log-std to report")
    return n


def eval_plan(args, env_ids, has_factory: bool) -> dict:
    """What --eval_one_launch and --q_bias N ask for, checked in the parent without touching a GPU, for every env id of the sweep: both go
    through the one-launch rollout (envs.policy_rollout), whose env physics runs inside the kernel -- so they need --device_env and a
    native env bundle without --env_factory.  -> the keys run_job takes, each only when its flag was given.  ValueError otherwise."""
    one, n = bool(getattr(args, "eval_one_launch", False)), int(getattr(args, "q_bias", 0) or 0)
    if n < 0:
        raise ValueError("--q_bias must be >= 0")
    if one or n:
        which = " and ".join(w for w, on in (("--eval_one_launch", one), ("--q_bias", n)) if on)
        foreign = [e for e in env_ids if e not in NATIVE_ENVS]
        if not args.device_env or has_factory or foreign:
            raise ValueError(f"{which} need(s) --device_env and a native env bundle without --env_factory: the evaluation episodes run "
                             "inside one kernel, with the env's physics" + (f" ({', '.join(foreign)} is simulated elsewhere)" if foreign else ""))
    return dict(**(dict(eval_one_launch=True) if one else {}), **(dict(q_bias=n) if n else {}))


def native_rollout_plan(env_ids, device_env: bool, has_factory: bool, offline: bool, overlap_acting: bool) -> None:
    """What --native_rollout excludes, checked without touching a GPU for every env id it is asked for: ValueError with a dataset or
    --overlap_acting beside it, and whatever env_plan refuses."""
    if offline or overlap_acting:
        raise ValueError("--native_rollout excludes --offline_dataset and --overlap_acting")
    for env_id in env_ids:
        env_plan(env_id, device_env, has_factory, native_rollout=True)


def goal_layout_of(env_id: str, has_factory: bool = False) -> Optional[dict]:
    """dict(achieved=, desired=, dim=, threshold=, horizon=) of a -native env id whose task has a goal (envs.GOAL_LAYOUTS), else None;
    decided without touching a GPU"""
    if env_id not in NATIVE_ENVS or has_factory:
        return None
    from . import envs      # (numpy and ctypes only)
    kind = envs.kind_of(NATIVE_ENVS[env_id])
    if kind not in envs.GOAL_LAYOUTS:
        return None
    return dict(envs.GOAL_LAYOUTS[kind], horizon=envs.SPECS[kind][3])


def hindsight_plan(env_ids, has_factory: bool, offline: bool) -> None:
    """What --hindsight needs, checked without touching a GPU for every env id it is asked for: ValueError for an env without a goal
    layout, and beside a dataset"""
    if offline:
        raise ValueError("--hindsight excludes --offline_dataset: there is no env loop whose episodes could be relabelled")
    for env_id in env_ids:
        if goal_layout_of(env_id, has_factory) is None:
            with_goal = [k for k in NATIVE_ENVS if goal_layout_of(k) is not None]
            raise ValueError(f"--hindsight needs an env with a goal layout ({', '.join(with_goal)}) without --env_factory: {env_id} has none")


def hindsight_keywords(env_id: str, num_envs: int) -> dict:
    """loop.train's hindsight=dict(...) for a goal env id: its layout, window = its horizon, stride = the env count"""
    lay = goal_layout_of(env_id)
    return dict(achieved=lay["achieved"], desired=lay["desired"], dim=lay["dim"], threshold=lay["threshold"], window=lay["horizon"],
                stride=int(num_envs))


def mode_flags(args, plan) -> dict:
    """the flags that shape the env loop, under the names run_job and train_keywords take them by (`plan`: offline_plan(args) or {});
    `hindsight` is among them only when --hindsight was given"""
    flags = dict(prioritized=args.prioritized, n_step=args.n_step, one_launch=args.one_launch, prior_fraction=plan.get("prior_fraction"),
                 updates_per_step=args.updates_per_step or 1, overlap_acting=args.overlap_acting, device_env=args.device_env,
                 native_rollout=args.native_rollout, policy_stats=policy_stats_plan(args))
    if getattr(args, "hindsight", False):
        flags["hindsight"] = True
    if getattr(args, "fused_rollout", False):    # (the same: the key is there only when the flag was given)
        flags["fused_rollout"] = True
    if getattr(args, "collected_rollout", False):           # (the same)
        flags["collected_rollout"] = True
    if getattr(args, "reset_every", None) is not None:      # (the same)
        flags["reset_every"] = int(args.reset_every)
        flags["reset_what"] = reset_names(getattr(args, "reset_what", None))
    elif getattr(args, "reset_what", None) is not None:
        raise ValueError("--reset_what needs --reset_every N: it names the networks that rule resets")
    if getattr(args, "init", "torch") != "torch":           # (the same)
        flags["init"] = args.init
    if getattr(args, "eval_one_launch", False) or getattr(args, "q_bias", 0):      # (the same: keys only when a flag was given; every job
        flags.update(eval_plan(args, ENV_BUNDLES[args.env_bundle], bool(args.env_factory)))      # of the sweep is asked, in the parent)
    return flags


def reset_names(text=None) -> tuple:
    """--reset_what 'actor,critics,alpha' -> the names as loop.train takes them (None: all three)"""
    return tuple(loop.RESET_ALL) if text is None else tuple(w.strip() for w in str(text).split(","))


def train_keywords(cfg, *, prioritized: bool, n_step: int, one_launch: bool, prior_fraction, updates_per_step, overlap_acting: bool,
                   device_env: bool, native_rollout: bool, policy_stats: int, hindsight=None, fused_rollout: bool = False,
                   reset_every=None, reset_what=None, init: str = "torch", num_updates=None, collected_rollout: bool = False) -> dict:
    """The command line's facts as the keywords of loop.train, in this one place, and asked of loop.update_plan on the way (`cfg`: a
    job_config; no agent, no GPU): ValueError for a run that loop.train would refuse.  run_job passes the keywords on; main() asks
    before a worker starts.  --prioritized is the engine-owned proportional priorities (Schaul et al. 2016: alpha 0.6, beta 0.4); it,
    --n_step N > 1 and --prior_fraction are issued call by call (fused=False), or with --one_launch as one graph launch per iteration.
    `hindsight` (--hindsight: the dict of hindsight_keywords for the job's env): call by call as well, or with --one_launch as one
    graph launch; the key is in the result only when it was given.
    `fused_rollout` (--fused_rollout: a loop body as one graph launch, loop.NativeRollout.cycle): asked of loop.rollout_for's own rules
    and of loop.update_plan beside the other keywords; the key is in the result only when it was given.
    `collected_rollout` (--collected_rollout: a segment as one call, loop.NativeRollout.collect): asked of loop.rollout_for's rules with
    the job's action_repeat, no env looked at; the key is in the result only when it was given.
    `reset_every` / `reset_what` (--reset_every N [--reset_what actor,critics,alpha]: periodic resets of the networks on the kept ring,
    loop.train reset_every=...): asked of loop.update_plan's table as well -- with `num_updates`, the length of an offline plan, which
    has to reach N; the keys are in the result only when --reset_every was given.  `init` (--init: who makes the initial parameters)
    is the Agent's keyword, not loop.train's: checked here, never in the result."""
    if init not in ("torch", "engine"):
        raise ValueError(f'--init is "torch" or "engine", not {init!r}')
    if fused_rollout and not (native_rollout and not overlap_acting):      # (its two rules stand in front of the env's: no env is looked at)
        loop.rollout_for(None, overlap=overlap_acting, device_env=device_env, native_rollout=native_rollout, fused_rollout=True)
    if collected_rollout:                                                  # (the same: its rules stand in front of the env's)
        loop.collected_rollout_rules(overlap=overlap_acting, native_rollout=native_rollout, fused_rollout=fused_rollout,
                                     action_repeat=int(cfg.action_repeat), segment_len=int(cfg.segment_len))
    update = dict(fused=not prioritized and n_step == 1 and prior_fraction is None and not hindsight,
                  prioritized=dict(alpha=0.6, beta=0.4, eps=1e-6) if prioritized else None, n_step=n_step, one_launch=one_launch,
                  prior_fraction=None if prior_fraction is None else float(prior_fraction), updates_per_step=int(updates_per_step))
    if hindsight:
        update["hindsight"] = dict(hindsight)
    if fused_rollout:
        update["fused_rollout"] = True
    if reset_every is not None:
        update["reset_every"], update["reset_what"] = int(reset_every), tuple(reset_what if reset_what is not None else loop.RESET_ALL)
    loop.update_plan(cfg, sampler=None, **update, **(dict(num_updates=int(num_updates)) if num_updates is not None else {}))
    rollout = dict(collected_rollout=True) if collected_rollout else {}
    return dict(update, overlap=overlap_acting, device_env=device_env, native_rollout=native_rollout, policy_stats=int(policy_stats), **rollout)


def run_job(algo: str, env_id: str, seed: int, device_index: int, out_dir, env_factory=None, overlap_acting: bool = False,
            device_env: bool = False, prioritized: bool = False, n_step: int = 1, one_launch: bool = False,
            offline_dataset=None, num_updates=None, prior_fraction=None, updates_per_step: int = 1, policy_stats: int = 0,
            native_rollout: bool = False, hindsight: bool = False, fused_rollout: bool = False, init: str = "torch",
            reset_every=None, reset_what=None, eval_one_launch: bool = False, q_bias: int = 0, collected_rollout: bool = False, **over):
    """One (env, seed) run = what one `main.py train` process of the reference does (main.py:126-195), on one GPU.
    `offline_dataset` (an .npz with the keys of rb.extend): no env loop -- the ring is filled once (loop.load_dataset) and
    `num_updates` iterations (default: cfg.num_timesteps) run through loop.train_offline, evaluated every cfg.eval_every of them;
    `bc_alpha` in `over` turns the TD3+BC actor term on.
    `prior_fraction` beside `offline_dataset`: an online run on top of the dataset instead -- the ring is filled and its rows pinned
    (loop.load_dataset(pin=True)), then loop.train draws that share of every batch from them; `updates_per_step`: updates per
    segment of any online run; `policy_stats`: rows put to the policy at every evaluation (loop.PolicyStats; SAC only);
    `native_rollout`: the env loop through loop.NativeRollout (needs `device_env` and a -native id: env_plan refuses otherwise);
    `hindsight`: the engine relabels goals while it stages each batch (loop.train hindsight=...; needs an env id with a goal layout:
    hindsight_plan refuses otherwise); with `one_launch` the draw and the relabelling are part of the iteration's one graph.
    `fused_rollout`: with `native_rollout`, a loop body past learning_starts as one graph launch (loop.train fused_rollout=True).
    `collected_rollout`: with `native_rollout`, every segment is one library call (loop.train collected_rollout=True).
    `init`: "engine" = the initial parameters come from the engine's own initialiser under the job's seed (Agent init="engine"), not
    from torch's; `reset_every` [, `reset_what`]: periodic resets of the networks on the kept ring (loop.train / loop.train_offline
    reset_every=...).
    `eval_one_launch`: with `device_env` on a native id, every evaluation window is one kernel launch (envs.device_episodes
    one_launch=True); `q_bias` = N > 0: N further evaluation envs, and at every evaluation the normalised Q-bias of the current policy on
    fresh episodes of them (loop.train q_bias=dict(env=, seed=)); both need what eval_plan states."""
    import json
    import time
    from pathlib import Path
    import numpy as np
    import torch
    from .agent import Agent, ReplayBuffer
    if int(policy_stats) and algo != "sac":      # (before anything is built)
        raise ValueError("policy_stats needs algo sac: TD3's deterministic actor has no log-probability, entropy or log-std to report")
    if native_rollout:                           # (before anything is built)
        native_rollout_plan([env_id], device_env, env_factory is not None, offline_dataset is not None, overlap_acting)
    if hindsight:                                # (before anything is built)
        hindsight_plan([env_id], env_factory is not None, offline_dataset is not None)
    if (eval_one_launch or int(q_bias)) and not (device_env and env_id in NATIVE_ENVS and env_factory is None):      # (before anything is built)
        raise ValueError("eval_one_launch / q_bias need device_env and a native env id without an env factory")
    cfg = job_config(algo, env_id, seed, **over)
    o, a, bound = ENV_DIMS[env_id]
    native = env_id in NATIVE_ENVS and env_factory is None      # the tasks this package simulates itself (env_plan)
    on_gpu = native and device_env                              # ... with --device_env on the GPU, training AND evaluation: no host env
    dev = torch.device("cuda", device_index)
    if native:
        from . import envs
        make = lambda n: envs.HostVecEnv(NATIVE_ENVS[env_id], n, seed=seed)      # the numpy twin on the host
    elif env_factory is None:   # no MuJoCo in this image: the synthetic vector env has the task's shapes and the gymnasium protocol
        make = lambda n: loop.SyntheticVecEnv(o, a, n, horizon=200, term_at=6.0, bound=bound)
    else:
        make = lambda n: env_factory(env_id, n, seed)
    if on_gpu:
        env, eval_env = envs.NativeVecEnv(NATIVE_ENVS[env_id], cfg.num_envs, seed=seed, device=dev), None
    else:
        env, eval_env = make(cfg.num_envs), make(1)
    if device_env and not native:   # the training env lives on the GPU (loop.DeviceRollout); evaluation keeps its host env and predict()
        env = loop.SyntheticDeviceVecEnv(o, a, cfg.num_envs, horizon=200, term_at=6.0, bound=bound, device=dev)
    torch.manual_seed(seed)                                           # main.py:145-146
    rb = ReplayBuffer(cfg.rb_capacity)
    agent = Agent({"ob_shape": (o,), "ac_shape": (a,)}, np.full(a, -bound, np.float32), np.full(a, bound, np.float32),
                  torch.device("cuda", device_index), cfg, rb, seed=seed, **(dict(init=init) if init != "torch" else {}))
    resets = dict(reset_every=reset_every, reset_what=reset_what) if reset_every is not None else {}
    run_dir = Path(out_dir) / f"{env_id}__{algo}__seed{seed:02d}"
    tab = loop.Tabular(run_dir)
    ev = loop.Evaluator(cfg, eval_env, agent, tabular=tab, ckpt_dir=run_dir)
    if on_gpu:                # cfg.eval_steps greedy episodes per evaluation, in lock-step on the GPU, read with one host wait
        ev.ep_gen = envs.device_episodes(envs.NativeVecEnv(NATIVE_ENVS[env_id], cfg.eval_steps, seed=seed, device=dev), agent, seed,
                                         **(dict(one_launch=True) if eval_one_launch else {}))
    bias = {}
    if int(q_bias):           # a horizon of its own: the task's plus the steps gamma needs to fall to q_bias' tail_tol, so that a time-limited
        g = float(getattr(cfg, "gamma", 0.99))                            # task (the pendulum) has rows whose return is complete enough to count
        tail = int(np.ceil(np.log(0.05) / np.log(g))) if 0.0 < g < 1.0 else 0
        horizon = min(envs.SPECS[envs.kind_of(NATIVE_ENVS[env_id])][3] + tail, 4096)
        bias = dict(q_bias=dict(env=envs.NativeVecEnv(NATIVE_ENVS[env_id], int(q_bias), seed=seed, device=dev, horizon=horizon), seed=seed))
    t0 = time.time()
    if offline_dataset is not None:
        with np.load(offline_dataset) as z:
            data = {k: z[k] for k in z.files}
        if data["observations"].shape[1:] != (o,) or data["actions"].shape[1:] != (a,):
            raise ValueError(f"{offline_dataset}: observations / actions are {data['observations'].shape[1:]} / {data['actions'].shape[1:]}, "
                             f"{env_id} has ({o},) / ({a},)")
        loop.load_dataset(agent, data, pin=prior_fraction is not None)
    if offline_dataset is not None and prior_fraction is None:
        metrics = loop.train_offline(cfg, agent, num_updates=int(num_updates if num_updates is not None else cfg.num_timesteps),
                                     evaluator=ev, eval_every_updates=int(cfg.eval_every), policy_stats=int(policy_stats),
                                     **({k: v for k, v in resets.items() if v is not None}), **bias)
    else:
        kw = train_keywords(cfg, prioritized=prioritized, n_step=n_step, one_launch=one_launch, prior_fraction=prior_fraction,
                            updates_per_step=updates_per_step, overlap_acting=overlap_acting, device_env=device_env,
                            native_rollout=native_rollout, policy_stats=policy_stats,
                            **(dict(hindsight=hindsight_keywords(env_id, cfg.num_envs)) if hindsight else {}),
                            **(dict(fused_rollout=True) if fused_rollout else {}),
                            **(dict(collected_rollout=True) if collected_rollout else {}), **resets)
        metrics = loop.train(cfg, env, agent, evaluator=ev, **kw, **bias)
    agent.engine.sync()
    dt = time.time() - t0
    tab.close()
    out = {"env_id": env_id, "algo": algo, "seed": seed, "gpu": device_index, "timesteps": int(agent.timesteps_so_far),
           "gradient_steps": int(agent.qnet_updates_so_far), "actor_updates": int(agent.actor_updates_so_far), "seconds": dt,
           "gradient_steps_per_s": agent.qnet_updates_so_far / max(dt, 1e-9), "best_eval_return": float(agent.best_eval_ep_ret),
           "final_metrics": metrics, "dir": str(run_dir)}
    (run_dir / "summary.json").write_text(json.dumps(out))
    agent.engine.close()
    return out


def _worker_main(args, plan, flags) -> int:
    import importlib
    import json
    jobs = shard_jobs(sweep_jobs(args.env_bundle, args.num_seeds), args.world, args.rank)
    factory = None
    if args.env_factory:
        mod, fn = args.env_factory.split(":")
        factory = getattr(importlib.import_module(mod), fn)
    for env_id, seed in jobs:
        if args.dry_run:
            out = {"env_id": env_id, "algo": args.algo, "seed": seed, "gpu": args.rank, "dry_run": True,
                   "rollout": env_plan(env_id, args.device_env, factory is not None, native_rollout=args.native_rollout)["rollout"]}
            if args.hindsight:                   # (the key is there only when the flag was given)
                out["hindsight"] = hindsight_keywords(env_id, job_config(args.algo, env_id, seed).num_envs)
                if args.one_launch:              # (... and the one-launch form of its iteration beside it)
                    out["one_launch"] = True
            if args.fused_rollout:               # (the same: a key only when the flag was given)
                out["fused_rollout"] = True
            if args.collected_rollout:           # (the same)
                out["collected_rollout"] = True
            for k in ("init", "reset_every", "reset_what", "eval_one_launch", "q_bias"):      # (the same)
                if k in flags:
                    out[k] = flags[k]
        else:
            out = run_job(args.algo, env_id, seed, args.device if args.device >= 0 else args.rank, args.out, factory,
                          num_timesteps=args.num_timesteps, learning_starts=args.learning_starts, eval_every=args.eval_every,
                          eval_steps=args.eval_steps, batch_size=args.batch_size, rb_capacity=args.rb_capacity,
                          offline_dataset=plan.get("dataset"), num_updates=plan.get("num_updates"), bc_alpha=args.bc_alpha, **flags)
        print("JOB " + json.dumps(out), flush=True)
    return 0


def main(argv=None) -> int:
    import argparse
    import json
    import subprocess
    import sys
    import time
    ap = argparse.ArgumentParser(prog="python -m sac_td3_cudagraphs_pytorch_amd.launcher",
                                 description="(env bundle x seeds) sweep, one learner process per GPU (spawner.py semantics, no Slurm / tmux)")
    ap.add_argument("--env_bundle", default="debug", choices=sorted(ENV_BUNDLES))
    ap.add_argument("--num_seeds", type=int, default=8)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--algo", default="sac", choices=["sac", "td3"])
    ap.add_argument("--out", default="runs")
    ap.add_argument("--num_timesteps", type=int, default=None)
    ap.add_argument("--learning_starts", type=int, default=None)
    ap.add_argument("--eval_every", type=int, default=None)
    ap.add_argument("--eval_steps", type=int, default=None)
    ap.add_argument("--batch_size", type=int, default=None)
    ap.add_argument("--rb_capacity", type=int, default=None)
    ap.add_argument("--env_factory", default=None, help="module:function(env_id, num_envs, seed) -> gymnasium-protocol vector env (default: synthetic)")
    ap.add_argument("--device", type=int, default=-1, help="run every worker on this device ordinal (one-GPU rehearsals of N workers)")
    ap.add_argument("--overlap_acting", action="store_true",
                    help="compute the next action on the engine's acting stream while the iteration's update runs (loop.train overlap=True)")
    ap.add_argument("--device_env", action="store_true",
                    help="train on the GPU-resident vector env (the synthetic one; for the -native ids envs.NativeVecEnv, which also evaluates "
                         "there): observations and actions never leave the device (loop.train device_env=True)")
    ap.add_argument("--native_rollout", action="store_true",
                    help="with --device_env and a -native env bundle: the env step writes ring records and choose / advance are one library "
                         "call each (loop.train native_rollout=True); the default stays loop.DeviceRollout")
    ap.add_argument("--fused_rollout", action="store_true",
                    help="with --device_env --native_rollout: past learning_starts a loop body -- env step, ring append, next action, update -- "
                         "is one library call and one graph launch (loop.train fused_rollout=True); excludes the other draws")
    ap.add_argument("--collected_rollout", action="store_true",
                    help="with --device_env --native_rollout: every segment of segment_len env steps -- actions, env steps, ring records, the "
                         "append -- is one library call and two launches (loop.train collected_rollout=True); excludes --fused_rollout and "
                         "--overlap_acting, needs action_repeat 1")
    ap.add_argument("--hindsight", action="store_true",
                    help="with an env bundle whose tasks have a goal (native_goal): the engine relabels goals while it stages each batch -- "
                         "hindsight experience replay, the future strategy, window = the task's horizon (loop.train hindsight=...; the "
                         "iteration is issued call by call, or with --one_launch as one graph launch)")
    ap.add_argument("--prioritized", action="store_true",
                    help="proportional prioritised replay kept by the engine (loop.train prioritized=...; the iteration is issued call by call)")
    ap.add_argument("--one_launch", action="store_true",
                    help="with --prioritized, --n_step N > 1, --prior_fraction and / or --hindsight: issue the iteration as one graph launch "
                         "(loop.train one_launch=True)")
    ap.add_argument("--n_step", type=int, default=1,
                    help="train the critics on N-step returns chained by the engine (loop.train n_step=...; above 1 the iteration is issued call by call)")
    ap.add_argument("--offline_dataset", default=None, metavar="FILE.npz",
                    help="train on a fixed dataset instead of an env loop: an .npz with observations, actions, rewards, next_observations, "
                         "terminations [, dones] of the job's env dims (loop.load_dataset + loop.train_offline); evaluated every --eval_every updates")
    ap.add_argument("--bc_alpha", type=float, default=None,
                    help="TD3+BC: the behaviour-cloning actor term with this alpha (2.5 in Fujimoto & Gu 2021); needs --algo td3")
    ap.add_argument("--num_updates", type=int, default=None, help="with --offline_dataset: iterations to run (default: --num_timesteps)")
    ap.add_argument("--prior_fraction", type=float, default=None, metavar="F",
                    help="with --offline_dataset: an ONLINE run on top of the dataset -- its rows are pinned in the ring and every batch takes "
                         "round(F * batch_size) rows from them, the others from the rows the run appends (loop.train prior_fraction=...)")
    ap.add_argument("--updates_per_step", type=int, default=None, metavar="G",
                    help="any online run: G updates after each segment instead of one (loop.train updates_per_step=...)")
    ap.add_argument("--init", default="torch", choices=["torch", "engine"],
                    help="who makes the initial parameters: torch's orthogonal_ on the host under torch's seed (the reference's values), or "
                         "the engine's own initialiser on the device under the job's seed (Agent init=...)")
    ap.add_argument("--reset_every", type=int, default=None, metavar="N",
                    help="reset the networks on the kept replay ring whenever the update count reaches a multiple of N (loop.train "
                         "reset_every=...): the companion of a high --updates_per_step")
    ap.add_argument("--reset_what", default=None, metavar="actor,critics,alpha",
                    help="with --reset_every: the networks a reset starts over (default: all three; TD3 has no alpha)")
    ap.add_argument("--policy_stats", type=int, default=0, metavar="N",
                    help="SAC: at every evaluation put N ring rows to the policy and record vitals/replay_log_prob, vitals/policy_entropy "
                         "and vitals/log_std_mean (loop.train policy_stats=...)")
    ap.add_argument("--eval_one_launch", action="store_true",
                    help="with --device_env and a native env bundle: every evaluation window -- reset, one horizon of greedy steps -- is one "
                         "kernel launch (envs.greedy_returns one_launch=True) instead of one loop body per step")
    ap.add_argument("--q_bias", type=int, default=0, metavar="N",
                    help="with --device_env and a native env bundle: at every evaluation roll N fresh on-policy episodes in one launch and record "
                         "the normalised Q-bias of the critics, vitals/q_bias_mean, vitals/q_bias_std, vitals/q_bias_rows (loop.train q_bias=...)")
    ap.add_argument("--dry-run", action="store_true", help="enumerate and shard the jobs, start the workers, run nothing on a GPU")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--rank", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--world", type=int, default=1, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    try:
        plan = offline_plan(args)
        flags = mode_flags(args, plan or {})     # (policy_stats_plan is asked in there)
        if args.native_rollout:                  # every job of the sweep, before a worker starts
            native_rollout_plan(ENV_BUNDLES[args.env_bundle], args.device_env, bool(args.env_factory), args.offline_dataset is not None,
                                args.overlap_acting)
        if args.hindsight:                       # every job of the sweep, before a worker starts
            hindsight_plan(ENV_BUNDLES[args.env_bundle], bool(args.env_factory), args.offline_dataset is not None)
        # what loop.train would refuse is refused here, with no worker started (no env loop: offline_plan left no flag for it to mind)
        facts = {k: v for k, v in flags.items() if k not in ("hindsight", "eval_one_launch", "q_bias")}
        if plan is not None and plan.get("prior_fraction") is None and "reset_every" in flags:      # an offline plan: nothing but updates
            facts["num_updates"] = plan["num_updates"] if plan["num_updates"] is not None else job_config(args.algo, None, 0).num_timesteps
        for env_id in (ENV_BUNDLES[args.env_bundle] if args.hindsight else [None]):      # (with --hindsight: each job's own layout)
            cfg0 = job_config(args.algo, env_id, 0, batch_size=args.batch_size)
            train_keywords(cfg0, **facts, **(dict(hindsight=hindsight_keywords(env_id, cfg0.num_envs)) if args.hindsight else {}))
    except ValueError as ex:
        ap.error(str(ex))
    if args.worker:
        return _worker_main(args, plan or {}, flags)
    if plan is not None and plan["plain"]:
        print(f"launcher: --offline_dataset without --bc_alpha: plain {args.algo.upper()} on a fixed ring (no behaviour-cloning term; "
              "--algo td3 --bc_alpha 2.5 is TD3+BC)", file=sys.stderr, flush=True)
    # parent: touches no GPU (no torch import, no HIP call); one fresh child per GPU
    jobs = sweep_jobs(args.env_bundle, args.num_seeds)
    world = max(1, min(args.gpus, len(jobs)))
    base = [sys.executable, "-m", "sac_td3_cudagraphs_pytorch_amd.launcher", "--worker", "--world", str(world)] + \
           [x for x in (argv if argv is not None else sys.argv[1:]) if x != "--worker"]
    env = dict(os.environ)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    t0 = time.time()
    procs = [subprocess.Popen(base + ["--rank", str(r)], env=env, stdout=subprocess.PIPE, text=True) for r in range(world)]
    done, rc = [], 0
    for p in procs:
        out, _ = p.communicate()
        rc = rc or p.returncode
        for ln in out.splitlines():
            if ln.startswith("JOB "):
                done.append(json.loads(ln[4:]))
                print(ln, flush=True)
    dt = time.time() - t0
    steps = sum(j.get("gradient_steps", 0) for j in done)
    print("SWEEP " + json.dumps({"env_bundle": args.env_bundle, "num_seeds": args.num_seeds, "gpus": world, "jobs": len(done),
                                 "expected_jobs": len(jobs), "seconds": dt, "gradient_steps": steps,
                                 "aggregate_gradient_steps_per_s": steps / max(dt, 1e-9)}), flush=True)
    return rc if rc else (0 if len(done) == len(jobs) else 1)


if __name__ == "__main__":
    raise SystemExit(main())
