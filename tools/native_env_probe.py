#!/usr/bin/env python3
"""Measurements around the GPU-resident vector envs (envs.py, include/sactd3_env.h) -> profiles/native_env.json.  Nothing in the record
is a pass / fail bar of this tool; tests/test_gpu_native_env.py takes the learning tests' budget and bar from its "learning" entry.

    python tools/native_env_probe.py --oracle          # CPU, minutes: the oracle agent (oracle/sac_td3_ref.py) on envs.HostVecEnv, 3 seeds
                                                       # per task at the learning tests' budget -> "learning" (budget, per-seed returns, bar)
    python tools/native_env_probe.py                   # GPU: alternating child processes, 5 runs each, median and range ->
                                                       #   "train": loop.train(device_env=True) iterations/s on NativeVecEnv against
                                                       #            loop.SyntheticDeviceVecEnv at the same (o, a, num_envs), the same build
                                                       #   "step":  one vector step -- the launch alone (fixed buffers) and NativeVecEnv.step
                                                       #   "eval":  envs.greedy_returns on the GPU against loop.evaluate on the host twin
    python tools/native_env_probe.py --bench TREE      # GPU: this checkout's bench.py against the bench.py of another, built checkout
                                                       # (the parent commit's), alternating, 5 runs each -> "bench"
    python tools/native_env_probe.py --step TREE       # GPU: the "step" figures on this build and on TREE's, alternating -> "step_vs_parent"
    python tools/native_env_probe.py --digest TREE     # GPU: do the env kernels of this build and of TREE's compute the same bits?  One
                                                       # child process per side runs pendulum, cartpole and pointgoal at n = 1, 4, 257
                                                       # (one thread, a partial wavefront, a ragged second block) through step and
                                                       # step_records and hashes every output, then state() and episode_stats().  The
                                                       # tool asserts that each run met 2 bad actions, a truncation and, on the cart-pole,
                                                       # a termination.  -> "digest"; exit status 1 if any of the 18 pairs differs.  (Not
                                                       # a committed expectation: the digests of the trigonometric tasks belong to one
                                                       # ROCm's sinf / cosf.)
Each mode rewrites its own entries of the record and leaves the others."""
import argparse
import json
import os
import subprocess
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "native_env.json")
RUNS = 5
SEEDS = (0, 1, 2)
EPISODES = 16
# the digest's fixed inputs
DIGEST_KINDS = ("pendulum", "cartpole", "pointgoal")
DIGEST_NS = (1, 4, 257)
DIGEST_HORIZON, DIGEST_SEED, DIGEST_STEPS = 10, 11, 60
# the learning tests' budget: SAC, default hyper-parameters, 4 envs, one iteration per vector step
LEARNING = {"pendulum": dict(num_envs=4, learning_starts=1000, updates=3500, batch_size=256),
            "cartpole": dict(num_envs=4, learning_starts=1000, updates=2000, batch_size=256)}


def learning_cfg(kind, seed, budget=None):
    """the SimpleNamespace loop.train and Agent take: launcher.DEFAULTS["sac"] with the budget's entries; no evaluation inside the run"""
    from sac_td3_cudagraphs_pytorch_amd import launcher
    b = dict(budget or LEARNING[kind])
    steps = b["learning_starts"] + b["updates"] * b["num_envs"]
    return launcher.job_config("sac", kind, seed, num_envs=b["num_envs"], learning_starts=b["learning_starts"], batch_size=b["batch_size"],
                               num_timesteps=steps - 1, eval_every=10 ** 9, rb_capacity=1 << 15)


def merge(entries):
    rec = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            rec = json.load(f)
    rec.update(entries)
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


def spread(xs):
    xs = sorted(float(x) for x in xs)
    return {"median": float(np.median(xs)), "min": xs[0], "max": xs[-1], "runs": len(xs)}


# ---------------------------------------------------------------------------------------------------- the oracle on the host twin
class OracleAgent:
    """oracle/sac_td3_ref.py:RefAgent behind the surface loop.train and envs.greedy_returns use: a numpy ring, uniform draws"""

    def __init__(self, kind, cfg, seed):
        import torch
        from oracle.sac_td3_ref import Hps, RefAgent
        from sac_td3_cudagraphs_pytorch_amd import envs
        o, a, bound = envs.SPECS[envs.kind_of(kind)][:3]
        torch.manual_seed(seed)
        self.ref = RefAgent(o, a, [-bound] * a, [bound] * a, Hps.sac(batch_size=cfg.batch_size))
        self.ref.keep_trace = False
        self.rng = np.random.default_rng(seed)
        self.B, self.rows, self.cursor, self.cap = cfg.batch_size, 0, 0, cfg.rb_capacity
        self.cols = {"observations": np.zeros((self.cap, o), np.float32), "actions": np.zeros((self.cap, a), np.float32),
                     "rewards": np.zeros((self.cap, 1), np.float32), "next_observations": np.zeros((self.cap, o), np.float32),
                     "dones": np.zeros((self.cap, 1), bool)}
        self.rb = self
        self.timesteps_so_far = self.qnet_updates_so_far = self.actor_updates_so_far = 0
        self.engine = SimpleNamespace(read_metrics=lambda: {}, cfg=SimpleNamespace(max_envs=1 << 20))

    def extend(self, td):
        n = len(td["rewards"])
        at = (self.cursor + np.arange(n)) % self.cap
        for k, col in self.cols.items():
            col[at] = np.asarray(td[k]).reshape(n, -1)
        self.cursor, self.rows = (self.cursor + n) % self.cap, min(self.cap, self.rows + n)

    def predict(self, td, *, explore):
        return self.ref.predict(td["observations"], explore=explore)

    def iteration(self, i):
        at = self.rng.integers(0, self.rows, self.B)
        c = self.cols
        self.ref.iteration(self.ref.to_batch(c["observations"][at], c["actions"][at], c["rewards"][at], c["next_observations"][at], c["dones"][at]), i)
        self.qnet_updates_so_far += 1


def oracle_run(kind, seed):
    from sac_td3_cudagraphs_pytorch_amd import envs, loop
    cfg = learning_cfg(kind, seed)
    agent = OracleAgent(kind, cfg, seed)
    eval_env = envs.HostVecEnv(kind, EPISODES, seed=seed + 1000)
    before = envs.greedy_returns(eval_env, agent, EPISODES)["return"]
    t0 = time.time()
    loop.train(cfg, envs.HostVecEnv(kind, cfg.num_envs, seed=seed), agent)
    after = envs.greedy_returns(eval_env, agent, EPISODES)["return"]
    return {"seed": seed, "untrained": float(before), "trained": float(after), "updates": agent.qnet_updates_so_far, "seconds": time.time() - t0}


def oracle_mode():
    out = {"what": "oracle.sac_td3_ref.RefAgent (SAC, default hyper-parameters) trained by loop.train on envs.HostVecEnv; greedy return by "
                   f"envs.greedy_returns over {EPISODES} envs for one horizon, before and after.  bar = midpoint between the worst trained and "
                   "the best untrained seed; a task keeps its learning test only if every seed clears the bar by a quarter of that gap",
           "episodes": EPISODES, "eval_seed_offset": 1000, "tasks": {}}
    for kind in LEARNING:
        runs = [oracle_run(kind, s) for s in SEEDS]
        worst, best = min(r["trained"] for r in runs), max(r["untrained"] for r in runs)
        gap = worst - best
        out["tasks"][kind] = {"budget": LEARNING[kind], "seeds": runs, "worst_trained": worst, "best_untrained": best,
                              "bar": 0.5 * (worst + best), "margin_needed": 0.25 * gap,
                              "test_kept": bool(gap > 0 and all(r["trained"] - 0.5 * (worst + best) >= 0.25 * gap for r in runs))}
        print(kind, json.dumps(out["tasks"][kind]), flush=True)
    merge({"learning": out})


# ---------------------------------------------------------------------------------------------------- GPU children: one measurement each
def child_train(kind, which):
    import torch
    from sac_td3_cudagraphs_pytorch_amd import Agent, ReplayBuffer, envs, loop
    cfg = learning_cfg(kind, 0, dict(num_envs=4, learning_starts=1000, updates=3000, batch_size=256))
    o, a, bound = envs.SPECS[envs.kind_of(kind)][:3]
    dev = torch.device("cuda", 0)
    env = envs.NativeVecEnv(kind, cfg.num_envs, seed=0, device=dev) if which == "native" else \
        loop.SyntheticDeviceVecEnv(o, a, cfg.num_envs, horizon=200, term_at=6.0, bound=bound, device=dev)
    torch.manual_seed(0)
    agent = Agent({"ob_shape": (o,), "ac_shape": (a,)}, np.full(a, -bound, np.float32), np.full(a, bound, np.float32), dev, cfg,
                  ReplayBuffer(cfg.rb_capacity), seed=0)
    warm = learning_cfg(kind, 0, dict(num_envs=4, learning_starts=1000, updates=200, batch_size=256))
    loop.train(warm, env, agent, device_env=True)          # graphs instantiated, allocator warm; the counters go on from here
    agent.engine.sync()
    u0, t0 = agent.qnet_updates_so_far, time.perf_counter()
    cfg.num_timesteps += agent.timesteps_so_far
    loop.train(cfg, env, agent, device_env=True)
    agent.engine.sync()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"iterations_per_s": (agent.qnet_updates_so_far - u0) / dt, "iterations": agent.qnet_updates_so_far - u0}


def child_step(kind, n):
    import ctypes as C
    import torch
    from sac_td3_cudagraphs_pytorch_amd import _lib, envs
    env = envs.NativeVecEnv(kind, n, seed=0)
    obs, _ = env.reset()
    act = env.action_space.sample()
    out = _lib.CEnvOut(obs.data_ptr(), obs.stride(0), None, 0, None, 0, None, 0, None, 0, None, 0)
    st = env._stream()
    reps = 2000
    res = {}
    for name, body in (("launch_only", lambda: env._call("sactd3_env_step", act.data_ptr(), act.stride(0), C.byref(out), st)),
                       ("env_step", lambda: env.step(act))):
        for _ in range(200):
            body()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(reps):
            body()
        e1.record()
        host = time.perf_counter() - t0
        torch.cuda.synchronize()
        res[name] = {"device_us_per_step": 1e3 * e0.elapsed_time(e1) / reps, "host_issue_us_per_step": 1e6 * host / reps}
    return res


def child_eval(kind, which):
    import torch
    from sac_td3_cudagraphs_pytorch_amd import Agent, ReplayBuffer, envs, loop
    cfg = learning_cfg(kind, 0)
    cfg.num_envs = EPISODES                                  # (max_envs of the engine: one predict call per step)
    o, a, bound = envs.SPECS[envs.kind_of(kind)][:3]
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    agent = Agent({"ob_shape": (o,), "ac_shape": (a,)}, np.full(a, -bound, np.float32), np.full(a, bound, np.float32), dev, cfg,
                  ReplayBuffer(1024), seed=0)
    if which == "native":
        env = envs.NativeVecEnv(kind, EPISODES, seed=5, device=dev)
        envs.greedy_returns(env, agent, EPISODES)
        t0 = time.perf_counter()
        got = envs.greedy_returns(env, agent, EPISODES)
    else:
        ev = SimpleNamespace(seed=5, num_episodes=EPISODES)
        env = envs.HostVecEnv(kind, 1, seed=5)
        loop.evaluate(SimpleNamespace(seed=5, num_episodes=2), env, agent)
        t0 = time.perf_counter()
        got = loop.evaluate(ev, env, agent)
    return {"seconds": time.perf_counter() - t0, "episodes": EPISODES, "return": float(got["return"])}


def child_bench(tree):
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "2000", "--warmup", "200"], cwd=tree,
                         capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit(out.stdout[-2000:] + out.stderr[-2000:])
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


def digest_actions(kind_index, n, ac_dim, bound):
    """[DIGEST_STEPS, n, ac_dim] float32, made on the host: 30 steps of large pushes with the sign of the env's parity (the cart-pole
    falls, the point mass runs into its wall), 30 small ones; one NaN and one +inf component"""
    rng = np.random.default_rng([n, kind_index])
    half = DIGEST_STEPS // 2
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[None, :, None]
    act = np.concatenate([sign * rng.uniform(0.5, 1.5, (half, n, ac_dim)) * bound, rng.uniform(-0.2, 0.2, (half, n, ac_dim)) * bound]).astype(np.float32)
    act[3, 0, 0] = np.nan
    act[5, n - 1, ac_dim - 1] = np.inf
    return act


def child_digest():
    """every (kind, n, form) of the digest on the package this process imported: -> {"library", "runs": {"kind-n-form": {"sha256",
    "terminations", "truncations", "bad_actions"}}}"""
    import hashlib
    import torch
    import sac_td3_cudagraphs_pytorch_amd as pkg
    from sac_td3_cudagraphs_pytorch_amd import envs
    dev = torch.device("cuda", 0)
    runs = {}
    for kind in DIGEST_KINDS:
        k = envs.kind_of(kind)
        o, a, bound = envs.SPECS[k][:3]
        eng = pkg.Engine(pkg.Config(ob_dim=o, ac_dim=a, batch_size=64, rb_capacity=256, max_envs=4, seed=0), [-bound] * a, [bound] * a)
        layout = eng.rb_layout()
        done_at = layout["next_obs_offset"] + layout["next_obs_width"] + 1
        for n in DIGEST_NS:
            actions = torch.as_tensor(digest_actions(k, n, a, bound), device=dev)
            for form in ("step", "step_records"):
                env = envs.NativeVecEnv(kind, n, seed=DIGEST_SEED, device=dev, horizon=DIGEST_HORIZON)
                obs, _ = env.reset()
                rec = torch.zeros((n, layout["record_floats"]), device=dev)
                h, term, trunc = hashlib.sha256(), 0, 0
                for t in range(DIGEST_STEPS):
                    if form == "step":
                        obs, rew, terminated, truncated, infos = env.step(actions[t])
                        outs = (obs, infos["final_observation"], rew, terminated, truncated, infos["_final_observation"])
                        term, trunc = term + int(terminated.sum()), trunc + int(truncated.sum())
                    else:
                        env.step_records(actions[t], layout, rec, obs)
                        outs = (rec, obs)
                        term += int((rec[:, done_at] != 0).sum())
                    for x in outs:
                        h.update(x.cpu().numpy().tobytes())
                state, stats = env.state(), env.episode_stats()
                for book in (state, stats):
                    for key in sorted(book):
                        h.update(np.asarray(book[key]).tobytes())
                if form == "step_records":
                    trunc = stats["episodes"] - term
                runs[f"{kind}-{n}-{form}"] = {"sha256": h.hexdigest(), "terminations": term, "truncations": trunc, "bad_actions": stats["bad_actions"]}
                env.close()
        eng.close()
    return {"library": os.path.realpath(pkg.library_path()), "runs": runs}


CHILDREN = {"train": child_train, "step": child_step, "eval": child_eval, "digest": child_digest}


def run_child(*argv, timeout=300, tree=ROOT):
    """a fresh process per measurement, importing the package of `tree`; -> its JSON.  A child that fails ends the whole probe: nothing
    more is started on the GPU."""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", tree, "--child", *map(str, argv)], capture_output=True, text=True,
                         timeout=timeout)
    if out.returncode != 0:
        raise SystemExit(f"child {argv} in {tree} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def gpu_mode(runs):
    rec = {"train": {}, "step": {}, "eval": {}}
    for kind in LEARNING:
        got = {"native": [], "synthetic": []}
        for _ in range(runs):
            for which in got:                                # alternating: native, synthetic, native, ...
                got[which].append(run_child("train", kind, which)["iterations_per_s"])
        rec["train"][kind] = {"what": "loop.train(device_env=True), SAC, 4 envs, B 256, 3000 iterations behind a 200-iteration warm-up: iterations/s",
                              **{k: spread(v) for k, v in got.items()}}
        print("train", kind, json.dumps(rec["train"][kind]), flush=True)
        ev = {"native": [], "host": []}
        for _ in range(runs):
            for which in ev:
                ev[which].append(run_child("eval", kind, which)["seconds"])
        rec["eval"][kind] = {"what": f"{EPISODES} greedy episodes: envs.greedy_returns on the GPU (one host wait) against loop.evaluate on a "
                                     "one-env HostVecEnv (a predict round trip per step): seconds", **{k: spread(v) for k, v in ev.items()}}
        print("eval", kind, json.dumps(rec["eval"][kind]), flush=True)
        for n in (4, 4096):
            runs_n = [run_child("step", kind, n) for _ in range(runs)]
            rec["step"][f"{kind}-{n}"] = {f"{name}.{fig}": spread([r[name][fig] for r in runs_n]) for name in ("launch_only", "env_step")
                                          for fig in ("device_us_per_step", "host_issue_us_per_step")}
            print("step", kind, n, json.dumps(rec["step"][f"{kind}-{n}"]), flush=True)
    merge(rec)


def commit_of(tree):
    """the commit a tree is a checkout of: git's word where the tree is a repository of its own, else its COMMIT_ID file, else None"""
    top = subprocess.run(["git", "-C", tree, "rev-parse", "--show-toplevel", "HEAD"], capture_output=True, text=True)
    if top.returncode == 0 and os.path.realpath(top.stdout.split()[0]) == os.path.realpath(tree):
        dirty = subprocess.run(["git", "-C", tree, "status", "--porcelain", "-uno"], capture_output=True, text=True).stdout.strip()
        return top.stdout.split()[1] + (" + uncommitted changes" if dirty else "")
    if os.path.exists(os.path.join(tree, "COMMIT_ID")):
        with open(os.path.join(tree, "COMMIT_ID")) as f:
            return f.read().strip()
    return None


def digest_mode(parent):
    """bit comparison of the env kernels against another build: one child per side, each on its own package and library"""
    sides = {"this": run_child("digest", tree=ROOT, timeout=600), "parent": run_child("digest", tree=parent, timeout=600)}
    for side, tree in (("this", ROOT), ("parent", parent)):
        assert os.path.dirname(sides[side]["library"]) == os.path.realpath(os.path.join(tree, "sac-td3-cudagraphs-pytorch_amd")), (side, sides[side]["library"])
        for name, run in sides[side]["runs"].items():      # a digest of a run that never resets would prove little
            assert run["bad_actions"] == 2 and run["truncations"] >= 1, (side, name, run)
            assert run["terminations"] >= 1 or not name.startswith("cartpole"), (side, name, run)
    names = sorted(sides["this"]["runs"])
    assert names == sorted(sides["parent"]["runs"]) and len(names) == len(DIGEST_KINDS) * len(DIGEST_NS) * 2
    differ = [name for name in names if sides["this"]["runs"][name]["sha256"] != sides["parent"]["runs"][name]["sha256"]]
    merge({"digest": {"what": f"SHA-256 over every output of {DIGEST_STEPS} steps (step: obs, final_obs, reward, the three flags; step_records: the "
                              f"record slab, obs), then state() and episode_stats(): horizon {DIGEST_HORIZON}, env seed {DIGEST_SEED}, host-made "
                              "actions with a NaN and a +inf, on this build and on the parent commit's, one process each",
                      "commits": {"this": commit_of(ROOT), "parent": commit_of(parent)}, "equal": not differ, "differ": differ,
                      **{side: got["runs"] for side, got in sides.items()}}})
    print(json.dumps({"pairs": len(names), "equal": not differ, "differ": differ}), flush=True)
    return 1 if differ else 0


def step_mode(parent, runs):
    """the "step" figures of this build and of the parent commit's, alternating"""
    rec = {}
    for kind in DIGEST_KINDS:
        for n in (4, 4096):
            got = {"this": [], "parent": []}
            for _ in range(runs):
                for side, tree in (("this", ROOT), ("parent", parent)):
                    got[side].append(run_child("step", kind, n, tree=tree))
            rec[f"{kind}-{n}"] = {side: {f"{name}.{fig}": spread([r[name][fig] for r in rs]) for name in ("launch_only", "env_step")
                                         for fig in ("device_us_per_step", "host_issue_us_per_step")} for side, rs in got.items()}
            print("step", kind, n, json.dumps(rec[f"{kind}-{n}"]), flush=True)
    merge({"step_vs_parent": {"what": "the \"step\" figures (2000 steps behind 200: the launch alone into fixed buffers, and NativeVecEnv.step) on "
                                      "this build and on the parent commit's, alternating fresh processes", **rec}})


def bench_mode(other, runs):
    got = {"this": [], "other": []}
    for _ in range(runs):
        got["this"].append(child_bench(ROOT))
        got["other"].append(child_bench(other))
    keys = [k for k in ("value", "ms_per_step") if k in got["this"][0]]
    merge({"bench": {"what": "bench.py --gpus 1 --steps 2000 --warmup 200 of this checkout and of the parent commit's, alternating processes",
                     **{side: {k: spread([r[k] for r in rs]) for k in keys} for side, rs in got.items()}}})
    print(json.dumps({side: {k: spread([r[k] for r in rs])["median"] for k in keys} for side, rs in got.items()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--bench", default=None, metavar="TREE")
    ap.add_argument("--digest", default=None, metavar="TREE")
    ap.add_argument("--step", default=None, metavar="TREE")
    ap.add_argument("--runs", type=int, default=RUNS)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--child", nargs="+", default=None)
    args = ap.parse_args()
    if args.child:
        sys.path.insert(0, os.path.abspath(args.tree))
        kind_args = [int(x) if x.isdigit() else x for x in args.child[1:]]
        print("RESULT " + json.dumps(CHILDREN[args.child[0]](*kind_args)), flush=True)
    elif args.oracle:
        oracle_mode()
    elif args.digest:
        return digest_mode(os.path.abspath(args.digest))
    elif args.step:
        step_mode(os.path.abspath(args.step), args.runs)
    elif args.bench:
        bench_mode(os.path.abspath(args.bench), args.runs)
    else:
        gpu_mode(args.runs)
    return 0


if __name__ == "__main__":
    sys.exit(main())
