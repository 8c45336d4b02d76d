#!/usr/bin/env python3
"""SHA-256 of what the kernels built on csrc/hidden_tile.h write, for comparing two builds of the library bit for bit.

    python tools/hidden_tile_bits.py [--tree CHECKOUT]      # CHECKOUT: a built checkout whose package is imported (default: this one)

One fresh process, fixed seeds, small shapes (K = 14: pad words; n = 17: a partial second tile; 16 * 128 + 5 rows: a workgroup of the scan
walks two tiles): a dormant scan, a feature rank with spectrum and gram, action_values for N = 16 / 32 / 64 from both sources with
data actions, a 12-step sampled evaluation and an exploring collect on the pendulum.  Prints one JSON object {output: digest}.  Run it
on the parent commit's build and on this one on the same machine and compare: no sum in these kernels is reordered by a refactor, so a
digest that differs is a changed operation order.  Nothing here is a golden: the digests depend on the ROCm libm in use."""
import argparse
import hashlib
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def digest(x):
    import torch
    if torch.is_tensor(x):
        x = x.detach().cpu().contiguous().numpy()
    if hasattr(x, "tobytes"):
        return hashlib.sha256(x.tobytes()).hexdigest()
    if isinstance(x, dict):
        x = {str(k): digest(v) for k, v in x.items()}
    elif isinstance(x, (list, tuple)):
        x = [digest(v) for v in x]
    return hashlib.sha256(json.dumps(x, sort_keys=True).encode()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    sys.path.insert(0, os.path.abspath(ap.parse_args().tree))
    import numpy as np
    import torch
    import sac_td3_cudagraphs_pytorch_amd as P
    from sac_td3_cudagraphs_pytorch_amd import _lib, envs, loop
    from oracle.sac_td3_ref import Hps
    out, dev, cap = {}, torch.device("cuda", 0), 4096

    def engine(o, a, ln=True, max_envs=4):
        eng = P.Engine(P.Config.from_hps(Hps.sac(layer_norm=ln, batch_size=64), o, a, rb_capacity=cap, max_envs=max_envs, seed=7), [-1.0] * a, [1.0] * a)
        eng.init_params(_lib.INIT_ACTOR | _lib.INIT_CRITICS, epoch=0)
        return eng

    def put(name, got):
        for k, v in sorted(got.items()):
            if v is not None:
                out[f"{name}.{k}"] = digest(v)

    # the ring front end: the scan and the feature rank
    for (o, a), ln in (((11, 3), True), ((70, 2), False)):
        eng, g = engine(o, a, ln), torch.Generator().manual_seed(8)
        obs, act = torch.randn(cap, o, generator=g), torch.rand(cap, a, generator=g) * 2 - 1
        eng.rb_extend(obs.numpy(), act.numpy(), np.zeros(cap, np.float32), obs.numpy(), np.zeros(cap, bool))
        for n in (17, 16 * 128 + 5):
            idx = torch.randint(0, cap, (n,), generator=g).to(dev)
            put(f"dormant_scan[{o},{a},ln={int(ln)},n={n}]", eng.dormant_scan(idx, tau=0.025, scores=True))
            put(f"feature_rank[{o},{a},ln={int(ln)},n={n}]", eng.feature_rank(idx, spectrum=True, gram=True))
        eng.close()
    # candidate scoring
    o, a = 11, 3
    eng, g = engine(o, a), torch.Generator().manual_seed(9)
    obs, act = torch.randn(21, o, generator=g).to(dev), (torch.rand(21, a, generator=g) * 2 - 1).to(dev)
    for N in (16, 32, 64):
        for source in ("policy", "uniform"):
            put(f"action_values[N={N},{source}]", eng.action_values(obs, act, candidates=N, source=source, dump=True))
    eng.close()
    # the actor pass: evaluation and collect on the pendulum
    o, a, _ = envs.SPECS[envs.kind_of("pendulum")][:3]
    eng = engine(o, a, max_envs=32)
    rb = P.ReplayBuffer(cap)
    rb._bind(eng)
    agent = SimpleNamespace(engine=eng, rb=rb, timesteps_so_far=0)
    env = envs.NativeVecEnv("pendulum", 17, seed=5, device=dev, horizon=5)
    put("eval_rollout[pendulum,T=12,sample]", envs.policy_rollout(env, agent, steps=12, mode="sample", seed=5, soft=True, trajectories=True))
    ro = loop.NativeRollout(env, agent, 5, 10 ** 9, 1)
    slab, eps = ro.collect(12, _lib.ROLLOUT_EXPLORE, eps=True)
    put("collect[pendulum,T=12,explore]", {"records": slab, "eps": eps, "obs": ro.obs, "actions": ro.actions})
    torch.cuda.synchronize()
    ro.close()
    env.close()
    eng.close()
    print("DIGESTS " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
