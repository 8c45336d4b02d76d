"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  A plain restatement of sactd3_action_gradient_device (include/sactd3_action_gradient.h): the
twin critics rebuilt from get_params in torch at a dtype of the caller's choice (float64: the reference; float32 on the CPU: the
yardstick of the tolerance), Q by the forward pass and every gradient by autograd -- no hand-written backward.  Used by
tests/test_gpu_action_gradient.py."""
import numpy as np
import torch

from tests import init_model


def critic(flat, K, ln, x, dtype):
    """one critic on x [n, K] -> (Q [n], the smallest |pre-ReLU value| per row [n])"""
    p = {(kind, layer): torch.as_tensor(np.array(v), dtype=dtype) for kind, layer, v in init_model.split(flat, K, 1, ln)}
    h, margin = x, None
    for layer in (0, 1):
        z = h @ p[("weight", layer)].T + p[("bias", layer)]
        if ln:
            d = z - z.mean(1, keepdim=True)
            z = d / torch.sqrt((d * d).mean(1, keepdim=True) + 1e-5) * p[("ln_weight", layer)] + p[("ln_bias", layer)]
        m = z.detach().abs().min(1).values
        margin = m if margin is None else torch.minimum(margin, m)
        h = torch.relu(z)
    return (h @ p[("weight", 2)].T + p[("bias", 2)])[:, 0], margin


def at(critics, o, a, ln, obs, act, dtype):
    """Q1, Q2 and their gradients at (obs, act) -> q [n, 2], grad [2, n, a], grad_obs [2, n, o], margin [n] (torch, `dtype`)"""
    obs, act = obs.clone().requires_grad_(True), act.clone().requires_grad_(True)
    q, ga, go, margin = [], [], [], None
    for flat in np.asarray(critics).reshape(2, -1):
        qk, m = critic(flat, o + a, ln, torch.cat([obs, act], 1), dtype)
        gs, gact = torch.autograd.grad(qk.sum(), (obs, act))
        q.append(qk.detach()); ga.append(gact); go.append(gs)
        margin = m if margin is None else torch.minimum(margin, m)
    return torch.stack(q, 1), torch.stack(ga), torch.stack(go), margin


def action_gradient(critics, o, a, ln, obs, act, lo, hi, steps, lr, dtype):
    """`critics`: the flat pair (get_params); obs [n, o], act [n, a]; lo / hi: the action bounds [a].  -> float64 numpy: q_start [n, 2],
    grad [2, n, a], grad_obs [2, n, o], refined [n, a], q_end [n, 2], summary [n, 8] (columns 0 - 5; 6 and 7 zeros) and `margin` [n]: the
    kink margin -- the smallest |pre-ReLU value| over both layers and critics at every action visited and, where a step was decided,
    |Q1 - Q2| there"""
    t = lambda v: torch.as_tensor(np.asarray(v), dtype=dtype)
    obs, act, lo, hi = t(obs), t(act), t(lo), t(hi)
    sc = (hi - lo) / 2
    q0, g0, go, margin = at(critics, o, a, ln, obs, act, dtype)
    q, g, cur = q0, g0, act
    for _ in range(int(steps)):
        margin = torch.minimum(margin, (q[:, 0] - q[:, 1]).abs())
        gu = torch.where((q[:, 0] <= q[:, 1])[:, None], g[0], g[1]) * sc
        nrm = torch.sqrt((gu * gu).sum(1, keepdim=True))
        cur = torch.minimum(torch.maximum(cur + (lr * gu / nrm.clamp_min(1e-8)) * sc, lo), hi)
        q, g, _, m = at(critics, o, a, ln, obs, cur, dtype)
        margin = torch.minimum(margin, m)
    n1, n2 = (torch.sqrt((g0[k] * g0[k]).sum(1)) for k in (0, 1))
    cos = torch.where((n1 == 0) | (n2 == 0), torch.zeros_like(n1), (g0[0] * g0[1]).sum(1) / (n1 * n2))
    zero = torch.zeros_like(n1)
    summary = torch.stack([q0.min(1).values, q.min(1).values, n1, n2, cos, torch.sqrt((((cur - act) / sc) ** 2).sum(1)), zero, zero], 1)
    out = {"q_start": q0, "grad": g0, "grad_obs": go, "refined": cur, "q_end": q, "summary": summary, "margin": margin}
    return {k: v.double().numpy() for k, v in out.items()}
