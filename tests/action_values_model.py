"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  A plain restatement of sactd3_action_values_device (include/sactd3_action_values.h) in
torch at a dtype of the caller's choice (float64: the reference; float32 on the CPU: the yardstick of the tolerance).  Used by
tests/test_gpu_action_values.py."""
import numpy as np
import torch

from tests import init_model

LOG_SQRT_2PI = 0.9189385332046727


def mlp(flat, K, nh, ln, x, dtype):
    """one net's output [n, nh] on x [n, K]: two hidden layers relu(LN(W x + b)) -- LN two-pass, eps inside the root, the identity
    without layer_norm -- and the linear head"""
    p = {(kind, layer): torch.as_tensor(np.array(v), dtype=dtype) for kind, layer, v in init_model.split(flat, K, nh, ln)}
    h = x
    for layer in (0, 1):
        z = h @ p[("weight", layer)].T + p[("bias", layer)]
        if ln:
            d = z - z.mean(1, keepdim=True)
            z = d / torch.sqrt((d * d).mean(1, keepdim=True) + 1e-5) * p[("ln_weight", layer)] + p[("ln_bias", layer)]
        h = torch.relu(z)
    return h @ p[("weight", 2)].T + p[("bias", 2)]


def action_values(params, o, a, td3, ln, obs, eps, source, sigma, tau, alpha, lo, hi, actions, dtype):
    """`params`: {"actor": flat, "critics": flat} (get_params); obs [n, o], eps [n, N, a], actions [n, a] or None; lo / hi: the action
    bounds [a].  -> {"cand" [n, N, a], "cand_logp" [n, N], "cand_q" [n, N, 2], "summary" [n, 8], "m" [n, N]} as float64 numpy,
    computed in `dtype`"""
    t = lambda v: torch.as_tensor(np.asarray(v), dtype=dtype)
    obs, eps, lo, hi = t(obs), t(eps), t(lo), t(hi)
    n, N, _ = eps.shape
    sc, bi = (hi - lo) / 2, (hi + lo) / 2
    (_, _, nh, actor), (_, K, _, q1), (_, _, _, q2) = init_model.nets_of(params, o, a, td3)
    logp = torch.zeros(n, N, dtype=dtype)
    if source == "uniform":
        cand = lo + eps * (hi - lo)
        logp = logp - torch.log(hi - lo).sum()
    else:
        u = mlp(actor, o, nh, ln, obs, dtype)[:, None, :]
        if td3:
            cand = torch.minimum(torch.maximum(torch.tanh(u) * sc + bi + eps * sigma * sc, lo), hi)
        else:
            mean, log_std = u[..., :a], -5.0 + 3.5 * (torch.tanh(u[..., a:]) + 1.0)
            sd = torch.exp(log_std)
            x = mean + eps * sd
            y, dx = torch.tanh(x), x - mean      # (the header's formula: the density of x as it was rounded, not of eps)
            cand = y * sc + bi
            logp = (-(dx * dx) / (2 * sd * sd) - torch.log(sd) - LOG_SQRT_2PI - torch.log(sc * (1 - y * y) + 1e-6)).sum(-1)
    sa = torch.cat([obs[:, None, :].expand(n, N, o), cand], -1).reshape(n * N, K)
    q = torch.stack([mlp(f, K, 1, ln, sa, dtype).reshape(n, N) for f in (q1, q2)], -1)
    m = q.min(-1).values
    q_max, q_mean = m.max(1).values, m.mean(1)
    soft = (m - alpha * logp).mean(1) if (source == "policy" and not td3) else q_mean
    if actions is None:
        q_data = torch.full((n,), float("nan"), dtype=dtype)
    else:
        sd_ = torch.cat([obs, t(actions)], -1)
        q_data = torch.minimum(mlp(q1, K, 1, ln, sd_, dtype)[:, 0], mlp(q2, K, 1, ln, sd_, dtype)[:, 0])
    summary = torch.stack([q_max, q_mean, q_max + tau * torch.log(torch.exp((m - q_max[:, None]) / tau).mean(1)),
                           torch.sqrt(((m - q_mean[:, None]) ** 2).mean(1)), soft, q_data, logp.mean(1),
                           torch.isfinite(m).sum(1).to(dtype)], 1)
    out = {"cand": cand.expand(n, N, a), "cand_logp": logp, "cand_q": q, "summary": summary, "m": m}
    return {k: v.double().numpy() for k, v in out.items()}
