"""TD3+BC (Fujimoto & Gu 2021) restated with torch autograd, for tests/test_td3bc_host.py and tests/test_gpu_td3bc.py.

The engine's form (include/sactd3.h, sactd3_set_bc), with pi = actor(s), q_b = Q1(s_b, pi_b) through online critic 1 as a constant,
a_b the stored action, A = ac_dim:

    lambda   = bc_alpha / max(mean_b |q_b|, 1e-8)                 (a constant of the backward pass)
    bc       = (1 / (B A)) sum_b sum_j (pi_bj - a_bj)^2
    L_actor  = -lambda mean_b q_b + bc_weight bc
    dL/dpi_bj = lambda (-1/B) dq_b/da_j + bc_weight 2 (pi_bj - a_bj) / (B A)

`actor_loss` is that loss for tensors of any dtype; `actor_update64` is the whole update_actor in float64 (autograd through copies of
the oracle's modules, clip_grad_norm_, torch.optim.Adam); `RefAgentBC` is the oracle's agent with that loss in place of TD3's, and
`offline_direction` the small offline experiment of the "it does what it is for" test on that agent, on the CPU.
"""
import copy

import numpy as np
import torch

from oracle.sac_td3_ref import Hps, RefAgent

BC_FLOOR = 1e-8


def actor_loss(pi, q, act, bc_alpha, bc_weight=1.0):
    """(L_actor, lambda, bc) -- lambda and bc detached"""
    lam = bc_alpha / torch.clamp(q.detach().abs().mean(), min=BC_FLOOR)
    bc = ((pi - act) ** 2).mean()
    return -lam * q.mean() + bc_weight * bc, lam.detach(), bc.detach()


def closed_form_dpi(dq_da, pi, act, lam, bc_weight=1.0):
    """dL_actor / dpi from dq_b / da (the gradient of each row's q with respect to its own action)"""
    B, A = pi.shape
    return lam * (-1.0 / B) * dq_da + bc_weight * 2.0 * (pi - act) / (B * A)


def actor_update64(actor, q1, obs, act, *, bc_alpha, bc_weight=1.0, lr, clip_norm=0.0):
    """One TD3+BC update_actor in float64 on copies of `actor` (the oracle's DetPolicy) and `q1` (its QNet), from Adam step 0.
    -> dict: loss, lam, bc (floats); pi, q, dpi (= dL/dpi), dq_da; grads {parameter name: gradient BEFORE clipping}; coef (the clip
    coefficient); actor (the stepped float64 copy)."""
    actor, q1 = copy.deepcopy(actor).double(), copy.deepcopy(q1).double()
    for p in q1.parameters():
        p.requires_grad_(False)
    obs, act = torch.as_tensor(obs).double(), torch.as_tensor(act).double()
    opt = torch.optim.Adam(actor.parameters(), lr=float(np.float32(lr)))
    pi = actor(obs)
    pi.retain_grad()
    q = q1(obs, pi).view(-1)
    loss, lam, bc = actor_loss(pi, q, act, bc_alpha, bc_weight)
    loss.backward()
    grads = {k: p.grad.clone() for k, p in actor.named_parameters()}
    a_leaf = pi.detach().clone().requires_grad_(True)
    dq_da, = torch.autograd.grad(q1(obs, a_leaf).sum(), a_leaf)
    coef = 1.0
    if clip_norm > 0:
        total = torch.nn.utils.clip_grad_norm_(actor.parameters(), clip_norm)
        coef = min(1.0, clip_norm / (float(total) + 1e-6))
    opt.step()
    return dict(loss=float(loss.detach()), lam=float(lam), bc=float(bc), pi=pi.detach(), q=q.detach(), dpi=pi.grad.clone(), dq_da=dq_da,
                grads=grads, coef=coef, actor=actor)


class RefAgentBC(RefAgent):
    """oracle.sac_td3_ref.RefAgent (TD3) whose update_actor minimises the TD3+BC loss when bc_alpha > 0"""

    def __init__(self, *args, bc_alpha=0.0, bc_weight=1.0, **kw):
        super().__init__(*args, **kw)
        self.bc_alpha, self.bc_weight = float(bc_alpha), float(bc_weight)

    def update_actor(self, b, eps=None, eps_alpha=None):
        if not self.bc_alpha > 0:
            return super().update_actor(b, eps, eps_alpha)
        assert self.hps.prefer_td3_over_sac
        self.actor_optimizer.zero_grad()
        pi = self.actor(b.observations)
        for p in self.qnets.parameters():
            p.requires_grad_(False)
        q = self.qnets[0](b.observations, pi).view(-1)
        for p in self.qnets.parameters():
            p.requires_grad_(True)
        loss, lam, bc = actor_loss(pi, q, b.actions, self.bc_alpha, self.bc_weight)
        loss.backward()
        if self.hps.clip_norm > 0:
            torch.nn.utils.clip_grad_norm_(self.actor.parameters(), self.hps.clip_norm)
        self.actor_optimizer.step()
        return {"loss/actor_loss": loss.detach(), "loss/bc_loss": bc, "vitals/bc_lambda": lam}


# ---- the offline experiment of "it does what it is for": a ring of rows whose actions are a fixed linear-tanh function of the
# observations and whose reward grows with the action's magnitude -- Q then pulls an unconstrained actor towards the bounds, away
# from the data, and the BC term pulls it back onto the data.
DIRECTION_SEED = 3
DIRECTION = dict(o=17, a=6, bound=1.0, rows=4096, B=256, iters=300, bc_alpha=2.5)


def direction_dataset(seed=DIRECTION_SEED, rows=DIRECTION["rows"], o=DIRECTION["o"], a=DIRECTION["a"], bound=DIRECTION["bound"]):
    g = torch.Generator().manual_seed(1000 + seed)
    obs, nobs = torch.randn(rows, o, generator=g), torch.randn(rows, o, generator=g)
    W, c = torch.randn(o, a, generator=g) / o ** 0.5, 0.1 * torch.randn(a, generator=g)
    act = torch.tanh(obs @ W + c) * bound
    rew = (act ** 2).mean(1) + 0.1 * torch.randn(rows, generator=g)
    done = torch.rand(rows, generator=g) < 0.01
    return obs, act, rew, nobs, done


def dataset_bc(predict, obs, act):
    """(1 / (n A)) sum (pi(s) - a)^2 over the whole dataset, on the host"""
    pi = np.asarray(predict(obs), np.float64)
    return float(((pi - np.asarray(act, np.float64)) ** 2).mean())


def offline_direction(bc_alpha, seed=DIRECTION_SEED, iters=DIRECTION["iters"]):
    """`iters` offline iterations of the oracle's TD3 (+BC) on direction_dataset from `seed`, uniform batches.
    -> (dataset_bc before, dataset_bc after, loss/bc_loss of the first iteration or None, of the last or None)"""
    d = DIRECTION
    obs, act, rew, nobs, done = direction_dataset(seed)
    torch.manual_seed(seed)
    ag = RefAgentBC(d["o"], d["a"], [-d["bound"]] * d["a"], [d["bound"]] * d["a"], Hps.td3(batch_size=d["B"]), bc_alpha=bc_alpha)
    ag.keep_trace = False
    predict = lambda x: ag.predict(x, explore=False)
    before = dataset_bc(predict, obs, act)
    g = torch.Generator().manual_seed(2000 + seed)
    first = last = None
    for i in range(iters):
        idx = torch.randint(0, obs.shape[0], (d["B"],), generator=g)
        out = ag.iteration(ag.to_batch(obs[idx], act[idx], rew[idx], nobs[idx], done[idx]), i)
        if "loss/bc_loss" in out:
            last = float(out["loss/bc_loss"])
            first = last if first is None else first
    return before, dataset_bc(predict, obs, act), first, last
