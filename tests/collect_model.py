"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  The checker of the collected rollout segment (include/sactd3_rollout_collect.h; device code:
csrc/collect_kernels.h).  Checked on the CPU by tests/test_collect_model.py; used by tests/test_gpu_collect.py.

What a call leaves -- the slab [T n, record_floats], time-major, and the draws eps [T, n, a] -- is checked against models none of which
takes a tolerance from an observed error and none of which leaves an element out:

  the actor    per record (t, i), float64 from the record's OWN s: tests/eval_model.py forward64 with its a-priori bound, then as intervals
               EXPLOIT      bounds.td3_policy: tanh(u) scale + bias (SAC: of the mean)
               EXPLORE SAC  bounds.squash with the recorded draw: tanh(mean + e std) scale + bias
               EXPLORE TD3  td3_policy's interval, + e fl32(scale noise_std): one rounding for the product, one for the sum
               the record's a must lie inside
  the draws    float64 Philox normals (tests/noise_model.py: bound) at the counter words (collect_ctr, t, 0x900, element >> 2), element =
               i ac_dim + j, keyed by the engine's seed; RANDOM and EXPLOIT: eps is +0 everywhere
  RANDOM       a is, bit for bit, the env's own draw number draws[i] + t (envs.random_actions)
  the slab     rebuilt from the recorded actions by stepping a twin from the state in front of the call and packing every step with
               envs.pack_records under the stored-next rule, row t n + i: the same bits, pads included.  On the CPU the twin is
               envs.HostVecEnv (rebuild_on_host); on the GPU the test steps a twin NativeVecEnv and hands the rebuilt slab in.
  the env      the state the call leaves (draws included) is the twin's

emulate32 is the whole call in numpy float32 on the host twin; the checker must accept it and must refuse each of DEFECTS.  This is not
a test module, so pytest does not rewrite its asserts: every assert here carries its own message."""
import numpy as np

from tests import bounds, eval_model, noise_model

STREAM_COLLECT = 0x900
RANDOM, EXPLORE, EXPLOIT = 0, 1, 2          # SACTD3_ROLLOUT_*
F = np.float32


def layout_for(o, a):
    """(record_floats, next_obs_offset, next_obs_width) of the engine for (ob_dim, ac_dim): [s | a] and s' padded to 4 floats, the record to 16"""
    off, width = -(-(o + a) // 4) * 4, -(-o // 4) * 4
    return -(-(off + width + 2) // 16) * 16, off, width


def fields(slab, layout, o, a):
    """a slab on the host -> its fields and its pads"""
    _, off, width = layout
    tail = off + width
    pads = np.concatenate([slab[:, o + a:off], slab[:, off + o:tail], slab[:, tail + 2:]], 1)
    return {"s": slab[:, :o], "a": slab[:, o:o + a], "next": slab[:, off:off + o], "r": slab[:, tail], "d": slab[:, tail + 1], "pads": pads}


# ---------------------------------------------------------------------------------------------------- the draws
def _uniforms(seed, ctr, T, n, a, stream=STREAM_COLLECT, with_t=True):
    t = np.repeat(np.arange(T, dtype=np.uint64), n * a)
    el = np.tile(np.arange(n * a, dtype=np.uint64), T)
    r = noise_model.replay_ref.philox4x32_10(np.full(T * n * a, ctr & 0xFFFFFFFF), t if with_t else np.zeros_like(t), stream, el >> np.uint64(2),
                                 seed & 0xFFFFFFFF, seed >> 32)
    k = (el & np.uint64(3)).astype(np.int64)
    return noise_model.u01(np.where(k < 2, r[0], r[2])), noise_model.u01(np.where(k < 2, r[1], r[3])), (k & 1).astype(bool)


def normals64(seed, ctr, T, n, a):
    """(z*, bound) [T, n, a] of the draws of the call numbered `ctr`: tests/noise_model.py's model at this feature's counter words"""
    z, b = noise_model.bound(*_uniforms(int(seed), int(ctr), T, n, a))
    return z.reshape(T, n, a), b.reshape(T, n, a)


def normals32(seed, ctr, T, n, a, stream=STREAM_COLLECT, with_t=True):
    """the same draws in numpy float32 (tests/noise_model.py: emulate32's reduction by quarter revolutions)"""
    u1, u2, odd = _uniforms(int(seed), int(ctr), T, n, a, stream, with_t)
    rad = np.sqrt(F(-2.0) * np.log(u1))
    q = np.floor(u2 * F(4.0) + F(0.5))
    ang = noise_model.TWO_PI_F32 * (u2 - q * F(0.25))
    s, c = np.sin(ang), np.cos(ang)
    qi = q.astype(np.int64) & 3
    sin_, cos_ = np.choose(qi, [s, c, -s, -c]), np.choose(qi, [c, -s, -c, s])
    z = (rad * np.where(odd, sin_, cos_)).astype(F)
    assert z.dtype == F, ("normals32", "not computed in float32")
    return z.reshape(T, n, a)


# ---------------------------------------------------------------------------------------------------- the actor as intervals
def action_intervals(p, S, eps, *, mode, sac, ln, scale, bias, noise_std):
    """(lo, hi) [N, a] of the action the policy chooses at the observation rows S [N, o] with the draws eps [N, a]"""
    a = len(scale)
    u, bu = eval_model.forward64(p, S, ln)
    if mode == EXPLORE and sac:
        return bounds.squash((u, bu), eps, scale, bias)["action"]
    act = bounds.td3_policy((u[:, :a], bu[:, :a]), scale, bias)["action"]
    if mode == EXPLORE:
        s32 = (np.asarray(scale, F) * F(noise_std)).astype(F)          # the kernel's own float32 product: exact here
        return (bounds._Iv(*act) + bounds._Iv(bounds.f64(eps)) * bounds.f64(s32)).pair()
    return act


# ---------------------------------------------------------------------------------------------------- the slab from the recorded actions
def host_twin(kind, n, horizon, env_seed, state):
    from sac_td3_cudagraphs_pytorch_amd import envs
    env = envs.HostVecEnv(kind, n, seed=env_seed, horizon=horizon)
    if state is not None:
        env.set_state(state)
    return env


def step_packed(env, obs, act, layout):
    """one step of a host twin with `act`, packed by the stored-next rule -> (records [n, record_floats], the observations to act on next)"""
    from sac_td3_cudagraphs_pytorch_amd import envs
    nobs, rew, term, trunc, infos = env.step(act)
    stored = nobs.copy()
    for k in np.flatnonzero(trunc):
        stored[k] = infos["final_observation"][k]
    return envs.pack_records(layout, obs, act, rew, stored, term), nobs


def rebuild_on_host(kind, n, T, horizon, env_seed, state, actions, layout):
    """the slab of T steps with actions [T, n, a] from `state`, on the numpy host twin -> (slab [T n, record_floats], the twin behind it)"""
    from sac_td3_cudagraphs_pytorch_amd import envs
    env = host_twin(kind, n, horizon, env_seed, state)
    obs = envs.observe(env.kind, env.s, env.goal)
    rows = []
    for t in range(T):
        rec, obs = step_packed(env, obs, np.asarray(actions[t], F), layout)
        rows.append(rec)
    return np.concatenate(rows, 0), env


# ---------------------------------------------------------------------------------------------------- the checker
def _same_bits(name, got, want):
    eval_model._same_bits(name, np.asarray(got), np.asarray(want))


def check_collect(got, p, *, kind, n, T, mode, sac, ln, scale, bias, noise_std, seed, ctr, env_seed, draws0, layout, rebuilt, twin_state):
    """Every element of what a call left: got = {slab [T n, record_floats] float32, eps [T, n, a] float32, state: the env's state behind the
    call}.  p: eval_model.actor_params (unused in RANDOM); ctr: collect_ctr in front of the call; draws0 [n]: the env's draw counts in
    front of it; rebuilt: the slab of a twin stepped with the recorded actions; twin_state: that twin's state behind them (draws as in
    front of the call: a twin that is handed its actions draws nothing).  Raises bounds.Violation; -> the worst |err| / bound of the
    bounded checks (0 for RANDOM: everything there is bits)."""
    from sac_td3_cudagraphs_pytorch_amd import envs
    k = envs.kind_of(kind)
    o, a = envs.SPECS[k][:2]
    slab, eps = np.asarray(got["slab"]), np.asarray(got["eps"])
    if slab.shape != (T * n, layout[0]) or slab.dtype != F or eps.shape != (T, n, a) or eps.dtype != F:
        raise bounds.Violation(f"shapes: slab {slab.shape} {slab.dtype}, eps {eps.shape} {eps.dtype}")
    f = fields(slab, layout, o, a)
    worst = 0.0
    want_draws = np.asarray(draws0, np.uint32)
    if mode == RANDOM:
        want = np.stack([envs.random_actions(k, env_seed, np.arange(n), want_draws + np.uint32(t)) for t in range(T)])
        _same_bits("a (the env's own draw number draws + t)", f["a"].reshape(T, n, a), want)
        want_draws = want_draws + np.uint32(T)
    else:
        lo, hi = action_intervals(p, f["s"], eps.reshape(T * n, a), mode=mode, sac=sac, ln=ln, scale=scale, bias=bias, noise_std=noise_std)
        worst = max(worst, bounds.check_interval("a", f["a"], lo, hi))
    if mode == EXPLORE:
        z, zb = normals64(seed, ctr, T, n, a)
        worst = max(worst, bounds.check("eps", eps, z, zb))
    else:
        _same_bits("eps (only an exploring call draws)", eps, np.zeros((T, n, a), F))
    _same_bits("slab (a twin stepped with the recorded actions, row t n + i)", slab, rebuilt)
    state = got["state"]
    for key in ("phys", "steps", "episode", "returns"):
        _same_bits("env state: " + key, state[key], twin_state[key])
    _same_bits("env state: draws", np.asarray(state["draws"], np.uint32), want_draws)
    return worst


# ---------------------------------------------------------------------------------------------------- the fp32 emulation and its defects
DEFECTS = ("stream_code", "no_t", "env_major", "next_not_arrival", "d_on_truncation", "noise_no_scale", "clamped_action", "draws_stuck")


def emulate32(kind, n, T, horizon, p, *, mode, sac, ln, noise_std, seed, ctr, env_seed, state=None, defect=None):
    """the whole call in numpy float32 on the env's host twin -> ({slab, eps, state}, scale, bias, draws0, layout)"""
    from sac_td3_cudagraphs_pytorch_amd import envs
    env = host_twin(kind, n, horizon, env_seed, state)
    o, a, bound = env.o, env.a, F(env.bound)
    layout = layout_for(o, a)
    scale, bias = np.full(a, bound, F), np.zeros(a, F)
    draws0 = env.draws.copy()
    obs = envs.observe(env.kind, env.s, env.goal)
    if mode == EXPLORE:
        e_all = normals32(seed, ctr, T, n, a, stream=0x800 if defect == "stream_code" else STREAM_COLLECT, with_t=defect != "no_t")
    else:
        e_all = np.zeros((T, n, a), F)
    rows = []
    for t in range(T):
        if mode == RANDOM:
            act = env.action_space.sample()
            if defect == "draws_stuck":
                env.draws = draws0.copy()
        else:
            u = eval_model.forward32(p, obs, ln)
            if mode == EXPLORE and sac:
                u0, u1 = u[:, :a], u[:, a:]
                sd = np.exp(F(-5.0) + F(3.5) * (np.tanh(u1) + F(1.0)))
                act = (np.tanh(u0 + e_all[t] * sd) * scale + bias).astype(F)
            else:
                act = (np.tanh(u[:, :a]) * scale + bias).astype(F)
                if mode == EXPLORE:
                    act = (act + e_all[t] * (F(noise_std) if defect == "noise_no_scale" else scale * F(noise_std))).astype(F)
        nobs, rew, term, trunc, infos = env.step(act)
        stored = nobs.copy()
        if defect != "next_not_arrival":
            for k in np.flatnonzero(trunc):
                stored[k] = infos["final_observation"][k]
        kept = np.minimum(np.maximum(act, -bound), bound) if defect == "clamped_action" else act
        rows.append(envs.pack_records(layout, obs, kept, rew, stored, (term | trunc) if defect == "d_on_truncation" else term))
        obs = nobs
    slab = np.stack(rows)                                                 # [T, n, record_floats]
    slab = (slab.transpose(1, 0, 2) if defect == "env_major" else slab).reshape(T * n, layout[0])
    return {"slab": np.ascontiguousarray(slab), "eps": e_all, "state": env.state()}, scale, bias, draws0, layout


def check_emulation(kind, n, T, horizon, p, *, state=None, defect=None, **kw):
    """emulate32 put to check_collect with the host twin as the twin -> the worst |err| / bound"""
    got, scale, bias, draws0, layout = emulate32(kind, n, T, horizon, p, state=state, defect=defect, **kw)
    o, a = _dims(kind)
    actions = fields(got["slab"], layout, o, a)["a"].reshape(T, n, a)      # (read where the header puts them: row t n + i)
    rebuilt, twin = rebuild_on_host(kind, n, T, horizon, kw["env_seed"], state, actions, layout)
    return check_collect(got, p, kind=kind, n=n, T=T, scale=scale, bias=bias, draws0=draws0, layout=layout, rebuilt=rebuilt,
                         twin_state=twin.state(), **kw), got


def _dims(kind):
    from sac_td3_cudagraphs_pytorch_amd import envs
    return envs.SPECS[envs.kind_of(kind)][:2]
