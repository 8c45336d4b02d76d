"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  A float64 model of one step of the two GPU-resident environments (include/sactd3_env.h,
csrc/env_kernels.h), the a-priori bound of the device's fp32 result around it, the checker that holds a step against both, and an fp32
emulation of the kernel with the defects the checker has to refuse.  Checked on the CPU by tests/test_env_model.py; used on the GPU
by tests/test_gpu_native_env.py.

The model takes the device's own fp32 inputs (state, action) as exact and computes the step in float64 with the true pi.  The bound is
built as tests/bounds.py builds its bounds and is never fitted to an observed error of the env: every fp32 operation of the kernel
adds U = 2^-24 times the magnitude of its result to the error carried by its operands (class V below propagates that to first order,
operation by operation, in the kernel's own operation order); an operation whose operands are exact and whose exact result is a
float32 adds nothing (x + 0.02 * 0 IS x: that is what lets a state be planted exactly on a threshold); sinf / cosf add their worst
absolute error over [-3.15, 3.15], measured against float64 on the MI355X over every float32 argument (tools/libm_trig.py ->
profiles/libm_trig.json) and used as measured, with no factor on top; the fp32 constants pi, 2 pi and 1 / (2 pi) add their distance
from the true ones where an angle wraps.  Angles are compared through their sine and cosine, so a wrap at +-pi that fp32 and float64
decide differently is not an error.

Flags must be exactly equal.  That is a condition on the INPUTS: a step whose model value lies within its bound of a threshold (the
cart-pole's two limits; +-pi under the pendulum's cost) cannot be decided by the model, `conditioned` says which envs can, and the
tests require every planted and rolled state to be conditioned -- decided on the CPU by the model alone.

This is not a test module, so pytest does not rewrite its asserts: every assert here carries its own message."""
import json
import os

import numpy as np

from oracle import replay_ref
from tests import bounds

U = bounds.U
F = np.float32
PENDULUM, CARTPOLE = 0, 1
KINDS = {"pendulum": PENDULUM, "cartpole": CARTPOLE}
OB_DIM = {PENDULUM: 3, CARTPOLE: 4}
BOUND = {PENDULUM: 2.0, CARTPOLE: 1.0}
HORIZON = 200
STREAM_ENV = 0x500
PI_F, TWO_PI_F, INV_2PI_F = F(3.14159274), F(6.28318548), F(0.159154937)
C_PI = abs(float(PI_F) - np.pi)                 # 8.74e-8: what fl32(pi) is away from pi
C_2PI = abs(float(TWO_PI_F) - 2.0 * np.pi)      # 1.75e-7
X_LIMIT, THETA_LIMIT = F(2.4), F(0.20943951)
TRIG_TOP = 3.15                                 # the range the library's error was measured over

with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "libm_trig.json")) as _f:
    _TRIG = json.load(_f)
SINF_ABS, COSF_ABS = float(_TRIG["sinf_abs"]), float(_TRIG["cosf_abs"])      # as measured: no factor on top
assert _TRIG["top"] >= TRIG_TOP - 1e-6, ("env_model", "profiles/libm_trig.json covers less than [-3.15, 3.15]")


def f32c(x):
    return float(F(x))


# ---------------------------------------------------------------------------------------------------- values with an error bound
class V:
    """a float64 array `v` and a bound `e` >= 0 of |device value - v|"""

    def __init__(self, v, e=0.0):
        self.v = bounds.f64(v)
        self.e = np.broadcast_to(bounds.f64(e), self.v.shape).copy()

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(f32c(x))

    @staticmethod
    def _rounded(r, e_in):
        """the bound behind one fp32 operation with exact result r whose operands' errors move it by at most e_in"""
        exact = (e_in == 0.0) & (r.astype(F).astype(np.float64) == r)
        return V(r, np.where(exact, 0.0, e_in + U * (np.abs(r) + e_in)))

    def __add__(self, o):
        o = V.of(o)
        return V._rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = V.of(o)
        return V._rounded(self.v - o.v, self.e + o.e)

    def __neg__(self):
        return V(-self.v, self.e)

    def __mul__(self, o):
        o = V.of(o)
        return V._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    __radd__, __rmul__ = __add__, __mul__

    def __truediv__(self, o):
        o = V.of(o)
        assert (np.abs(o.v) > 2.0 * o.e).all(), ("env_model", "a divisor is not bounded away from zero")
        r = self.v / o.v
        return V._rounded(r, (self.e + np.abs(r) * o.e) / (np.abs(o.v) - o.e))

    def clamp(self, b):
        return V(np.clip(self.v, -b, b), self.e)      # 1-Lipschitz: the error does not grow

    def sin(self):
        assert (np.abs(self.v) <= TRIG_TOP).all(), ("env_model", "an angle outside the range sinf was measured over")
        return V(np.sin(self.v), self.e + SINF_ABS)

    def cos(self):
        assert (np.abs(self.v) <= TRIG_TOP).all(), ("env_model", "an angle outside the range cosf was measured over")
        return V(np.cos(self.v), self.e + COSF_ABS)


def angnorm(x):
    """x - 2 pi floor((x + pi) / (2 pi)) with the true pi -> (V, ambiguous): `ambiguous` where the device's floor may be another than the
    model's.  There the device's result is the model's up to a whole turn and the bound covers both choices: good for a sine or a
    cosine, not for a square."""
    k = np.floor((x.v + np.pi) / (2.0 * np.pi))
    r = x.v - 2.0 * np.pi * k
    # the device floors fl(fl(x_d + pi_f) * inv_f): in units of x that is (x + pi) moved by at most x.e, pi_f - pi, and four roundings
    # (the sum, the constant 1 / (2 pi), the product) of at most |x| + pi each; 5 covers the second-order terms
    margin = x.e + C_PI + 5.0 * U * (np.abs(x.v) + np.pi)
    amb = np.minimum(r + np.pi, np.pi - r) <= margin
    kk = np.maximum(np.abs(k), amb.astype(np.float64))                     # whole turns taken off by either choice
    moved = kk > 0
    e = x.e + np.where(moved, U * (np.pi + x.e) + kk * C_2PI + np.where(kk > 1, U * 2.0 * np.pi * kk, 0.0), 0.0)
    return V(r, e), amb


# ---------------------------------------------------------------------------------------------------- the model of one step
def physics(kind, phys, act):
    """phys [n, 4], act [n]: the device's fp32 state and action.  -> dict(s2: [V] the state arrived at; reward: V; obs: [V] its
    observation; angle: indices of s2 that are angles compared through sine and cosine; terminal [n] bool; conditioned [n] bool;
    bad [n] bool)"""
    phys, a = bounds.f64(phys), bounds.f64(act).reshape(-1)
    bad = ~np.isfinite(a)
    u = V(np.clip(np.where(bad, 0.0, a), -BOUND[kind], BOUND[kind]))
    n = len(a)
    if kind == PENDULUM:
        th, w = V(phys[:, 0]), V(phys[:, 1])
        thn, amb = angnorm(th)
        cost = ((thn * thn) + (V.of(0.1) * (w * w))) + (V.of(0.001) * (u * u))
        acc = (V.of(15.0) * th.sin()) + (V.of(3.0) * u)
        w2 = (w + (acc * V.of(0.05))).clamp(8.0)
        th2, _ = angnorm(th + (V.of(0.05) * w2))
        obs = [V(np.cos(th2.v), th2.e + COSF_ABS), V(np.sin(th2.v), th2.e + SINF_ABS), w2]
        return dict(s2=[th2, w2], reward=-cost, obs=obs, angle=(0,), terminal=np.zeros(n, bool), conditioned=~amb, bad=bad)
    x, xd, th, thd = (V(phys[:, j]) for j in range(4))
    f = V.of(10.0) * u
    c, sn = th.cos(), th.sin()
    temp = (f + ((V.of(0.05) * (thd * thd)) * sn)) / V.of(1.1)
    den = V.of(0.5) * (V.of(1.33333337) - ((V.of(0.1) * (c * c)) / V.of(1.1)))
    thacc = ((V.of(9.8) * sn) - (c * temp)) / den
    xacc = temp - (((V.of(0.05) * thacc) * c) / V.of(1.1))
    s2 = [x + (V.of(0.02) * xd), xd + (V.of(0.02) * xacc), th + (V.of(0.02) * thd), thd + (V.of(0.02) * thacc)]
    terminal, sure = np.zeros(n, bool), np.ones(n, bool)
    for j, limit in ((0, float(X_LIMIT)), (2, float(THETA_LIMIT))):
        terminal |= np.abs(s2[j].v) > limit
        sure &= (s2[j].e == 0.0) | (np.abs(np.abs(s2[j].v) - limit) > s2[j].e)
    return dict(s2=s2, reward=V(np.ones(n)), obs=s2, angle=(), terminal=terminal, conditioned=sure, bad=bad)


def u01(x):
    return ((np.asarray(x, np.uint32) >> np.uint32(8)).astype(F) + F(0.5)) * F(1.0 / 16777216.0)


def first_states(kind, seed, env_index, episode):
    """[n, 4] float32, bit for bit what the device draws: Philox words (episode, env, 0x500, 0) keyed by the seed, through philox_u01"""
    env_index, episode = np.asarray(env_index, np.uint64), np.asarray(episode, np.uint64)
    r = replay_ref.philox4x32_10(episode, env_index, np.full(len(env_index), STREAM_ENV), np.zeros(len(env_index), np.uint64),
                                 int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    u = np.stack([u01(w) for w in r], 1)
    s = np.zeros(u.shape, F)
    if kind == PENDULUM:
        s[:, 0] = -PI_F + TWO_PI_F * u[:, 0]
        s[:, 1] = F(-1.0) + F(2.0) * u[:, 1]
    else:
        s[:] = F(-0.05) + F(0.1) * u
    return s


def random_actions(kind, seed, env_index, draw):
    """[n, 1] float32, bit for bit: word 0 of Philox (draw, env, 0x500, 1)"""
    env_index, draw = np.asarray(env_index, np.uint64), np.asarray(draw, np.uint64)
    r = replay_ref.philox4x32_10(draw, env_index, np.full(len(env_index), STREAM_ENV), np.ones(len(env_index), np.uint64),
                                 int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    b = F(BOUND[kind])
    return (-b + (b - (-b)) * u01(r[0])).astype(F).reshape(-1, 1)


def observe64(kind, s):
    """the observation of an fp32 state as (value, bound): exact for the cart-pole, through sinf / cosf for the pendulum"""
    s = bounds.f64(s)
    if kind == PENDULUM:
        return (np.stack([np.cos(s[:, 0]), np.sin(s[:, 0]), s[:, 1]], 1),
                np.stack([np.full(len(s), COSF_ABS), np.full(len(s), SINF_ABS), np.zeros(len(s))], 1))
    return s.copy(), np.zeros_like(s)


# ---------------------------------------------------------------------------------------------------- the checker
def conditioned(kind, before, actions):
    """[n] bool: the envs whose step the model can decide (module docstring)"""
    return physics(kind, before["phys"], actions)["conditioned"]


def _near(name, got, want, bound):
    got = bounds.f64(got)
    want, bound = np.broadcast_to(bounds.f64(want), got.shape), np.broadcast_to(bounds.f64(bound), got.shape)
    err = np.abs(got - want)
    ok = err <= bound                                                    # (a NaN fails)
    if not ok.all():
        i = int(np.argmax(np.where(ok, -np.inf, np.where(np.isnan(err), np.inf, err - bound))))
        raise bounds.Violation(f"{name}: {int((~ok).sum())} of {ok.size} outside the bound; worst at env {i}: got {got[i]!r} want {want[i]!r} "
                               f"err {err[i]:.3e} bound {bound[i]:.3e}")
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, 0.0)
    return float(ratio.max()) if ratio.size else 0.0


def _same(name, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype or got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got.reshape(len(got), -1) != want.reshape(len(want), -1)).any(1)) if got.shape == want.shape else []
        raise bounds.Violation(f"{name}: not the same bits (envs {list(bad[:8])}; {got.dtype}{got.shape} against {want.dtype}{want.shape})")


def check_step(kind, seed, horizon, before, actions, got, after):
    """One vector step against the model.  before / after: the env's state() on either side of the step (phys [n, 4], steps, episode,
    returns); actions [n, 1] as given; got: obs, final_obs [n, o], reward [n], terminated, truncated, ended [n] as the step returned
    them.  Raises bounds.Violation; every env must be conditioned (the caller's inputs are at fault otherwise: AssertionError).
    -> the worst |err| / bound."""
    n = len(before["steps"])
    m = physics(kind, before["phys"], actions)
    assert m["conditioned"].all(), ("check_step", "inputs within the bound of a threshold", np.flatnonzero(~m["conditioned"])[:8])
    worst = _near("reward", got["reward"], m["reward"].v, m["reward"].e)
    for j, ob in enumerate(m["obs"]):
        worst = max(worst, _near(f"final_obs[{j}]", np.asarray(got["final_obs"])[:, j], ob.v, ob.e))
    # flags: exactly the model's
    t2 = np.asarray(before["steps"], np.int64) + 1
    term = m["terminal"]
    trunc = ~term & (t2 >= horizon)
    ended = term | trunc
    _same("terminated", np.asarray(got["terminated"]).astype(bool), term)
    _same("truncated", np.asarray(got["truncated"]).astype(bool), trunc)
    _same("ended", np.asarray(got["ended"]).astype(bool), ended)
    # the state behind the step, and the observation to act on
    env = np.arange(n)
    ep2 = (np.asarray(before["episode"], np.uint32) + ended.astype(np.uint32)).astype(np.uint32)
    fresh = first_states(kind, seed, env, ep2)
    _same("episode", np.asarray(after["episode"], np.uint32), ep2)
    _same("steps", np.asarray(after["steps"], np.int32), np.where(ended, 0, t2).astype(np.int32))
    run = (np.asarray(before["returns"], F) + np.asarray(got["reward"], F)).astype(F)          # one fp32 addition of the device's own reward
    _same("returns", np.asarray(after["returns"], F), np.where(ended, F(0.0), run).astype(F))
    phys2 = np.asarray(after["phys"], F)
    if ended.any():
        _same("state behind a reset", phys2[ended], fresh[ended])
        want, wb = observe64(kind, fresh[ended])
        for j in range(OB_DIM[kind]):
            worst = max(worst, _near(f"obs[{j}] behind a reset", np.asarray(got["obs"])[ended, j], want[:, j], wb[:, j]))
    go = ~ended
    if go.any():
        _same("obs of an env that goes on (= final_obs)", np.asarray(got["obs"])[go], np.asarray(got["final_obs"])[go])
        for j, s in enumerate(m["s2"]):
            if j in m["angle"]:                                                      # through sine and cosine, and inside [-pi, pi]
                worst = max(worst, _near(f"sin state[{j}]", np.sin(bounds.f64(phys2[go, j])), np.sin(s.v[go]), s.e[go]))
                worst = max(worst, _near(f"cos state[{j}]", np.cos(bounds.f64(phys2[go, j])), np.cos(s.v[go]), s.e[go]))
                worst = max(worst, _near(f"range of state[{j}]", np.maximum(np.abs(bounds.f64(phys2[go, j])) - np.pi, 0.0), 0.0, s.e[go] + C_2PI + U * np.pi))
            else:
                worst = max(worst, _near(f"state[{j}]", phys2[go, j], s.v[go], s.e[go]))
    return worst


# ---------------------------------------------------------------------------------------------------- planted states
def planted(kind, horizon=HORIZON):
    """-> (phys [m, 4] float32, steps [m] int32, actions [m, 1] float32): the states a step can go wrong at"""
    up = lambda x: np.nextafter(F(x), F(np.inf))
    last = horizon - 1
    if kind == PENDULUM:
        rows = [  # theta, omega, steps, action
            (PI_F - F(1e-3), 2.0, 0, 0.5),          # theta just below pi: wraps
            (-PI_F + F(1e-3), -2.0, 3, -0.5),       # ... and the other way
            (0.5, 8.0, 7, 2.0),                     # omega at +8, pushed further: the clip
            (-0.5, -8.0, 7, -2.0),                  # omega at -8
            (1.0, 0.3, last, 0.7),                  # the horizon step: truncated
            (2.5, -7.5, last - 1, 5.0),             # one before it; an action beyond the bounds
            (-3.0, 6.0, 0, -9.0),
            (0.0, 0.0, 10, 0.0),                    # at rest, upright
            (3.0, 7.9, 1, 2.0),                     # fast towards +pi: clip and wrap in one step
        ]
        phys = np.array([[r[0], r[1], 0, 0] for r in rows], F)
    else:
        rows = [  # x, x_dot, theta, theta_dot, steps, action
            (X_LIMIT, 0, 0, 0, 5, 0.0),                       # exactly 2.4: not beyond it
            (up(X_LIMIT), 0, 0, 0, 5, 0.0),                   # one ulp above: terminated
            (-X_LIMIT, 0, 0.01, 0, 5, 0.3),
            (-up(X_LIMIT), 0, 0.01, 0, 5, 0.3),
            (0.1, 0.2, THETA_LIMIT, 0, 9, -1.0),              # the pole at the angle threshold
            (0.1, 0.2, up(THETA_LIMIT), 0, 9, -1.0),
            (0.1, 0.2, -THETA_LIMIT, 0, 9, 1.0),
            (2.5, 1.0, 0.05, 0.1, last, 0.5),                 # termination on the horizon step: terminated, not truncated
            (0.3, -0.4, 0.02, 0.3, last, -0.2),               # the horizon step: truncated
            (0.3, -0.4, 0.02, 0.3, last - 1, 3.0),            # one before it; an action beyond the bounds
            (-1.0, 2.0, -0.15, -1.5, 0, -7.0),
            (0.0, 0.0, 0.0, 0.0, 0, 0.0),
        ]
        phys = np.array([r[:4] for r in rows], F)
    return phys, np.array([r[-2] for r in rows], np.int32), np.array([[r[-1]] for r in rows], F)


def random_states(kind, n, rng, horizon=HORIZON):
    """n states and actions spread over what an episode visits (and a little beyond the bounds of the action)"""
    if kind == PENDULUM:
        phys = np.stack([rng.uniform(-3.1, 3.1, n), rng.uniform(-8, 8, n), np.zeros(n), np.zeros(n)], 1).astype(F)
    else:
        phys = np.stack([rng.uniform(-2.3, 2.3, n), rng.uniform(-2, 2, n), rng.uniform(-0.2, 0.2, n), rng.uniform(-2, 2, n)], 1).astype(F)
    steps = rng.integers(0, horizon, n).astype(np.int32)
    return phys, steps, rng.uniform(-1.2 * BOUND[kind], 1.2 * BOUND[kind], (n, 1)).astype(F)


def batch(kind, n, offset, rng, horizon=HORIZON):
    """n envs' worth of inputs: the planted rows from `offset` on (cyclically, as many as fit), random states behind them"""
    p, s, a = planted(kind, horizon)
    take = (offset + np.arange(min(n, len(s)))) % len(s)
    rp, rs, ra = random_states(kind, n - len(take), rng, horizon)
    return np.concatenate([p[take], rp]), np.concatenate([s[take], rs]), np.concatenate([a[take], ra])


# ---------------------------------------------------------------------------------------------------- the fp32 emulation and its defects
DEFECTS = ("reward_from_next_state", "no_speed_clip", "angle_not_normalised", "ge_at_threshold", "final_obs_after_reset",
           "truncated_with_terminated", "reset_ignores_episode", "force_not_scaled")


def _sin32(x):
    """sinf as the correctly rounded sine (error at most half an ulp: inside what the library's measured figure allows)"""
    return np.sin(x.astype(np.float64)).astype(F)


def _cos32(x):
    return np.cos(x.astype(np.float64)).astype(F)


def _angnorm32(x):
    return x - TWO_PI_F * np.floor((x + PI_F) * INV_2PI_F)


def _observe32(kind, s):
    return np.stack([_cos32(s[:, 0]), _sin32(s[:, 0]), s[:, 1]], 1) if kind == PENDULUM else s.copy()


def emulate32(kind, seed, horizon, before, actions, defect=None):
    """csrc/env_kernels.h: k_env_step in numpy float32, the kernel's operation order -> (got, after) as check_step takes them"""
    assert defect is None or defect in DEFECTS, ("emulate32", "unknown defect", defect)
    s, a = np.asarray(before["phys"], F), np.asarray(actions, F).reshape(-1)
    n = len(a)
    b = F(BOUND[kind])
    u = np.minimum(np.maximum(np.where(np.isfinite(a), a, F(0.0)), -b), b).astype(F)
    s2 = np.zeros_like(s)
    norm = (lambda x: x) if defect == "angle_not_normalised" else _angnorm32
    if kind == PENDULUM:
        th, w = s[:, 0], s[:, 1]
        acc = (F(15.0) * _sin32(th)) + (F(3.0) * u)
        w2 = w + (acc * F(0.05))
        if defect != "no_speed_clip":
            w2 = np.minimum(np.maximum(w2, F(-8.0)), F(8.0))
        s2[:, 0] = norm(th + (F(0.05) * w2))
        s2[:, 1] = w2
        cth, cw = (s2[:, 0], s2[:, 1]) if defect == "reward_from_next_state" else (th, w)
        thn = norm(cth)
        rew = -(((thn * thn) + (F(0.1) * (cw * cw))) + (F(0.001) * (u * u)))
        term = np.zeros(n, bool)
    else:
        x, xd, th, thd = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
        f = u if defect == "force_not_scaled" else F(10.0) * u
        c, sn = _cos32(th), _sin32(th)
        temp = (f + ((F(0.05) * (thd * thd)) * sn)) / F(1.1)
        den = F(0.5) * (F(1.33333337) - ((F(0.1) * (c * c)) / F(1.1)))
        thacc = ((F(9.8) * sn) - (c * temp)) / den
        xacc = temp - (((F(0.05) * thacc) * c) / F(1.1))
        s2[:, 0], s2[:, 1] = x + (F(0.02) * xd), xd + (F(0.02) * xacc)
        s2[:, 2], s2[:, 3] = th + (F(0.02) * thd), thd + (F(0.02) * thacc)
        rew = np.ones(n, F)
        beyond = np.greater_equal if defect == "ge_at_threshold" else np.greater
        term = beyond(np.abs(s2[:, 0]), X_LIMIT) | beyond(np.abs(s2[:, 2]), THETA_LIMIT)
    assert s2.dtype == F and rew.dtype == F, ("emulate32", "not computed in float32")
    t2 = np.asarray(before["steps"], np.int32) + np.int32(1)
    trunc = t2 >= horizon
    if defect != "truncated_with_terminated":
        trunc = trunc & ~term
    ended = term | trunc
    ret = (np.asarray(before["returns"], F) + rew).astype(F)
    final = _observe32(kind, s2)
    ep2 = (np.asarray(before["episode"], np.uint32) + ended.astype(np.uint32)).astype(np.uint32)
    fresh = first_states(kind, seed, np.arange(n), np.zeros(n, np.uint32) if defect == "reset_ignores_episode" else ep2)
    nxt = np.where(ended[:, None], fresh, s2).astype(F)
    obs = _observe32(kind, nxt)
    got = {"obs": obs, "final_obs": obs.copy() if defect == "final_obs_after_reset" else final, "reward": rew,
           "terminated": term, "truncated": trunc, "ended": ended}
    after = {"phys": nxt, "steps": np.where(ended, 0, t2).astype(np.int32), "episode": ep2, "returns": np.where(ended, F(0.0), ret).astype(F),
             "draws": np.asarray(before.get("draws", np.zeros(n, np.uint32)), np.uint32)}
    return got, after
