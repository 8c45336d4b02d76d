"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  A float64 model and a float32 restatement of the goal env (include/sactd3_env.h:
SACTD3_ENV_POINTGOAL; csrc/env_kernels.h), with its resets, goals and random actions from the oracle's Philox.  Checked on the CPU by
tests/test_goal_env_host.py; used on the GPU by tests/test_gpu_goal_env.py.

The float64 model takes the device's own fp32 inputs as exact.  Its bound is one rounding per fp32 operation of the kernel, carried
to first order in the kernel's operation order by the class V below (an operation with exact operands and an exactly
representable result adds nothing: that is what lets a state be planted exactly on the wall or on the goal's threshold).  The reward
is a comparison: an env whose model d2 lies within its bound of thr^2 cannot be decided by the model, `conditioned` says which can.
The task calls no libm function, so the float32 restatement (`step32`) is what the kernel and the host twin compute, bit for bit.

This is not a test module, so pytest does not rewrite its asserts: every assert here carries its own message."""
import numpy as np

from oracle import replay_ref
from tests import bounds

U = bounds.U
F = np.float32


def f32c(x):
    return float(F(x))


# ---------------------------------------------------------------------------------------------------- values with an error bound
class V:
    """a float64 array `v` and a bound `e` >= 0 of |device value - v| (the rule of tests/env_model.py, restated: this task needs +, -, *
    and the clamp only)"""

    def __init__(self, v, e=0.0):
        self.v = bounds.f64(v)
        self.e = np.broadcast_to(bounds.f64(e), self.v.shape).copy()

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(f32c(x))

    @staticmethod
    def _rounded(r, e_in):
        """the bound behind one fp32 operation with exact result r whose operands' errors move it by at most e_in: an operation whose
        operands are exact and whose exact result is a float32 adds nothing"""
        exact = (e_in == 0.0) & (r.astype(F).astype(np.float64) == r)
        return V(r, np.where(exact, 0.0, e_in + U * (np.abs(r) + e_in)))

    def __add__(self, o):
        o = V.of(o)
        return V._rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = V.of(o)
        return V._rounded(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = V.of(o)
        return V._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def clamp(self, b):
        return V(np.clip(self.v, -b, b), self.e)      # 1-Lipschitz: the error does not grow


def u01(x):
    return ((np.asarray(x, np.uint32) >> np.uint32(8)).astype(F) + F(0.5)) * F(1.0 / 16777216.0)


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


KIND, OB_DIM, AC_DIM, BOUND, HORIZON = 2, 6, 2, 1.0, 50
STREAM_ENV = 0x500
THR = F(0.1)
THR2 = F(THR * THR)                               # one fp32 product
C08, C02, C01 = F(0.8), F(0.2), F(0.1)
LAYOUT = dict(achieved=0, desired=4, dim=2, threshold=0.1)


def _philox(seed, first, env_index, which):
    env_index, first = np.asarray(env_index, np.uint64), np.asarray(first, np.uint64)
    n = len(env_index)
    return replay_ref.philox4x32_10(first, env_index, np.full(n, STREAM_ENV), np.full(n, which, np.uint64), int(seed) & 0xFFFFFFFF,
                                    (int(seed) >> 32) & 0xFFFFFFFF)


def first_states(seed, env_index, episode):
    """[n, 4] float32: words 0 and 1 of Philox (episode, env, 0x500, 0) -> x, y in (-1, 1); at rest"""
    r = _philox(seed, episode, env_index, 0)
    s = np.zeros((len(r[0]), 4), F)
    s[:, 0], s[:, 1] = F(-1.0) + F(2.0) * u01(r[0]), F(-1.0) + F(2.0) * u01(r[1])
    return s


def goals(seed, env_index, episode):
    """[n, 2] float32: words 0 and 1 of Philox (episode, env, 0x500, 2)"""
    r = _philox(seed, episode, env_index, 2)
    return np.stack([F(-1.0) + F(2.0) * u01(r[0]), F(-1.0) + F(2.0) * u01(r[1])], 1).astype(F)


def random_actions(seed, env_index, draw):
    """[n, 2] float32: words 0 and 1 of Philox (draw, env, 0x500, 1)"""
    r = _philox(seed, draw, env_index, 1)
    b = F(BOUND)
    return np.stack([(-b + (b - (-b)) * u01(r[j])).astype(F) for j in range(AC_DIM)], 1)


def reward32(achieved, goal):
    """the thresholded squared distance in float32, in the stated order: [n, 2] against [n, 2] -> [n] (0 or -1)"""
    achieved, goal = np.asarray(achieved, F), np.asarray(goal, F)
    dx, dy = achieved[:, 0] - goal[:, 0], achieved[:, 1] - goal[:, 1]
    d2 = (dx * dx) + (dy * dy)
    assert d2.dtype == F, ("goal_env_model", "not computed in float32")
    return np.where(d2 <= THR2, F(0.0), F(-1.0)).astype(F)


# ---------------------------------------------------------------------------------------------------- float64, with the bound
def physics(phys, act, goal):
    """phys [n, 4], act [n, 2], goal [n, 2]: the device's fp32 values -> dict(s2: [V] x', y', vx', vy'; d2: V; reward [n];
    conditioned [n] bool; bad [n] bool)"""
    phys, a, g = bounds.f64(phys), bounds.f64(act).reshape(-1, AC_DIM), bounds.f64(goal)
    nonfinite = ~np.isfinite(a)
    u = np.clip(np.where(nonfinite, 0.0, a), -BOUND, BOUND)
    pos, vel = [], []
    for c in range(2):
        v = (V.of(C08) * V(phys[:, 2 + c])) + (V.of(C02) * V(u[:, c]))
        pos.append((V(phys[:, c]) + (V.of(C01) * v)).clamp(1.0))
        vel.append(v)
    dx, dy = pos[0] - V(g[:, 0]), pos[1] - V(g[:, 1])
    d2 = (dx * dx) + (dy * dy)
    # where the arrival is known exactly (a planted state at rest), the stated fp32 expression IS the answer: nothing to bound
    known = (pos[0].e == 0.0) & (pos[1].e == 0.0)
    sure = known | (np.abs(d2.v - float(THR2)) > d2.e)
    exact = reward32(np.stack([pos[0].v, pos[1].v], 1).astype(F), g.astype(F)).astype(np.float64)
    return dict(s2=pos + vel, d2=d2, reward=np.where(known, exact, np.where(d2.v <= float(THR2), 0.0, -1.0)), conditioned=sure,
                bad=nonfinite.any(1))


def conditioned(seed, before, actions):
    n = len(before["steps"])
    return physics(before["phys"], actions, goals(seed, np.arange(n), before["episode"]))["conditioned"]


# ---------------------------------------------------------------------------------------------------- float32, bit for bit
def step32(seed, horizon, before, actions, defect=None):
    """k_env_step<POINTGOAL> in numpy float32 -> (got, after) as check_step takes them"""
    s, a = np.asarray(before["phys"], F), np.asarray(actions, F).reshape(-1, AC_DIM)
    n = len(a)
    env = np.arange(n)
    ep = np.asarray(before["episode"], np.uint32)
    g = goals(seed, env, ep)
    u = np.minimum(np.maximum(np.where(np.isfinite(a), a, F(0.0)), F(-1.0)), F(1.0)).astype(F)
    v = (C08 * s[:, 2:4]) + (C02 * u)
    p = s[:, 0:2] + (C01 * v)
    if defect != "no_wall":
        p = np.minimum(np.maximum(p, F(-1.0)), F(1.0))
    s2 = np.concatenate([p, v], 1).astype(F)
    assert s2.dtype == F and v.dtype == F, ("goal_env_model", "not computed in float32")
    rew = reward32(s[:, 0:2] if defect == "reward_from_departure" else p, g)
    if defect == "lt_at_threshold":
        d = p - g
        rew = np.where(((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) < THR2, F(0.0), F(-1.0)).astype(F)
    t2 = np.asarray(before["steps"], np.int32) + np.int32(1)
    term = np.zeros(n, bool)
    trunc = t2 >= horizon
    ep2 = (ep + trunc.astype(np.uint32)).astype(np.uint32)
    g2 = g if defect == "goal_kept_behind_reset" else goals(seed, env, ep2)
    nxt = np.where(trunc[:, None], first_states(seed, env, ep2), s2).astype(F)
    final = np.concatenate([s2, g2 if defect == "final_obs_with_new_goal" else g], 1)
    ret = (np.asarray(before["returns"], F) + rew).astype(F)
    got = {"obs": np.concatenate([nxt, g2], 1), "final_obs": final, "reward": rew, "terminated": term, "truncated": trunc, "ended": trunc.copy()}
    after = {"phys": nxt, "steps": np.where(trunc, 0, t2).astype(np.int32), "episode": ep2, "returns": np.where(trunc, F(0.0), ret).astype(F),
             "draws": np.asarray(before.get("draws", np.zeros(n, np.uint32)), np.uint32)}
    return got, after


DEFECTS = ("no_wall", "reward_from_departure", "lt_at_threshold", "goal_kept_behind_reset", "final_obs_with_new_goal")


# ---------------------------------------------------------------------------------------------------- the checker
def check_step(seed, horizon, before, actions, got, after, exact=False):
    """One vector step against the float64 model and its bound; flags, books, resets and goals bit for bit.  `exact`: also every
    float against step32, bit for bit (the host twin everywhere; the kernel too, since nothing here goes through libm).  Every env
    must be conditioned.  Raises bounds.Violation.  -> the worst |err| / bound"""
    n = len(before["steps"])
    env = np.arange(n)
    ep = np.asarray(before["episode"], np.uint32)
    g = goals(seed, env, ep)
    m = physics(before["phys"], actions, g)
    assert m["conditioned"].all(), ("check_step", "inputs within the bound of the threshold", np.flatnonzero(~m["conditioned"])[:8])
    fin = np.asarray(got["final_obs"])
    worst = 0.0
    for j, s in enumerate(m["s2"]):
        worst = max(worst, _near(f"final_obs[{j}]", fin[:, j], s.v, s.e))
    _same("final_obs goal", np.ascontiguousarray(fin[:, 4:6]).astype(F), g)
    _same("reward", np.asarray(got["reward"], F), m["reward"].astype(F))
    _same("reward of the device's own arrival", np.asarray(got["reward"], F), reward32(fin[:, 0:2], g))
    t2 = np.asarray(before["steps"], np.int64) + 1
    trunc = t2 >= horizon
    _same("terminated", np.asarray(got["terminated"]).astype(bool), np.zeros(n, bool))
    _same("truncated", np.asarray(got["truncated"]).astype(bool), trunc)
    _same("ended", np.asarray(got["ended"]).astype(bool), trunc)
    ep2 = (ep + trunc.astype(np.uint32)).astype(np.uint32)
    _same("episode", np.asarray(after["episode"], np.uint32), ep2)
    _same("steps", np.asarray(after["steps"], np.int32), np.where(trunc, 0, t2).astype(np.int32))
    run = (np.asarray(before["returns"], F) + np.asarray(got["reward"], F)).astype(F)
    _same("returns", np.asarray(after["returns"], F), np.where(trunc, F(0.0), run).astype(F))
    phys2, obs = np.asarray(after["phys"], F), np.asarray(got["obs"], F)
    _same("obs = state | goal of the running episode", obs, np.concatenate([phys2, goals(seed, env, ep2)], 1))
    if trunc.any():
        _same("state behind a reset", phys2[trunc], first_states(seed, env[trunc], ep2[trunc]))
    go = ~trunc
    if go.any():
        _same("obs of an env that goes on (= final_obs)", obs[go], np.ascontiguousarray(fin[go]).astype(F))
    if exact:
        want, want_after = step32(seed, horizon, before, actions)
        for k in ("obs", "final_obs", "reward"):
            _same(k + " (float32 restatement)", np.asarray(got[k], F), want[k])
        _same("phys (float32 restatement)", phys2, want_after["phys"])
    return worst


# ---------------------------------------------------------------------------------------------------- planted states
def on_threshold(goal, beyond):
    """a position whose fp32 d2 from `goal` is exactly thr^2 (`beyond`: one ulp above it), found by search over positions near the
    circle's 45-degree point, on the side of the goal that stays inside the walls"""
    g = np.asarray(goal, F)
    want = np.nextafter(THR2, F(np.inf)) if beyond else THR2
    sx, sy = (F(-1.0) if g[0] > 0 else F(1.0)), (F(-1.0) if g[1] > 0 else F(1.0))
    base = F(0.0707106781)
    k = np.arange(-1500, 1500)
    xs = (g[0] + sx * (base + k.astype(F) * F(2.0 ** -24))).astype(F)
    ys = (g[1] + sy * (base + k.astype(F) * F(2.0 ** -24))).astype(F)
    dx, dy = (xs - g[0]).astype(F), (ys - g[1]).astype(F)
    d2 = ((dx * dx)[:, None] + (dy * dy)[None, :]).astype(F)
    hit = np.argwhere(d2 == want)
    assert len(hit), ("goal_env_model", "no position on the threshold found", goal)
    i, j = hit[len(hit) // 2]
    return xs[i], ys[j]


def planted(seed, episode=1, horizon=HORIZON):
    """-> (phys [m, 4], steps [m], episode [m], actions [m, 2]): the states a step can go wrong at, for envs 0 .. m-1 in episode
    `episode`: on the walls, exactly on the goal's threshold and one ulp beyond it (at rest, unpushed: the arrival IS the state),
    on the goal, the horizon step and the one before it, actions beyond the bounds"""
    m = 11
    g = goals(seed, np.arange(m), np.full(m, episode))
    away = (-1.0 if g[10, 0] > 0 else 1.0, -1.0 if g[10, 1] > 0 else 1.0)
    last = horizon - 1
    on, off = on_threshold(g[2], False), on_threshold(g[3], True)
    rows = [  # x, y, vx, vy, steps, ax, ay
        (1.0, 0.3, 0.5, 0.0, 3, 1.0, 0.0),                # on the right wall, moving into it: clamped
        (-0.2, -1.0, 0.0, -0.4, 3, 0.3, -2.0),            # on the lower wall; an action beyond the bounds
        (on[0], on[1], 0.0, 0.0, 7, 0.0, 0.0),            # d2 == thr^2 exactly: on the goal (<=)
        (off[0], off[1], 0.0, 0.0, 7, 0.0, 0.0),          # one ulp beyond: off it
        (g[4, 0], g[4, 1], 0.0, 0.0, 0, 0.0, 0.0),        # on the goal itself
        (0.1, -0.2, 0.3, -0.1, last, 0.5, 0.5),           # the horizon step: truncated
        (0.1, -0.2, 0.3, -0.1, last - 1, -3.0, 7.0),      # one before it
        (0.99, 0.99, 1.0, 1.0, 1, 1.0, 1.0),              # into the corner
        (-0.99, 0.5, -1.0, 0.2, 1, -1.0, 0.1),
        (0.0, 0.0, 0.0, 0.0, 10, 0.0, 0.0),               # at rest
        (g[10, 0], g[10, 1], away[0], away[1], 2, away[0], away[1]),      # leaves its goal in this step: the reward is the arrival's
    ]
    assert len(rows) == m, ("goal_env_model", "planted rows and goals differ in number")
    r = np.array(rows, np.float64)
    return r[:, :4].astype(F), r[:, 4].astype(np.int32), np.full(m, episode, np.uint32), r[:, 5:7].astype(F)
