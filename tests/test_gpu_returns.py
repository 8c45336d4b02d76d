"""GPU: returns-to-go of ring rows (include/sactd3_returns.h) against the sequential float64 restatement of tests/returns_model.py.
Data: the test's own arrays, signed rewards, next_obs[t] = obs[t + stride] inside episodes of 1 .. 40 rows per chain, ended in turn by a
termination, a fresh state, +0.0 against -0.0.  The bound is taken from no kernel: any evaluation order of the flagged affine scan puts
at most L multiplications and L additions on a term's path, so |G - G64| <= gamma_m A with m = 2 L + 8 roundings, gamma_m = m u /
(1 - m u), u = 2^-24, A = sum_j gamma^j |r_{t+j}|; the same for the undiscounted sum.  Measured on an MI355X: worst 0.21 of the bound."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.sac_td3_ref import Hps
from tests import returns_model as rm
from tests.gpu_support import DEV, MAXN, P, _lib, assert_same_state, build_engines, close_engines, engine_state, same_bits, track  # noqa: F401
from tests.nstep_ref import place

pytestmark = pytest.mark.gpu
SPAN = _lib.RTG_SPAN
CAP = 4 * SPAN
SHAPES = ((3, 1), (17, 6), (70, 2))
RINGS = {"1": 1, "3": 3, "span-1": SPAN - 1, "span": SPAN, "span+1": SPAN + 1, "2span+3": 2 * SPAN + 3, "wrapped": CAP + 100}
CASES = [(o, a, s, r, False) for o, a in SHAPES for s in (1, 4, 7) for r in RINGS] + [(3, 1, 1, "2span+3", True)]
U = 2.0 ** -24


def episodes(rows, o, a, stride, seed=5, single=False):
    """the five arrays in append order"""
    g = np.random.default_rng(seed)
    obs = g.normal(size=(rows + stride, o)).astype(np.float32)
    nobs, obs = obs[stride:].copy(), obs[:rows].copy()
    act, rew = g.uniform(-0.5, 0.5, size=(rows, a)).astype(np.float32), g.normal(size=rows).astype(np.float32)
    done, k = np.zeros(rows, np.float32), 0
    for c in range(0 if single else stride):
        t = c
        while t < rows:
            t += int(g.integers(1, 41)) * stride
            e, k = t - stride, k + 1
            if e >= rows:
                break
            if k % 3 == 0:
                done[e] = 1.0
            elif k % 3 == 1:
                nobs[e] = g.normal(size=o)
            else:
                nobs[e, 0] = 0.0
                if e + stride < rows:
                    obs[e + stride, 0] = -0.0
    return obs, act, rew, nobs, done


def new_engine(o, a, five=None):
    eng = track(P.Engine(P.Config.from_hps(Hps.sac(batch_size=64), o, a, rb_capacity=CAP, max_envs=MAXN, seed=0), [-0.5] * a, [0.5] * a))
    if five is not None:
        eng.rb_extend(*five)
    return eng


def model(five, gamma, stride, **kw):
    (obs, _, rew, nobs, done), length, cursor = place(five, CAP)
    return rm.returns_to_go(obs, nobs, rew, done, float(np.float32(gamma)), stride, length, cursor, CAP, **kw)


def check(got, want, plain, gamma, what):
    """the exact outputs, and the bound on the two sums over the rows whose model return is finite; `plain`: the model at gamma = 1,
    whose A is the undiscounted sum's yardstick"""
    got = {k: v.cpu().numpy() for k, v in got.items()}
    sl = want["rows"]
    for k, m in (("length", "L"), ("last", "last"), ("ends", "ends")):
        assert (got[k][sl] == want[m][sl]).all(), (what, k)
    one = sl[want["L"][sl] == 1]
    rew = want["G"][one].astype(np.float32)
    assert same_bits(got["returns"][one], rew) and same_bits(got["undiscounted"][one], rew), (what, "chains of one row")
    fin = sl[np.isfinite(want["G"][sl])]
    assert np.isfinite(got["returns"][fin]).all() and not np.isfinite(got["returns"][np.setdiff1d(sl, fin)]).any(), (what, "non-finite rows")
    m = 2.0 * want["L"][fin] + 8.0
    bound = m * U / (1.0 - m * U)
    ratio = max(float((np.abs(got["returns"][fin] - want["G"][fin]) / (bound * want["A"][fin] + 1e-300)).max()),
                float((np.abs(got["undiscounted"][fin] - want["U"][fin]) / (bound * plain["A"][fin] + 1e-300)).max()))
    print("returns_to_go", what, "gamma", gamma, "worst |error| / bound", ratio)
    assert ratio <= 1.0, (what, gamma, ratio)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_against_float64(case):
    o, a, stride, ring, single = case
    five = episodes(RINGS[ring], o, a, stride, single=single)
    eng = new_engine(o, a, five)
    plain = model(five, 1.0, stride)
    for gamma, want in ((0.99, model(five, 0.99, stride)), (1.0, plain)):
        assert not single or want["L"].max() == RINGS[ring]
        check(eng.returns_to_go(gamma, stride), want, plain, gamma, case)
    st, chains = eng.returns_stats(), int((plain["ends"][plain["rows"]] & rm.START != 0).sum())
    assert st["calls"] == 2 and st["rows_scanned"] == 2 * len(plain["rows"]) and st["starts"] == 2 * chains == st["terminated"] + st["truncated"] + st["open"]


def test_nonfinite_rewards_stay_in_their_episode():
    o, a, stride = 17, 6, 4
    five = episodes(SPAN + 1, o, a, stride)
    want = model(five, 0.99, stride)
    long = [int(s) for s in want["rows"] if want["L"][s] >= 9 and want["ends"][s] & rm.START]
    five[2][long[0] + 4 * stride], five[2][long[1] + 6 * stride] = np.nan, np.inf      # (nothing wraps: slot == append order)
    eng, want = new_engine(o, a, five), model(five, 0.99, stride)
    assert (~np.isfinite(want["G"][want["rows"]])).sum() == 5 + 7
    check(eng.returns_to_go(0.99, stride), want, model(five, 1.0, stride), 0.99, "nonfinite")
    assert eng.returns_stats()["rewards_nonfinite"] == 2


def test_range_form_on_a_pinned_prefix_determinism_and_refusals():
    o, a, stride, pin = 70, 2, 4, SPAN + 37
    five = episodes(pin + 500, o, a, stride)
    eng = new_engine(o, a, five)
    eng.rb_pin(pin)
    n = eng.rb_len()
    out = {k: torch.full((n,), -7, dtype=getattr(torch, d), device=DEV) for k, d in P.Engine.RTG_OUT}
    got = eng.returns_to_go(0.99, stride, 0, pin, out=out)
    check(got, model(five, 0.99, stride, first=0, count=pin), model(five, 1.0, stride, first=0, count=pin), 0.99, "pinned prefix")
    assert all(bool((v[pin:] == -7).all()) for v in got.values())
    again = eng.returns_to_go(0.99, stride, 0, pin)
    assert all(same_bits(again[k][:pin].cpu().numpy(), got[k][:pin].cpu().numpy()) for k in got)
    tail = eng.returns_to_go(0.99, stride, pin, n - pin)
    check(tail, model(five, 0.99, stride, first=pin, count=n - pin), model(five, 1.0, stride, first=pin, count=n - pin), 0.99, "live rows")
    before, kept = engine_state(eng), {k: v.clone() for k, v in out.items()}
    host = torch.zeros(n)

    def raw(handle=eng._h, gamma=0.99, stride=stride, first=0, count=pin, io=True, flags=0, **f):
        s = _lib.CReturnsIO(**{"returns": out["returns"].data_ptr(), "returns_ld": 1, **f})
        return eng.lib.sactd3_returns_to_go_device(handle, gamma, stride, first, count, C.byref(s) if io else None, None, flags)

    bad = [dict(handle=None), dict(io=False), dict(returns=None), dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=float("nan")), dict(stride=0),
           dict(stride=CAP + 1), dict(first=-1), dict(count=-1), dict(first=1, count=n), dict(count=n + 1), dict(flags=4), dict(returns_ld=0),
           dict(length=out["length"].data_ptr(), length_ld=0), dict(returns=host.data_ptr())]
    assert [raw(**b) for b in bad] == [_lib.EINVAL] * len(bad)
    assert raw(count=0) == _lib.ESTATE and raw(handle=new_engine(o, a)._h) == _lib.ESTATE
    assert_same_state(before, engine_state(eng))
    assert all(torch.equal(out[k], kept[k]) for k in out) and eng.returns_stats()["calls"] == 3 and raw() == 0


def test_invisible_between_two_periods():
    _, (R, Q), (o, a, bound) = build_engines("sac", (17, 6, 0.5), 64, count=2, seed=3, cap=CAP, max_envs=MAXN)
    five = episodes(CAP + 100, o, a, 4)
    for eng in (R, Q):
        eng.rb_extend(*five)
        it = eng.run_iterations(0, 6)
        if eng is R:
            R.returns_to_go(None, 4)
            R.returns_to_go(1.0, 1, 100, 200)
        eng.run_iterations(it, 6)
    assert_same_state(R, Q, "index", "noise", "ring")


def test_the_data_bias_through_the_agent_and_the_loop():
    """Agent.mc_q_bias is its composition from the model's returns, its own draw, rows and q_values; episode_stats counts the whole
    episodes; loop.train_offline with mc_returns= ends with the bits of the run without the keyword and logs the three vitals"""
    from sac_td3_cudagraphs_pytorch_amd import loop
    o, a, stride, rows, seed = 3, 1, 2, 700, 3
    cfg = P.launcher.job_config("sac", "pendulum", seed, num_envs=2, learning_starts=10, batch_size=4, num_timesteps=100, eval_every=100, rb_capacity=1024)
    five = episodes(rows, o, a, stride)
    runs = []
    for kw in (dict(), dict(mc_returns=dict(rows=64, stride=stride))):
        agent = P.Agent({"ob_shape": (o,), "ac_shape": (a,)}, np.full(a, -0.5, np.float32), np.full(a, 0.5, np.float32), torch.device(DEV),
                        cfg, P.ReplayBuffer(cfg.rb_capacity), seed=seed, init="engine")
        track(agent.engine).rb_extend(*five)
        runs.append((agent, loop.train_offline(cfg, agent, num_updates=20, eval_every_updates=10, **kw)))
    (plain, _), (agent, out) = runs
    assert_same_state(plain.engine, agent.engine, "index", "noise", "ring")
    assert all(np.isfinite(out[k]) for k in loop.McReturns.KEYS) and out["vitals/q_bias_data_rows"] == 64 and agent.engine.returns_stats()["calls"] == 2
    (obs, _, rew, nobs, done), length, cursor = place(five, cfg.rb_capacity)
    g = float(np.float32(agent.engine.cfg.gamma))
    want = rm.returns_to_go(obs, nobs, rew, done, g, stride, length, cursor, cfg.rb_capacity)
    ok = np.flatnonzero(((want["ends"][:rows] & rm.TERMINATED) != 0) | (g ** want["L"][:rows].astype(np.float64) <= 0.05))
    agent._mc_gen = None
    got = agent.mc_q_bias(128, stride, seed=11)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(11)
    index = torch.as_tensor(ok, device=DEV)[torch.randint(0, len(ok), (128,), generator=gen, device=DEV, dtype=torch.int64)]
    rec = agent.rb.rows(index)
    q = agent.q_values({"observations": rec["observations"], "actions": rec["actions"]}).view(2, -1).min(0).values.double().cpu().numpy()
    G = want["G"][index.cpu().numpy()]
    # (a float32 sum of at most 40 rewards of size ~1 lies within (2 x 40 + 8) 2^-24 x 40 x 5 = 1e-3 of the float64 one)
    assert got["rows"] == 128 and got["admitted"] == len(ok)
    assert np.isclose(got["bias_mean"], (q - G).mean(), atol=1e-3) and np.isclose(got["bias_std"], (q - G).std(), atol=1e-3)
    assert np.isclose(got["return_mean"], G.mean(), atol=1e-3) and got["mean"] == got["bias_mean"] / abs(got["return_mean"])
    whole = np.flatnonzero((want["ends"][:rows] & rm.START != 0) & (want["ends"][:rows] & rm.OPEN == 0))
    st = agent.rb.episode_stats(stride)
    assert st["episodes"] == len(whole) and np.isclose(st["return_mean"], want["U"][whole].mean(), atol=1e-3) and np.isclose(st["length_mean"], want["L"][whole].mean())
    assert np.isclose(st["return_min"], want["U"][whole].min(), atol=1e-3) and np.isclose(st["return_max"], want["U"][whole].max(), atol=1e-3)
