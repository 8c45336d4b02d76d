"""CPU: the host side of TD3+BC (include/sactd3.h: sactd3_set_bc) -- header, binding and config; the float64 restatement the GPU
tests compare against (tests/td3bc_ref.py) checked against its own closed form; loop.load_dataset, loop.train_offline and the
launcher's offline switches against fakes.  Nothing here needs a GPU."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sac_td3_cudagraphs_pytorch_amd as P
from sac_td3_cudagraphs_pytorch_amd import _lib, launcher, loop
from sac_td3_cudagraphs_pytorch_amd.engine import Engine
from tests import td3bc_ref as R
from tests.helpers import SlotGeneration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ header, binding, config

def test_header_and_binding_carry_the_bc_surface():
    src = open(os.path.join(ROOT, "include", "sactd3.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("sactd3_set_bc", "sactd3_get_bc"):
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in _lib.SYMBOLS
    assert re.search(r"SACTD3_M_BC_LOSS\s*=\s*4\b", code) and re.search(r"SACTD3_M_BC_LAMBDA\s*=\s*5\b", code)
    assert re.search(r"SACTD3_NUM_METRICS\s*=\s*8\b", code) and re.search(r"#define SACTD3_ABI_VERSION 1\b", code)
    assert re.search(r"float\s+bc_alpha\s*;", code) and "reserved1" not in code
    assert (_lib.M_BC_LOSS, _lib.M_BC_LAMBDA, _lib.NUM_METRICS, _lib.ABI_VERSION) == (4, 5, 8, 1)
    lib = P.load_library()
    assert lib.sactd3_set_bc(None, 2.5, 1.0) == _lib.EINVAL and lib.sactd3_get_bc(None, (C.c_float * 2)()) == _lib.EINVAL


def test_config_field_layout_default_and_from_hps():
    assert _lib.CConfig.bc_alpha.offset == 116 and C.sizeof(_lib.CConfig) == 128 and _lib.CConfig.seed.offset == 120
    lib = P.load_library()
    for td3 in (0, 1):
        cc = _lib.CConfig()
        cc.bc_alpha = 7.0
        lib.sactd3_default_config(C.byref(cc), td3)
        assert cc.bc_alpha == 0.0
    assert P.Config().bc_alpha == 0.0
    assert P.Config.from_hps(SimpleNamespace(prefer_td3_over_sac=True, bc_alpha=2.5), 17, 6).bc_alpha == 2.5
    assert P.Config.from_hps({"prefer_td3_over_sac": True, "bc_alpha": 1.25}, 17, 6).bc_alpha == 1.25
    assert P.Config.from_hps({"prefer_td3_over_sac": True}, 17, 6).bc_alpha == 0.0
    assert P.Config.from_hps(SimpleNamespace(bc_alpha=None), 17, 6).bc_alpha == 0.0
    cc = P.Config(ob_dim=17, ac_dim=6, prefer_td3_over_sac=True, bc_alpha=2.5).to_c()
    assert cc.bc_alpha == 2.5 and cc.abi_version == 1


# ------------------------------------------------------------------------------------------ the restatement against its closed form

@pytest.mark.parametrize("o,a,B,ln,w", [(5, 2, 8, True, 1.0), (13, 7, 11, False, 0.25), (10, 8, 6, True, 0.0)])
def test_restatement_autograd_equals_the_closed_form(o, a, B, ln, w):
    """float64 autograd of L_actor through small random actor and critic modules = lambda (-1/B) dq/da + w 2 (pi - a) / (B A)"""
    from oracle.sac_td3_ref import DetPolicy, QNet
    torch.manual_seed(o * 100 + a)
    lo, hi = -torch.ones(a) * 0.7, torch.ones(a) * 0.7
    actor, q1 = DetPolicy(o, a, lo, hi, 0.1, ln), QNet(o, a, ln)
    obs, act = torch.randn(B, o), (torch.rand(B, a) * 2 - 1) * 0.7
    u = R.actor_update64(actor, q1, obs, act, bc_alpha=2.5, bc_weight=w, lr=3e-4)
    lam = 2.5 / max(float(u["q"].abs().mean()), 1e-8)
    assert u["lam"] == pytest.approx(lam, rel=1e-14)
    want = R.closed_form_dpi(u["dq_da"], u["pi"], act.double(), lam, w)
    scale = float(want.abs().max())
    assert scale > 0 and float((u["dpi"] - want).abs().max()) <= 1e-13 * scale
    assert u["bc"] == pytest.approx(float(((u["pi"] - act.double()) ** 2).sum()) / (B * a), rel=1e-14)
    assert u["loss"] == pytest.approx(-lam * float(u["q"].mean()) + w * u["bc"], rel=1e-13, abs=1e-15)
    # ... and the floor: q == 0 everywhere gives lambda = bc_alpha / 1e-8, finite
    with torch.no_grad():
        q1.head.weight.zero_(); q1.head.bias.zero_()
    z = R.actor_update64(actor, q1, obs, act, bc_alpha=2.5, bc_weight=w, lr=3e-4)
    assert z["lam"] == pytest.approx(2.5e8) and all(torch.isfinite(p).all() for p in z["actor"].parameters())


def test_restatement_shows_the_direction_on_its_own():
    """the experiment of tests/test_gpu_td3bc.py's last test on the oracle's TD3, CPU only, from the seed that test uses: with the BC
    term the policy closes in on the dataset's actions, without it it does not"""
    before, after, first, last = R.offline_direction(R.DIRECTION["bc_alpha"])
    assert last < first and after < before
    p_before, p_after, _, _ = R.offline_direction(0.0)
    assert p_before == before and p_after >= p_before


# ------------------------------------------------------------------------------------------ load_dataset

class RecordingRb:
    def __init__(self, capacity, held=0):
        self.capacity, self.held, self.calls = capacity, held, []

    def extend(self, td):
        assert set(td) == {"observations", "actions", "rewards", "next_observations", "terminations", "dones"}
        self.calls.append({k: np.array(v) for k, v in td.items()})
        self.held += len(td["observations"])

    def __len__(self):
        return self.held


def dataset(n, o=3, a=2, with_dones=False):
    r = np.random.default_rng(n)
    d = dict(observations=r.normal(size=(n, o)).astype(np.float32), actions=r.normal(size=(n, a)).astype(np.float32),
             rewards=r.normal(size=(n, 1)).astype(np.float32), next_observations=r.normal(size=(n, o)).astype(np.float32),
             terminations=r.random(n) < 0.3)
    if with_dones:
        d["dones"] = r.random(n) < 0.5
    return d


@pytest.mark.parametrize("n,chunk", [(10, 4), (8, 4), (3, 65536), (1, 1), (0, 5)])
def test_load_dataset_appends_every_row_once_in_order(n, chunk):
    agent = SimpleNamespace(rb=RecordingRb(capacity=16, held=2))
    d = dataset(n)
    assert loop.load_dataset(agent, d, chunk=chunk) == n
    calls = agent.rb.calls
    assert [len(c["observations"]) for c in calls] == [min(chunk, n - lo) for lo in range(0, n, chunk)]      # the chunk boundaries
    for k in ("observations", "actions", "rewards", "next_observations", "terminations"):
        got = np.concatenate([c[k] for c in calls]) if calls else d[k][:0]
        assert np.array_equal(got, d[k]), k
    if calls:
        assert np.array_equal(np.concatenate([c["dones"] for c in calls]), d["terminations"])      # dones defaults to terminations


def test_load_dataset_keeps_dones_apart_and_refuses_what_does_not_fit():
    agent = SimpleNamespace(rb=RecordingRb(capacity=16))
    d = dataset(9, with_dones=True)
    loop.load_dataset(agent, d, chunk=5)
    assert np.array_equal(np.concatenate([c["dones"] for c in agent.rb.calls]), d["dones"])
    assert np.array_equal(np.concatenate([c["terminations"] for c in agent.rb.calls]), d["terminations"])
    with pytest.raises(ValueError, match="do not fit"):      # 9 held + 8 > 16: the ring would wrap
        loop.load_dataset(agent, dataset(8))
    assert len(agent.rb.calls) == 2 and len(agent.rb) == 9      # nothing was appended by the refused call
    loop.load_dataset(agent, dataset(7))                        # exactly full is fine
    assert len(agent.rb) == 16
    with pytest.raises(ValueError, match="missing"):
        loop.load_dataset(agent, {k: v for k, v in dataset(1).items() if k != "rewards"})
    bad = dataset(4)
    bad["actions"] = bad["actions"][:3]
    with pytest.raises(ValueError, match="disagree"):
        loop.load_dataset(SimpleNamespace(rb=RecordingRb(64)), bad)
    with pytest.raises(ValueError, match="chunk"):
        loop.load_dataset(SimpleNamespace(rb=RecordingRb(64)), dataset(4), chunk=0)


# ------------------------------------------------------------------------------------------ train_offline

class FakeEngine(SlotGeneration):
    """records run_iterations calls and expands them with Engine.run_iterations' own routing"""

    def __init__(self, delay=2, td3=True):
        self.cfg = SimpleNamespace(actor_update_delay=delay, prefer_td3_over_sac=td3, crit_targ_update_freq=1)
        self.runs, self.calls = [], []

    step = lambda self, a: self.calls.append(("step", bool(a)))
    step_period = lambda self: self.calls.append(("period",))
    step_prefix = lambda self, m: self.calls.append(("prefix", m))
    step_periods = lambda self, k: self.calls.append(("periods", k))

    def run_iterations(self, i0, n):
        self.runs.append((i0, n))
        self.slot_refilled()
        return Engine.run_iterations(self, i0, n)

    def read_metrics(self):
        return {"loss/qf_loss": 1.0, "n": len(self.runs)}


def fake_agent(delay=2):
    return SimpleNamespace(engine=FakeEngine(delay), qnet_updates_so_far=0, actor_updates_so_far=0, timesteps_so_far=123)


@pytest.mark.parametrize("delay", [2, 1, 3])
@pytest.mark.parametrize("num,every", [(0, None), (1, None), (7, None), (12, None), (12, 4), (13, 5), (10, 3), (6, 6), (5, 10), (9, 1)])
def test_train_offline_cuts_runs_at_evaluation_points_and_keeps_the_counters(delay, num, every):
    agent, evals, seen = fake_agent(delay), [], []
    out = loop.train_offline(SimpleNamespace(), agent, num_updates=num, eval_every_updates=every,
                             evaluator=lambda ag: evals.append(ag.qnet_updates_so_far), on_eval=lambda ag, n: seen.append(n))
    runs = agent.engine.runs
    # the runs tile [0, num) in order, each ends at a multiple of `every` or at num, and none crosses one
    assert [r[0] for r in runs] == [sum(n for _, n in runs[:k]) for k in range(len(runs))] and sum(n for _, n in runs) == num
    step = every if every is not None else max(num, 1)
    points = sorted(set(list(range(step, num + 1, step)) + ([num] if num else [])))
    assert [i0 + n for i0, n in runs] == points
    assert evals == points and seen == points                   # evaluated where the runs end, with the counters already advanced
    period = delay + 1
    assert agent.qnet_updates_so_far == num
    assert agent.actor_updates_so_far == delay * len([i for i in range(num) if i % period == 0])      # as Agent.iteration counts
    assert agent.timesteps_so_far == 123                        # no env step was taken
    assert agent.engine.batch_generation() == 5 + len(runs)     # run_iterations itself counts the new rows, not the loop
    assert out == {"loss/qf_loss": 1.0, "n": len(runs)}
    # the iterations issued are exactly 0 .. num - 1 with the actor updates at the multiples of the period
    i = 0
    for c in agent.engine.calls:
        if c[0] == "periods":
            assert i % period == 0
            i += period * c[1]
        elif c[0] == "period":
            assert i % period == 0
            i += period
        elif c[0] == "prefix":
            assert i % period == 0
            i += c[1]
        else:
            assert c[1] == (i % period == 0)
            i += 1
    assert i == num


def test_train_offline_refuses_bad_arguments():
    with pytest.raises(ValueError, match="num_updates"):
        loop.train_offline(SimpleNamespace(), fake_agent(), num_updates=-1)
    with pytest.raises(ValueError, match="eval_every_updates"):
        loop.train_offline(SimpleNamespace(), fake_agent(), num_updates=4, eval_every_updates=0)


# ------------------------------------------------------------------------------------------ launcher wiring

def launcher_args(**kw):
    base = dict(algo="td3", offline_dataset=None, bc_alpha=None, num_updates=None, overlap_acting=False, device_env=False,
                prioritized=False, one_launch=False, n_step=1)
    base.update(kw)
    return SimpleNamespace(**base)


def test_launcher_offline_plan():
    assert launcher.offline_plan(launcher_args()) is None
    assert launcher.offline_plan(launcher_args(bc_alpha=2.5)) is None                      # online TD3 with the BC term: allowed
    p = launcher.offline_plan(launcher_args(offline_dataset="d.npz", bc_alpha=2.5, num_updates=300))
    assert p == dict(dataset="d.npz", num_updates=300, bc_alpha=2.5, plain=False)
    # a dataset without --bc_alpha: plain TD3 / plain SAC on a fixed ring, accepted and flagged
    assert launcher.offline_plan(launcher_args(offline_dataset="d.npz")) == dict(dataset="d.npz", num_updates=None, bc_alpha=0.0, plain=True)
    assert launcher.offline_plan(launcher_args(algo="sac", offline_dataset="d.npz"))["plain"] is True
    with pytest.raises(ValueError, match="--algo td3"):                                    # SAC has no BC form
        launcher.offline_plan(launcher_args(algo="sac", offline_dataset="d.npz", bc_alpha=2.5))
    with pytest.raises(ValueError, match="--algo td3"):
        launcher.offline_plan(launcher_args(algo="sac", bc_alpha=2.5))
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="bc_alpha"):
            launcher.offline_plan(launcher_args(offline_dataset="d.npz", bc_alpha=bad))
    with pytest.raises(ValueError, match="needs --offline_dataset"):
        launcher.offline_plan(launcher_args(num_updates=5))
    with pytest.raises(ValueError, match="num_updates"):
        launcher.offline_plan(launcher_args(offline_dataset="d.npz", num_updates=0))
    with pytest.raises(ValueError, match="excludes --prioritized, --n_step"):
        launcher.offline_plan(launcher_args(offline_dataset="d.npz", prioritized=True, n_step=3))


def test_launcher_command_line_refuses_bc_alpha_on_sac_before_any_worker_starts(capsys):
    with pytest.raises(SystemExit) as ex:
        launcher.main(["--algo", "sac", "--offline_dataset", "d.npz", "--bc_alpha", "2.5"])
    assert ex.value.code == 2 and "--algo td3" in capsys.readouterr().err
    assert launcher.job_config("td3", "HalfCheetah-v4", 0, bc_alpha=2.5).bc_alpha == 2.5       # hps carries it to Config.from_hps
    assert not hasattr(launcher.job_config("td3", "HalfCheetah-v4", 0, bc_alpha=None), "bc_alpha")
