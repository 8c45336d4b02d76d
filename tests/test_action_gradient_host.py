"""CPU: the host side of the action-gradient call (include/sactd3_action_gradient.h) -- the header, the binding and the built library
cover each other; the keyword rule of `action_grad` in loop.train / loop.train_offline and the launcher's flags, each asked before an
agent is touched."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import pytest

import sac_td3_cudagraphs_pytorch_amd as P
from sac_td3_cudagraphs_pytorch_amd import _lib, launcher, loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(seed=0, learning_starts=10, action_repeat=1, segment_len=1, num_envs=2, num_timesteps=10, eval_every=10, batch_size=4,
           actor_update_delay=2)


class Untouchable:      # an agent (an env) that fails on any attribute access: a refusal must come before either is touched
    def __getattr__(self, name):
        raise AssertionError(f"touched .{name} before the refusal")


def test_header_binding_and_library_cover_each_other(tmp_path):
    header = os.path.join(ROOT, "include", "sactd3_action_gradient.h")
    with open(header) as f:
        code = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sactd3_[a-z0-9_]+)\s*\(", code))) == sorted(_lib.ACTION_GRADIENT_SYMBOLS)
    struct = re.search(r"typedef struct sactd3_action_gradient_io \{(.*?)\}", code, re.S).group(1)
    assert re.findall(r"(\w+);", struct) == [n for n, _ in _lib.CActionGradientIO._fields_]
    assert int(re.search(r"SACTD3_AG_MAX_STEPS\s+(\d+)", code).group(1)) == _lib.AG_MAX_STEPS
    assert len(_lib.AG_SUMMARY) == int(re.search(r"SACTD3_AG_SUMMARY\s+(\d+)", code).group(1)) == 8 and _lib.ABI_VERSION == 1
    assert not set(_lib.ACTION_GRADIENT_SYMBOLS) & set(_lib.SYMBOLS)
    probe = tmp_path / "probe.c"
    probe.write_text('#include "sactd3_action_gradient.h"\nint main(void) { return sizeof(sactd3_action_gradient_io) == 0; }\n')
    subprocess.run(["cc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(probe)], check=True)
    lib = P.load_library()
    assert lib.sactd3_action_gradient_device(None, None, 1, None, 1, 1, 0, 0, 0.0, C.byref(_lib.CActionGradientIO()), None, 0) == _lib.EINVAL
    assert lib.sactd3_action_gradient_stats(None, (C.c_int64 * 8)()) == _lib.EINVAL


BAD = [(dict(steps=4), "rows"), (dict(rows=0), "rows"), (dict(rows=64, steps=17), "steps"), (dict(rows=64, lr=-0.1), "lr"),
       (dict(rows=64, lr=float("nan")), "lr"), (dict(rows=64, tau=1.0), "must be a dict")]


@pytest.mark.parametrize("spec,word", BAD, ids=[str(i) for i in range(len(BAD))])
def test_bad_keywords_are_refused_before_an_agent_is_touched(spec, word):
    cfg = SimpleNamespace(**CFG)
    with pytest.raises(ValueError, match=word):
        loop.train(cfg, Untouchable(), Untouchable(), action_grad=spec)
    with pytest.raises(ValueError, match=word):
        loop.train_offline(cfg, Untouchable(), num_updates=100, action_grad=spec)


def test_off_makes_no_call_and_on_records_the_vitals():
    calls = []
    engine = SimpleNamespace(cfg=SimpleNamespace(actor_update_delay=2, prefer_td3_over_sac=False), read_metrics=lambda: {}, run_iterations=lambda i, n: None)
    got = {"action_grad_norm": 0.5, "action_grad_cos": 0.25, "refine_gain": 0.125}
    agent = SimpleNamespace(engine=engine, qnet_updates_so_far=0, actor_updates_so_far=0, critic_smoothness=lambda **kw: calls.append(kw) or got)
    out = loop.train_offline(SimpleNamespace(**CFG), agent, num_updates=20, eval_every_updates=10)
    assert not calls and not any(k.startswith("vitals/action_grad") or k == "vitals/refine_gain" for k in out)
    out = loop.train_offline(SimpleNamespace(**CFG), agent, num_updates=20, eval_every_updates=10, action_grad=dict(rows=64, steps=2, lr=0.1))
    assert calls == [dict(rows=64, steps=2, lr=0.1)] * 2
    assert {k: out[k] for k in loop.ActionGrad.KEYS} == {"vitals/action_grad_norm": 0.5, "vitals/action_grad_cos": 0.25, "vitals/refine_gain": 0.125}


def test_the_launcher_maps_the_flags():
    cfg = launcher.job_config("sac", None, 0)
    base = dict(prioritized=False, n_step=1, one_launch=False, prior_fraction=None, updates_per_step=1, overlap_acting=False, device_env=False,
                native_rollout=False, policy_stats=0)
    plain = launcher.train_keywords(cfg, **base)
    kw = launcher.train_keywords(cfg, **base, action_grad=256, action_grad_steps=2, action_grad_lr=0.1)
    assert "action_grad" not in plain and kw["action_grad"] == dict(rows=256, steps=2, lr=0.1)
    assert {k: v for k, v in kw.items() if k != "action_grad"} == plain
    assert launcher.train_keywords(cfg, **base, action_grad=8)["action_grad"] == dict(rows=8)
    for bad in (dict(action_grad_steps=2), dict(action_grad_lr=0.1), dict(action_grad=256, action_grad_steps=20)):
        with pytest.raises(ValueError, match="action_grad|steps"):
            launcher.train_keywords(cfg, **base, **bad)
