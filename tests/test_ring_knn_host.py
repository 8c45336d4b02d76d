"""CPU: the host side of the nearest-ring-rows call (include/sactd3_ring_knn.h) -- the header, the binding and the built library cover
each other; its kernels live in a translation unit of their own; the keyword rule of `knn` in loop.train /
loop.train_offline and the launcher's flags, each asked before an agent is touched; the brute-force model against a plain loop."""
import ctypes as C
import glob
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import sac_td3_cudagraphs_pytorch_amd as P
from sac_td3_cudagraphs_pytorch_amd import _lib, launcher, loop
from tests import ring_knn_model as km

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sac-td3-cudagraphs-pytorch_amd", "csrc")
CFG = dict(seed=0, learning_starts=10, action_repeat=1, segment_len=1, num_envs=2, num_timesteps=10, eval_every=10, batch_size=4,
           actor_update_delay=2)


class Untouchable:      # an agent (an env) that fails on any attribute access: a refusal must come before either is touched
    def __getattr__(self, name):
        raise AssertionError(f"touched .{name} before the refusal")


def test_header_binding_and_library_cover_each_other(tmp_path):
    with open(os.path.join(ROOT, "include", "sactd3_ring_knn.h")) as f:
        code = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sactd3_[a-z0-9_]+)\s*\(", code))) == sorted(_lib.RING_KNN_SYMBOLS)
    struct = re.search(r"typedef struct sactd3_ring_knn_io \{(.*?)\}", code, re.S).group(1)
    assert re.findall(r"(\w+);", struct) == [n for n, _ in _lib.CRingKnnIO._fields_]
    assert int(re.search(r"SACTD3_KNN_MAX_K\s+(\d+)", code).group(1)) == _lib.KNN_MAX_K
    assert int(re.search(r"SACTD3_KNN_MAX_D\s+(\d+)", code).group(1)) == _lib.KNN_MAX_D and _lib.ABI_VERSION == 1
    assert not set(_lib.RING_KNN_SYMBOLS) & set(_lib.SYMBOLS)
    probe = tmp_path / "probe.c"
    probe.write_text('#include "sactd3_ring_knn.h"\nint main(void) { return sizeof(sactd3_ring_knn_io) == 0; }\n')
    subprocess.run(["cc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(probe)], check=True)
    lib = P.load_library()
    assert lib.sactd3_ring_knn_device(None, None, 1, 1, 1, 0, 0, 0, C.byref(_lib.CRingKnnIO()), None, 0) == _lib.EINVAL
    assert lib.sactd3_ring_knn_stats(None, (C.c_int64 * 8)()) == _lib.EINVAL


def test_the_kernels_live_in_their_own_unit():
    where = {}
    for path in glob.glob(os.path.join(CSRC, "*")):
        with open(path) as f:
            for name in re.findall(r"__global__[^;{]*?\b(k_knn_\w+)\s*\(", f.read()):
                where.setdefault(name, set()).add(os.path.basename(path))
    assert where == {k: {"ring_knn_kernels.h"} for k in ("k_knn_scan", "k_knn_finish", "k_knn_count")}
    with open(os.path.join(CSRC, "engine.hip")) as f:
        assert not re.search(r"hipLaunchKernelGGL\(\s*k_knn_", f.read())


def test_the_model_against_a_plain_loop():
    g = np.random.default_rng(0)
    q, x, c, w = g.normal(size=(3, 5)), g.normal(size=(9, 5)), g.normal(size=5), g.uniform(0.5, 2.0, size=5)
    x[7] = x[2]
    index, dist2, _, _ = km.knn(q, x, 4, c, w, exclude=[2, -1, 0], first=1, last=8)
    for i in range(3):
        d = [(sum(((q[i, j] - c[j]) * w[j] - (x[s, j] - c[j]) * w[j]) ** 2 for j in range(5)), s) for s in range(1, 8) if s != [2, -1, 0][i]]
        want = sorted(d)[:4]
        assert [s for _, s in want] == index[i].tolist() and np.allclose([v for v, _ in want], dist2[i], rtol=1e-12)
    short = km.knn(q, x[:2], 4)
    assert (short[0][:, 2:] == -1).all() and np.isinf(short[1][:, 2:]).all()


BAD = [(dict(k=5), "rows"), (dict(rows=0), "rows"), (dict(rows=64, k=17), "k"), (dict(rows=64, beta=0.0), "beta"),
       (dict(rows=64, beta=float("nan")), "beta"), (dict(rows=64, tau=1.0), "must be a dict")]


@pytest.mark.parametrize("spec,word", BAD, ids=[str(i) for i in range(len(BAD))])
def test_bad_keywords_are_refused_before_an_agent_is_touched(spec, word):
    cfg = SimpleNamespace(**CFG)
    with pytest.raises(ValueError, match=word):
        loop.train(cfg, Untouchable(), Untouchable(), knn=spec)
    with pytest.raises(ValueError, match=word):
        loop.train_offline(cfg, Untouchable(), num_updates=100, knn=spec)


def test_off_makes_no_call_on_records_the_vitals_and_the_launcher_maps_the_flags():
    calls = []
    engine = SimpleNamespace(cfg=SimpleNamespace(actor_update_delay=2, prefer_td3_over_sac=False), read_metrics=lambda: {}, run_iterations=lambda i, n: None)
    got = {"knn_state_entropy": 0.5, "knn_policy_distance": 0.25}
    agent = SimpleNamespace(engine=engine, qnet_updates_so_far=0, actor_updates_so_far=0, knn_vitals=lambda **kw: calls.append(kw) or got)
    out = loop.train_offline(SimpleNamespace(**CFG), agent, num_updates=20, eval_every_updates=10)
    assert not calls and not any(k.startswith("vitals/knn") for k in out)
    out = loop.train_offline(SimpleNamespace(**CFG), agent, num_updates=20, eval_every_updates=10, knn=dict(rows=64, k=3, beta=1.5))
    assert calls == [dict(rows=64, k=3, beta=1.5)] * 2
    assert {k: out[k] for k in loop.Knn.KEYS} == {"vitals/knn_state_entropy": 0.5, "vitals/knn_policy_distance": 0.25}
    cfg = launcher.job_config("sac", None, 0)
    base = dict(prioritized=False, n_step=1, one_launch=False, prior_fraction=None, updates_per_step=1, overlap_acting=False, device_env=False,
                native_rollout=False, policy_stats=0)
    plain = launcher.train_keywords(cfg, **base)
    kw = launcher.train_keywords(cfg, **base, knn=256, knn_k=3, knn_beta=1.5)
    assert "knn" not in plain and kw["knn"] == dict(rows=256, k=3, beta=1.5) and {k: v for k, v in kw.items() if k != "knn"} == plain
    for bad in (dict(knn_k=2), dict(knn_beta=0.1), dict(knn=256, knn_k=20)):
        with pytest.raises(ValueError, match="knn|k"):
            launcher.train_keywords(cfg, **base, **bad)
