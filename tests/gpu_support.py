"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  What two or more GPU test modules share, once: the package handles, the shape tables,
one engine builder whose engines are closed when the test ends, one definition of "the same bits", one definition of "the state
an engine is left in", and the small helpers around the C ABI.  A helper only one module uses stays in that module; no test module
imports another (tests/test_host_logic.py checks that).

This is not a test module, so pytest does not rewrite its asserts: every assert here carries its own message tuple."""
import ctypes as C
import functools
from collections.abc import Mapping

import numpy as np
import pytest
import torch

from oracle.sac_td3_ref import Hps, RefAgent
from tests.helpers import DIMS, randomize_ln, synth_transitions

P = pytest.importorskip("sac_td3_cudagraphs_pytorch_amd")
from sac_td3_cudagraphs_pytorch_amd import _lib, agent as agent_mod, loop, schema  # noqa: E402, F401

DEV = "cuda:0"
PARAM_SETS = {"actor": _lib.ACTOR, "critics": _lib.CRITICS, "actor_target": _lib.ACTOR_TARGET, "critics_target": _lib.CRITICS_TARGET,
              "log_alpha": _lib.LOG_ALPHA}
SETS = tuple(PARAM_SETS.values())
OPTIMISERS = {"actor": _lib.ACTOR, "critics": _lib.CRITICS, "log_alpha": _lib.LOG_ALPHA}

# ------------------------------------------------------------------------------------------ shape tables
MAXN = 96                     # max_envs of the engines that act on, score or query many rows
NROWS = 1041                  # the rows of data(): a chunk of 1024 and one of 17
SENTINEL = -12345.678
# name -> (algo, (o, a, bound), layer_norm)
SHAPES = {"sac-hopper": ("sac", DIMS["hopper"], True), "td3-halfcheetah": ("td3", DIMS["halfcheetah"], True),
          "sac-humanoid": ("sac", DIMS["humanoid"], True), "sac-hopper-noln": ("sac", DIMS["hopper"], False),
          "sac-k64": ("sac", (47, 17, 0.7), True), "sac-k65": ("sac", (48, 17, 0.7), True), "td3-td3_2": ("td3", DIMS["td3_2"], True)}
# shapes for the places a pack kernel can go wrong: o % 4 = 1 and a one-line record; o % 4 = 3 with s|a ending inside a chunk;
# o % 4 = 0 with an odd a; an action wider than the observation; 196 chunks per record
PACK_SHAPES = ["td3_2", "hopper", "o48a17", "o3a32", "humanoid"]
# the engine-owned priorities and the one-launch iteration: name -> (shape, batch size); a 5000-slot ring that holds 2500 rows
PRIO_CASES = {"sac-hopper-64": ("sac-hopper", 64), "sac-hopper-40": ("sac-hopper", 40), "td3-halfcheetah-64": ("td3-halfcheetah", 64),
              "sac-hopper-1024": ("sac-hopper", 1024)}
CAP, HELD, SEED = 5000, 2500, 3          # (SEED: the Philox key of shape_engines())
# the largest relative difference between the device's float32 weights / leaves and the float64 restatement, measured on an MI355X
# over every case of tests/test_gpu_native_priorities.py tests 4 and 6, and the bound applied: 8 x the measured value, never above 1e-4
MEASURED_REL = {"weights": 2.215e-7, "leaves": 1.293e-7}      # (both at sac-hopper-1024; bounds 1.77e-6 and 1.03e-6)
BOUND_REL = {k: min(8.0 * v, 1e-4) for k, v in MEASURED_REL.items()}


# ------------------------------------------------------------------------------------------ engines, closed when the test ends
_OPEN = []      # the engines of the running test


def track(eng):
    """register an engine (or anything with close()) made outside the builder, an Agent's for instance; -> eng"""
    _OPEN.append(eng)
    return eng


@pytest.fixture(autouse=True)
def close_engines():
    """every engine a test made is destroyed when the test ends, passed or not (Engine.close() is idempotent).  Autouse in every
    module that imports it by name."""
    yield
    while _OPEN:
        _OPEN.pop().close()


def new_engine(hps, dims, **cfg):
    """one tracked engine of Config.from_hps(hps, o, a, **cfg) with symmetric action bounds; no parameters are set"""
    o, a, bound = dims
    return track(P.Engine(P.Config.from_hps(hps, o, a, **cfg), [-bound] * a, [bound] * a))


def build_engines(algo, dims, B, *, ln=True, count=1, seed=0, cap=4096, max_envs=8, use_graphs=True, randomize=True, push=True, **fields):
    """Hps -> RefAgent -> randomize_ln -> Config.from_hps -> Engine -> push_params, once.  -> (the oracle, [engines], dims).
    torch is seeded with `seed` before the oracle draws its parameters; `seed` is also the engines' Philox key.  `fields`: further
    Hps fields (clip_norm, actor_update_delay, ...) and Config fields (bc_alpha, ...).  use_graphs may be a sequence, one entry per
    engine.  randomize=False keeps the oracle's initial parameters; push=False leaves the engines' parameters alone."""
    hp = {k: fields.pop(k) for k in list(fields) if k in Hps.__dataclass_fields__}
    hps = (Hps.td3 if algo == "td3" else Hps.sac)(layer_norm=ln, batch_size=B, **hp)
    o, a, bound = dims
    torch.manual_seed(seed)
    ref = RefAgent(o, a, [-bound] * a, [bound] * a, hps)
    if randomize:
        randomize_ln(ref)
    engs = []
    for graphs in (use_graphs if isinstance(use_graphs, (tuple, list)) else (use_graphs,) * count):
        engs.append(new_engine(hps, dims, rb_capacity=cap, max_envs=max_envs, seed=seed, use_graphs=graphs, **fields))
        if push:
            push_params(engs[-1], ref)
    return ref, engs, dims


def make_pair(algo, env, B, ln=True, seed=0, use_graphs=True, rb_capacity=4096, **hp):
    """the oracle and one engine with its parameters at the dimensions of helpers.DIMS[env]"""
    ref, (eng,), dims = build_engines(algo, DIMS[env], B, ln=ln, seed=seed, cap=rb_capacity, use_graphs=use_graphs, **hp)
    return ref, eng, dims


def shape_engines(shape, count=1, B=64, seed=3, cap=2048, **kw):
    """the oracle and `count` engines with its (perturbed, so that every parameter matters) parameters, at a shape of SHAPES"""
    algo, dims, ln = SHAPES[shape]
    return build_engines(algo, dims, B, ln=ln, count=count, seed=seed, cap=cap, max_envs=MAXN, **kw)


def make_engine(c, log_alpha=None, bcq=None, rb_capacity=None, bc_alpha=0.0):
    """an engine for a case of tests/tail_checks.py:make_case: parameters drawn directly (no torch oracle), per-dimension bounds"""
    sac = c["sac"]
    cfg = P.Config(ob_dim=c["o"], ac_dim=c["a"], batch_size=c["B"], rb_capacity=rb_capacity or max(4096, c["B"]), max_envs=8,
                   prefer_td3_over_sac=not sac, layer_norm=c["ln"], bcq_style_targ_mix=(not sac) if bcq is None else bcq,
                   qnets_lr=1e-3 if sac else 3e-4, bc_alpha=bc_alpha, seed=0)
    eng = track(P.Engine(cfg, c["lo"], c["hi"]))
    flat = lambda p, i, n: schema.dict_to_flat(p, i, n, c["ln"])
    eng.set_params(_lib.ACTOR, flat(c["actor"], c["o"], c["nh"]))
    eng.set_params(_lib.ACTOR_TARGET, flat(c["actor_t"], c["o"], c["nh"]))
    eng.set_params(_lib.CRITICS, np.concatenate([flat(p, c["o"] + c["a"], 1) for p in c["critics"]]))
    eng.set_params(_lib.CRITICS_TARGET, np.concatenate([flat(p, c["o"] + c["a"], 1) for p in c["critics_t"]]))
    if sac and log_alpha is not None:
        eng.set_params(_lib.LOG_ALPHA, np.array([log_alpha], np.float32))
    return eng


def flat_actor(ref, module):
    nh = ref.ac_dim if ref.hps.prefer_td3_over_sac else 2 * ref.ac_dim
    sd = {k: v for k, v in module.state_dict().items() if k.startswith(("fc_stack", "head"))}
    return schema.dict_to_flat(sd, ref.ob_dim, nh, ref.hps.layer_norm)


def flat_critics(ref, modules):
    return np.concatenate([schema.dict_to_flat(m.state_dict(), ref.ob_dim + ref.ac_dim, 1, ref.hps.layer_norm) for m in modules])


def push_params(eng, ref):
    eng.set_params(_lib.ACTOR, flat_actor(ref, ref.actor))
    eng.set_params(_lib.ACTOR_TARGET, flat_actor(ref, ref.actor_target))
    eng.set_params(_lib.CRITICS, flat_critics(ref, ref.qnets))
    eng.set_params(_lib.CRITICS_TARGET, flat_critics(ref, ref.qnets_target))
    if ref.log_alpha is not None:
        eng.set_params(_lib.LOG_ALPHA, np.array([float(ref.log_alpha)], np.float32))


def crit_layout(ref):
    return (ref.ob_dim + ref.ac_dim, 1, ref.hps.layer_norm, 2)


def actor_layout(ref):
    return (ref.ob_dim, ref.ac_dim if ref.hps.prefer_td3_over_sac else 2 * ref.ac_dim, ref.hps.layer_norm, 1)


# ------------------------------------------------------------------------------------------ the same bits
def same_bits(x, y):
    """the same shape, the same dtype and the same bytes: -0.0 differs from +0.0, a NaN equals the same NaN pattern, float32 differs
    from float64.  Nothing is cast; a call site whose sides differ in dtype on purpose casts one of them itself."""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()


def assert_same_bits(x, y, keys=None, what=""):
    """two mappings of arrays, key by key (every key of x, or `keys`)"""
    for k in keys or x:
        assert same_bits(np.asarray(x[k]), np.asarray(y[k])), (what, k)


# ------------------------------------------------------------------------------------------ the state an engine is left in
STATE_PARTS = ("index", "slot", "noise", "td", "prio", "ring")


def engine_state(eng, *parts, extra=None):
    """name -> array, in a fixed order: what a sequence of calls leaves in an engine.  Always: the five parameter sets; m, v, t of
    the three optimisers (log alpha's where the engine serves it); every metric.  `parts` add
        "index"  the ring indices of the batch slot            "slot"   the whole read_batch(), indices included
        "noise"  the critic site's draws                        "td"     the TD errors of the last critic update
        "prio"   prio_leaf, prio_sums, prio_max and the prio_stats counters
        "ring"   every ring row, through rb_sample_with_indices + read_batch, and the ring's length.  THIS PART CONSUMES THE BATCH
                 SLOT: it is read last, and the engine's slot afterwards holds the ring's last rows.
    `extra`: further arrays of the caller's own (counters, a ring read another way, ...)."""
    assert set(parts) <= set(STATE_PARTS), ("engine_state", "unknown part", sorted(set(parts) - set(STATE_PARTS)))
    out = {f"params.{name}": eng.get_params(which) for name, which in PARAM_SETS.items()}
    for name, which in OPTIMISERS.items():
        try:
            m, v, t = eng.get_adam_state(which)
        except P.EngineError:
            if which != _lib.LOG_ALPHA:
                raise
            continue
        out[f"adam_m.{name}"], out[f"adam_v.{name}"], out[f"adam_t.{name}"] = np.asarray(m), np.asarray(v), np.array([t], np.int64)
    for k, v in eng.read_metrics().items():
        out[f"metrics.{k}"] = np.array([v], np.float32)      # (read_metrics widens the engine's float32 slots: exact both ways)
    if "slot" in parts:
        out.update({f"slot.{k}": v for k, v in eng.read_batch().items()})
    elif "index" in parts:
        out["slot.index"] = eng.read_batch()["index"]
    if "noise" in parts:
        out["noise.critic"] = eng.read_noise(_lib.SITE_CRITIC)
    if "td" in parts:
        out["td"] = td_of(eng)
    if "prio" in parts:
        for k in ("prio_leaf", "prio_sums", "prio_max"):
            out[k] = eng.debug_read(k)
        out["prio_stats"] = np.array(list(eng.prio_stats().values()), np.int64)
    if "ring" in parts:
        n, bs = eng.rb_len(), eng.cfg.batch_size
        out["ring.len"] = np.array([n], np.int64)
        blocks = []
        for lo in range(0, n, bs):                                   # index sets that cover every row
            eng.rb_sample_with_indices(np.minimum(np.arange(lo, lo + bs), n - 1))
            blocks.append(eng.read_batch())
        for k in (blocks[0] if blocks else ()):
            out[f"ring.{k}"] = np.concatenate([b[k] for b in blocks])
    for k, v in (extra or {}).items():
        assert k not in out, ("engine_state", "extra key shadows a state key", k)
        out[k] = np.asarray(v)
    return out


def assert_same_state(A, B, *parts, what=""):
    """two engines (their engine_state(., *parts)) or two states taken earlier: the same keys, and per key the same bits AND
    np.array_equal -- the first tells -0.0 from +0.0, the second keeps a NaN on both sides a failure."""
    x, y = (s if isinstance(s, Mapping) else engine_state(s, *parts) for s in (A, B))
    assert list(x) == list(y), (what, "keys", sorted(set(x) ^ set(y)))
    for k in x:
        assert same_bits(x[k], y[k]) and np.array_equal(x[k], y[k]), (what, k)


# ------------------------------------------------------------------------------------------ numeric closeness against the oracle
def close(got, want, rtol=1e-5, atol=1e-5, name=""):
    got = np.asarray(got, np.float32)
    want = want.detach().cpu().numpy() if hasattr(want, "detach") else np.asarray(want, np.float32)
    np.testing.assert_allclose(got.reshape(want.shape), want, rtol=rtol, atol=atol, err_msg=name)


def gclose(got, want, name=""):
    want = want.detach().cpu().numpy() if hasattr(want, "detach") else np.asarray(want, np.float32)
    close(got, want, rtol=2e-4, atol=2e-6 + 1e-5 * float(np.abs(want).max()), name=name)


def logp_close(got, want, action, scale, bias, name=""):
    """per-sample log pi(a|s) (agents/nets.py:228-231).  The tanh correction log(scale (1 - y^2) + 1e-6) is ill-conditioned where
    the squashed action saturates: an error of one or two fp32 ulps in y = tanh(x) (two correct tanh implementations differ by
    that) moves the term by 2.4e-7 scale |y| / (scale (1 - y^2) + 1e-6) -- 1e-3 at 1 - y^2 = 1e-4.  The bound per sample is the
    usual rtol 1e-5 + atol 2e-5 plus that conditioning term summed over the action dimensions, computed from the oracle's own
    action; the batch MEAN of logp, which is what enters the losses, is checked at 1e-5 through the loss values."""
    want = want.detach().cpu().numpy() if hasattr(want, "detach") else np.asarray(want, np.float32)
    action = action.detach().cpu().numpy() if hasattr(action, "detach") else np.asarray(action, np.float32)
    y = np.clip((action.astype(np.float64) - bias) / scale, -1.0, 1.0)
    cond = (2.4e-7 * scale * np.abs(y) / (scale * (1.0 - y * y) + 1e-6)).sum(1)
    got, want = np.asarray(got, np.float64).reshape(-1), want.astype(np.float64).reshape(-1)
    bad = np.abs(got - want) > 2e-5 + 1e-5 * np.abs(want) + cond
    assert not bad.any(), (name, int(bad.sum()), float(np.abs(got - want)[bad].max()), float(cond[bad].min()))
    return cond


# ------------------------------------------------------------------------------------------ rows, and the device boundary
def stream():
    return torch.cuda.current_stream().cuda_stream


def rows(n, o, a, bound, seed, first=0):
    """n transitions whose every 7th flag (counted from row `first` of the run) is done"""
    obs, act, rew, nobs, _ = synth_transitions(n, o, a, bound, seed=seed)
    done = (torch.arange(first, first + n) % 7) == 0
    return obs, act, rew, nobs, done


def cuda(five):
    return tuple(t.to(DEV) for t in five)


def fields_of(eng, five):
    """(fields, n, keep) of five CUDA tensors, through the mirror's own routing helper"""
    got = agent_mod._device_route(eng, *five)
    assert got is not None, ("fields_of", "the routing helper sent CUDA tensors down the host route")
    return got


def extend_device(eng, five):
    fields, n, keep = fields_of(eng, five)
    eng.rb_extend_fields_device(fields, n, stream())


def load_device(eng, five):
    fields, n, keep = fields_of(eng, five)
    eng.load_batch_device(fields, n, stream())


@functools.lru_cache(maxsize=None)
def data(shape):
    """(obs, act) [1041, .] on the host: computed once per shape, never written"""
    _, (o, a, bound), _ = SHAPES[shape]
    obs, act = synth_transitions(NROWS, o, a, bound, seed=5)[:2]
    return obs, act


def score(eng, obs, act=None, target=False):
    """q_values_device on CUDA tensors -> [2, n] on the host (read on the current stream, which the call made wait)"""
    n = obs.shape[0]
    out = torch.empty(2, n, device=DEV)
    eng.q_values_device(obs.data_ptr(), max(obs.stride(0), obs.shape[1]), 0 if act is None else act.data_ptr(),
                        eng.cfg.ac_dim if act is None else max(act.stride(0), act.shape[1]), n, target, out.data_ptr(), 1, n, stream())
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------ the batch slot: staging, weights, TD errors
def stage(eng, idx, w=None):
    """sactd3_rb_sample_indices_device on CUDA tensors (any stride); -> what has to stay alive"""
    idx = idx if torch.is_tensor(idx) else torch.as_tensor(idx, device=DEV)
    w = w.to(DEV) if torch.is_tensor(w) and not w.is_cuda else w
    eng.rb_sample_indices_device(idx.data_ptr(), max(idx.stride(0), 1), 0 if w is None else w.data_ptr(), 1 if w is None else max(w.stride(0), 1),
                                 idx.shape[0], stream())
    return idx, w


def td_of(eng):
    """sactd3_td_errors_device -> [2, B] on the host"""
    B = eng.cfg.batch_size
    out = torch.full((2, B), SENTINEL, device=DEV)
    eng.td_errors_device(out.data_ptr(), 1, B, stream())
    return out.cpu().numpy()


def slot(eng):
    d = {k: eng.debug_read(k) for k in ("X", "Xn", "rew", "done")}
    d["index"] = eng.read_batch()["index"]
    return d


# ------------------------------------------------------------------------------------------ n-step trajectories
NSTEP_STRIDE = 4
NSTEP_LENGTHS = (1, 2, 3, 4, 5, 6, 15, 16, 17)
NSTEP_SENTINEL = -77


def trajectories(o, a, n_rows, seed):
    """n_rows / NSTEP_STRIDE env steps of NSTEP_STRIDE envs in append order: within an episode row t+1 of an env starts at the s' of
    row t.  Episode lengths cycle through NSTEP_LENGTHS; episodes end by termination or, alternately, by a fresh s without a flag."""
    rng = np.random.default_rng(seed)
    T = n_rows // NSTEP_STRIDE
    obs, nobs = np.zeros((T, NSTEP_STRIDE, o), np.float32), np.zeros((T, NSTEP_STRIDE, o), np.float32)
    done = np.zeros((T, NSTEP_STRIDE), np.float32)
    for e in range(NSTEP_STRIDE):
        t, ep = 0, e                                                   # (each env starts at another place of the cycle)
        while t < T:
            n = NSTEP_LENGTHS[ep % len(NSTEP_LENGTHS)]
            s = rng.standard_normal(o).astype(np.float32)
            for j in range(n):
                if t >= T:
                    break
                obs[t, e] = s
                s = rng.standard_normal(o).astype(np.float32)
                nobs[t, e] = s
                if j == n - 1 and (ep // len(NSTEP_LENGTHS) + ep) % 2 == 0:
                    done[t, e] = 1.0                                   # ends by termination; otherwise by a fresh s without a flag
                t += 1
            ep += 1
    act = rng.uniform(-1, 1, (T, NSTEP_STRIDE, a)).astype(np.float32)
    rew = rng.standard_normal((T, NSTEP_STRIDE)).astype(np.float32)
    return [obs.reshape(-1, o), act.reshape(-1, a), rew.reshape(-1), nobs.reshape(-1, o), done.reshape(-1)]


def info(eng):
    """sactd3_nstep_info_device -> (k, last) on the host; a sentinel on either side of both arrays must survive"""
    B = eng.cfg.batch_size
    k = torch.full((B + 2,), NSTEP_SENTINEL, dtype=torch.int32, device=DEV)
    last = torch.full((B + 2,), NSTEP_SENTINEL, dtype=torch.int32, device=DEV)
    eng.nstep_info_device(k[1:].data_ptr(), 1, last[1:].data_ptr(), 1, stream())
    k, last = k.cpu().numpy(), last.cpu().numpy()
    assert k[0] == k[-1] == last[0] == last[-1] == NSTEP_SENTINEL, ("info", "a sentinel beside the outputs was overwritten")
    return k[1:-1], last[1:-1]


# ------------------------------------------------------------------------------------------ engine-owned priorities
@functools.lru_cache(maxsize=None)
def ring_rows(shape, n=HELD, seed=9):
    """the transitions every engine's ring holds: computed once per shape, never written"""
    _, (o, a, bound), _ = SHAPES[shape]
    return synth_transitions(n, o, a, bound, seed=seed)


def upload_priorities(eng, idx, prio):
    """sactd3_prio_update_device on host arrays (uploaded first); -> what has to stay alive"""
    i = torch.as_tensor(np.asarray(idx, np.int64), device=DEV)
    p = torch.as_tensor(np.asarray(prio, np.float32), device=DEV)
    eng.prio_update_device(i.data_ptr(), 1, p.data_ptr(), 1, i.shape[0], stream())
    return i, p


def integer_priorities():
    """2500 priorities from {0, 1, 2}: 100 zeros (the ring's first and last rows and both sides of a group boundary among them), 160 twos,
    ones elsewhere -- T = 2560 = 5 * 2^9, so u = k / 4096 with 8 | k puts u * T exactly on a running-sum boundary"""
    rng = np.random.default_rng(11)
    p = np.ones(HELD, np.float32)
    fixed_zero, fixed_two = [0, 1023, 1024, HELD - 1], [1, 1022, 1025, 2047, 2048, HELD - 2]
    rest = rng.permutation(np.setdiff1d(np.arange(HELD), fixed_zero + fixed_two))
    p[fixed_zero + list(rest[:96])] = 0.0
    p[fixed_two + list(rest[96:96 + 154])] = 2.0
    assert p.sum() == 2560.0, ("integer_priorities", float(p.sum()))
    return p


def boundary_uniforms(B):
    """k / 4096: 0, the largest, and multiples of 8 (mass exactly on a boundary) among arbitrary k"""
    rng = np.random.default_rng(12)
    k = rng.integers(0, 4096, B)
    k[:8] = [0, 4095, 8, 16, 4088, 2048, 1024, 3072]
    k[8:B // 2] = 8 * rng.integers(0, 512, B // 2 - 8)
    return (k / 4096.0).astype(np.float32)


# ------------------------------------------------------------------------------------------ the one-launch iteration and what it replaces
def sampled_draw(beta, n_step=1, stride=1):
    """the draw of a prioritised (beta) or uniform (beta None) n-step iteration, as call_sequence takes it"""
    def draw(eng):
        if beta is None:
            eng.rb_sample_nstep(n_step, stride)
        elif n_step == 1:
            eng.rb_sample_prioritized(beta)
        else:
            eng.rb_sample_prioritized_nstep(beta, n_step, stride)
    return draw


def call_sequence(eng, do_actor, draw, updates, write_back=False):
    """the iteration call by call -- what sactd3_step_sampled has to equal: draw(eng) fills the batch slot, then the critic update,
    write_back: the TD write-back of the priorities, the actor updates, the targets"""
    draw(eng)
    eng.update_qnets()
    if write_back:
        eng.prio_update_from_td()
    if do_actor:
        for _ in range(eng.cfg.actor_update_delay):
            eng.update_actor()
    eng.update_targ_nets(updates)


def iteration_state(eng, prio=False):
    """what one iteration leaves for the next to see: the slot with its ring indices, the TD errors, the metrics; prio: the slot
    weights and the priority table"""
    d = dict(eng.read_batch())
    d["td"] = td_of(eng)
    d["metrics"] = np.float32(list(eng.read_metrics().values()))
    if prio:
        for k in ("prio_weights", "prio_leaf", "prio_sums", "prio_max"):
            d[k] = eng.debug_read(k)
    return d


def raw_step(eng, do_actor, draw, n_step, stride, beta):
    """sactd3_step_sampled through the raw ABI -> its return code"""
    sm = _lib.CSampling(draw, n_step, stride, beta)
    return eng.lib.sactd3_step_sampled(eng._h, do_actor, C.byref(sm))
