"""Object wrapper over the C ABI (include/sactd3.h): numpy in, numpy out, exceptions for error codes."""
from __future__ import annotations

import ctypes as C
from dataclasses import asdict, dataclass
from typing import Dict, Optional

import numpy as np

from . import _lib
from ._lib import EngineError

_F = C.POINTER(C.c_float)


def _f32(x, shape=None) -> np.ndarray:
    arr = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    if shape is not None:
        arr = arr.reshape(shape)
    return arr


def _fp(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(_F)


def _vp(address) -> C.c_void_p:
    """a device address or stream handle the caller holds as an integer, as the C ABI takes it (0 = NULL)"""
    return C.c_void_p(int(address) or None)


def _flag(bit: int, on) -> int:
    return bit if on else 0


@dataclass
class Config:
    """Mirror of `sactd3_config`; defaults = tasks/defaults/sac.yml of the reference."""
    ob_dim: int = 0
    ac_dim: int = 0
    batch_size: int = 256
    rb_capacity: int = 1_000_000
    max_envs: int = 4
    prefer_td3_over_sac: bool = False
    layer_norm: bool = True
    autotune: bool = True
    bcq_style_targ_mix: bool = False
    targ_actor_smoothing: bool = True
    actor_update_delay: int = 2
    crit_targ_update_freq: int = 1
    use_graphs: bool = True
    device_id: int = 0
    actor_lr: float = 3e-4
    qnets_lr: float = 1e-3
    log_alpha_lr: float = 1e-3
    gamma: float = 0.99
    polyak: float = 0.005
    alpha_init: float = 0.2
    clip_norm: float = 0.0
    td3_std: float = 0.2
    td3_c: float = 0.5
    actor_noise_std: float = 0.1
    adam_beta1: float = 0.9
    adam_beta2: float = 0.999
    adam_eps: float = 1e-8
    bc_alpha: float = 0.0      # TD3+BC (include/sactd3.h: sactd3_set_bc): > 0 turns the behaviour-cloning actor term on; TD3 only
    seed: int = 0

    @staticmethod
    def from_hps(hps, ob_dim: int, ac_dim: int, **over) -> "Config":
        """Fill from any attribute- or key-style cfg (OmegaConf DictConfig, SimpleNamespace, dict, the
        oracle's Hps): only the keys the hot path reads, with the reference's branch-specific absences
        (td3.yml has no alpha_*/crit_targ_update_freq; sac.yml has no td3_*), agents/agent.py:47-139."""
        def get(k, default):
            if isinstance(hps, dict):
                return hps.get(k, default)
            try:
                v = getattr(hps, k)
            except Exception:
                return default
            return default if v is None else v
        c = Config(ob_dim=ob_dim, ac_dim=ac_dim)
        for k in ("batch_size", "rb_capacity", "prefer_td3_over_sac", "layer_norm", "autotune", "bcq_style_targ_mix",
                  "targ_actor_smoothing", "actor_update_delay", "crit_targ_update_freq", "actor_lr", "qnets_lr",
                  "log_alpha_lr", "gamma", "polyak", "alpha_init", "clip_norm", "td3_std", "td3_c", "actor_noise_std",
                  "bc_alpha", "seed"):
            setattr(c, k, type(getattr(c, k))(get(k, getattr(c, k))))
        c.max_envs = max(int(get("num_envs", 4)), 1)
        # NOT hps.cudagraphs: INTEGRATION.md runs the reference loop with `cudagraphs: false` so that orchestrator.py:313-315
        # does not wrap these methods in CudaGraphModule; the engine's own hipGraphs stay on unless `use_graphs=False` is passed
        for k, v in over.items():
            setattr(c, k, v)
        return c

    def to_c(self) -> _lib.CConfig:
        cc = _lib.CConfig()
        for k, v in asdict(self).items():
            setattr(cc, k, int(v) if isinstance(v, (bool, int)) else v)
        cc.abi_version = _lib.ABI_VERSION
        return cc


class Engine:
    """One learner on one MI355X.  All update calls are asynchronous on the engine's HIP stream."""

    # ReplayBuffer.extend / Agent._stage hand device arrays to the device entry points (rb_extend_fields_device /
    # load_batch_device); False forces the host route (copy to the host, pack there), e.g. to compare the two in one process
    device_inputs = True

    def __init__(self, cfg: Config, min_ac, max_ac):
        self.lib = _lib.load_library()
        self.cfg = cfg
        self._h = C.c_void_p()
        lo = _f32(np.broadcast_to(np.asarray(min_ac, np.float32).reshape(-1), (cfg.ac_dim,)))
        hi = _f32(np.broadcast_to(np.asarray(max_ac, np.float32).reshape(-1), (cfg.ac_dim,)))
        cc = cfg.to_c()
        rc = self.lib.sactd3_create(C.byref(cc), _fp(lo), _fp(hi), C.byref(self._h))
        if rc != 0:
            msg = self.lib.sactd3_last_error(None)
            self._h = C.c_void_p()
            raise EngineError(f"sactd3_create failed ({rc}): {msg.decode() if msg else '?'}")
        # host-side staging for the per-env-step calls (rb_extend of num_envs rows, predict): numpy -> ctypes pointer conversion
        # is ~1-2 us per array; these arrays' pointers are made once
        n0, o, a = max(int(cfg.max_envs), 1), cfg.ob_dim, cfg.ac_dim
        self._st_n = n0
        self._st = [np.zeros((n0, o), np.float32), np.zeros((n0, a), np.float32), np.zeros(n0, np.float32),
                    np.zeros((n0, o), np.float32), np.zeros(n0, np.uint8), np.zeros((n0, o), np.float32), np.zeros((n0, a), np.float32)]
        self._st_p = [x.ctypes.data_as(C.POINTER(C.c_uint8) if x.dtype == np.uint8 else _F) for x in self._st]
        self._df = _lib.CDeviceFields()     # argument block of the device-field calls, filled per call
        self._dfo = _lib.CDeviceFieldsOut()  # ... and of the two read-out calls

    # -- plumbing
    def _ck(self, rc):
        if rc < 0:
            msg = self.lib.sactd3_last_error(self._h)
            raise EngineError(f"libsactd3_hip error {rc}: {msg.decode() if msg else '?'}")
        return rc

    def _stats(self, fn, names) -> Dict[str, int]:
        """the four int64 counters a sactd3_*_stats call fills, under `names`"""
        out = (C.c_int64 * 4)()
        self._ck(fn(self._h, out))
        return {k: int(v) for k, v in zip(names, out)}

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.sactd3_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- parameters
    def param_count(self, which: int) -> int:
        return int(self._ck(self.lib.sactd3_param_count(self._h, which)))

    def get_params(self, which: int) -> np.ndarray:
        out = np.empty(self.param_count(which), np.float32)
        self._ck(self.lib.sactd3_get_params(self._h, which, _fp(out)))
        return out

    def set_params(self, which: int, flat) -> None:
        flat = _f32(flat).reshape(-1)
        if flat.size != self.param_count(which):
            raise ValueError(f"expected {self.param_count(which)} floats, got {flat.size}")
        self._ck(self.lib.sactd3_set_params(self._h, which, _fp(flat)))

    def get_adam_state(self, which: int):
        n = self.param_count(which)
        m, v, step = np.empty(n, np.float32), np.empty(n, np.float32), C.c_int64(0)
        self._ck(self.lib.sactd3_get_adam_state(self._h, which, _fp(m), _fp(v), C.byref(step)))
        return m, v, int(step.value)

    def set_adam_state(self, which: int, m, v, step: int) -> None:
        m, v = _f32(m).reshape(-1), _f32(v).reshape(-1)
        n = self.param_count(which)
        if m.size != n or v.size != n:
            raise ValueError(f"expected {n} floats of exp_avg / exp_avg_sq, got {m.size} / {v.size}")
        self._ck(self.lib.sactd3_set_adam_state(self._h, which, _fp(m), _fp(v), int(step)))

    # -- initialise / reset the networks on the device (include/sactd3_init.h)
    def init_params(self, what: int, seed: Optional[int] = None, epoch: int = 0) -> None:
        """sactd3_init_params: orthogonal weights, zero biases, LayerNorm ones / zeros for the networks `what` names (a sum of
        _lib.INIT_ACTOR / INIT_CRITICS / INIT_ALPHA), their targets a copy, their optimiser state cleared -- a pure function of
        (seed, epoch); seed None: the engine's configured seed.  Enqueued on the engine's stream: no wait, no copy."""
        seed = self.cfg.seed if seed is None else seed
        self._ck(self.lib.sactd3_init_params(self._h, int(what), int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch)))

    def init_stats(self) -> Dict[str, int]:
        """counters of init_params (sactd3_init_stats; waits for the engine's stream: the third lives on the device)"""
        st = self._stats(self.lib.sactd3_init_stats, ("calls", "matrices", "columns_redrawn", "reserved0"))
        return {k: st[k] for k in ("calls", "matrices", "columns_redrawn")}

    # -- replay
    def _rows(self, obs, act, rew, nobs, done):
        o, a = self.cfg.ob_dim, self.cfg.ac_dim
        obs, nobs = _f32(obs).reshape(-1, o), _f32(nobs).reshape(-1, o)
        n = obs.shape[0]
        act, rew = _f32(act).reshape(n, a), _f32(rew).reshape(n)
        done = np.ascontiguousarray(np.asarray(done).reshape(n) != 0, dtype=np.uint8)
        assert nobs.shape[0] == n
        return obs, act, rew, nobs, done, n

    def rb_extend(self, obs, act, rew, nobs, done) -> None:
        obs = np.asarray(obs)
        n = obs.size // self.cfg.ob_dim
        if 0 < n <= self._st_n and obs.size == n * self.cfg.ob_dim:      # an env step's rows: through the pre-bound staging arrays
            st, p = self._st, self._st_p
            st[0][:n] = obs.reshape(n, -1)
            st[1][:n] = np.asarray(act).reshape(n, -1)
            st[2][:n] = np.asarray(rew).reshape(n)
            st[3][:n] = np.asarray(nobs).reshape(n, -1)
            st[4][:n] = np.asarray(done).reshape(n) != 0
            self._ck(self.lib.sactd3_rb_extend(self._h, p[0], p[1], p[2], p[3], p[4], n))
            return
        obs, act, rew, nobs, done, n = self._rows(obs, act, rew, nobs, done)
        self._ck(self.lib.sactd3_rb_extend(self._h, _fp(obs), _fp(act), _fp(rew), _fp(nobs),
                                           done.ctypes.data_as(C.POINTER(C.c_uint8)), n))

    def rb_layout(self) -> Dict[str, int]:
        out = (C.c_int32 * 4)()
        self._ck(self.lib.sactd3_rb_layout(self._h, out))
        return dict(record_floats=int(out[0]), next_obs_offset=int(out[1]), next_obs_width=int(out[2]), capacity=int(out[3]))

    def pack_records(self, obs, act, rew, nobs, done) -> np.ndarray:
        """[n, record_floats] float32 in the ring's record layout (include/sactd3.h: sactd3_rb_layout)."""
        obs, act, rew, nobs, done, n = self._rows(obs, act, rew, nobs, done)
        lay, o, a = self.rb_layout(), self.cfg.ob_dim, self.cfg.ac_dim
        rec = np.zeros((n, lay["record_floats"]), np.float32)
        rec[:, :o], rec[:, o:o + a] = obs, act
        rec[:, lay["next_obs_offset"]:lay["next_obs_offset"] + o] = nobs
        tail = lay["next_obs_offset"] + lay["next_obs_width"]
        rec[:, tail], rec[:, tail + 1] = rew, done.astype(np.float32)
        return rec

    def rb_extend_device(self, device_ptr: int, n: int) -> None:
        """append n packed records that already live in device memory (kept alive by the caller until sync())."""
        self._ck(self.lib.sactd3_rb_extend_device(self._h, C.c_void_p(int(device_ptr)), int(n)))

    def rb_extend_records_device(self, device_ptr: int, n: int, producer_stream: int = 0, ordered: bool = True) -> None:
        """sactd3_rb_extend_records_device: rb_extend_device for a 16-byte aligned slab of n packed records that `producer_stream` (a
        hipStream_t as an integer; 0 = the default stream) may still be writing.  `ordered`: the engine orders its read behind that
        stream and the stream's next write behind the read, on the GPU; otherwise as rb_extend_device."""
        self._ck(self.lib.sactd3_rb_extend_records_device(self._h, _vp(device_ptr), int(n), _vp(producer_stream), _flag(_lib.SRC_ORDERED, ordered)))

    def _fields(self, fields):
        df = self._df
        (df.obs, df.obs_ld), (df.actions, df.actions_ld), (df.rewards, df.rewards_ld), (df.next_obs, df.next_obs_ld), (df.dones, df.dones_ld) = fields
        return C.byref(df)

    def rb_extend_fields_device(self, fields, n: int, producer_stream: int = 0, ordered: bool = True) -> None:
        """sactd3_rb_extend_fields_device: append n rows whose five fields -- `fields` = (device address, row stride in elements) of
        obs, actions, rewards, next_obs, dones (bytes) -- are in this device's memory.  `ordered`: the engine orders its read against
        `producer_stream` (a hipStream_t as an integer; 0 = the default stream) on the GPU; otherwise the caller has synchronised and
        keeps the arrays untouched until sync()."""
        self._ck(self.lib.sactd3_rb_extend_fields_device(self._h, self._fields(fields), int(n), _vp(producer_stream), _flag(_lib.SRC_ORDERED, ordered)))

    def load_batch_device(self, fields, n: int, producer_stream: int = 0, ordered: bool = True) -> None:
        """sactd3_load_batch_device: a caller-owned device batch (arguments as rb_extend_fields_device, n == batch_size) into the batch slot."""
        self._ck(self.lib.sactd3_load_batch_device(self._h, self._fields(fields), int(n), _vp(producer_stream), _flag(_lib.SRC_ORDERED, ordered)))

    def boundary_stats(self) -> Dict[str, int]:
        """host counters of the device boundary (sactd3_boundary_stats)"""
        return self._stats(self.lib.sactd3_boundary_stats, ("device_extends", "device_rows", "device_batches", "ordered_calls"))

    def _fields_out(self, fields):
        dfo = self._dfo
        ((dfo.obs, dfo.obs_ld), (dfo.actions, dfo.actions_ld), (dfo.rewards, dfo.rewards_ld), (dfo.next_obs, dfo.next_obs_ld),
         (dfo.dones, dfo.dones_ld), (dfo.index, dfo.index_ld)) = [(int(p) or None, int(ld)) for p, ld in fields]
        return C.byref(dfo)

    def read_batch_device(self, fields, consumer_stream: int = 0, ordered: bool = True) -> None:
        """sactd3_read_batch_device: the batch slot read_batch() reports, left in this device's memory.  `fields` = (device address,
        row stride in elements) of obs, actions, rewards, next_obs, dones (bytes), index (int64); address 0 = field not wanted.  One
        launch on the engine's stream, no host wait.  `ordered`: the engine orders its write against `consumer_stream` (a hipStream_t
        as an integer; 0 = the default stream) on the GPU and that stream may read the arrays at once; otherwise the caller has
        synchronised and calls sync() before it reads."""
        self._ck(self.lib.sactd3_read_batch_device(self._h, self._fields_out(fields), _vp(consumer_stream), _flag(_lib.DST_ORDERED, ordered)))

    def rb_read_rows_device(self, idx_ptr: int, idx_ld: int, n: int, fields, consumer_stream: int = 0, ordered: bool = True) -> None:
        """sactd3_rb_read_rows_device: n ring records chosen by a device int64 array (`idx_ptr`, stride `idx_ld` elements) into `fields`
        (as read_batch_device).  An index outside [0, rb_len) yields a zero row with flag 0, its index echoed, and is counted in
        readout_stats()["rows_refused"]."""
        self._ck(self.lib.sactd3_rb_read_rows_device(self._h, _vp(idx_ptr), int(idx_ld), int(n), self._fields_out(fields),
                                                     _vp(consumer_stream), _flag(_lib.DST_ORDERED, ordered)))

    def readout_stats(self) -> Dict[str, int]:
        """counters of the outward device boundary (sactd3_readout_stats; waits for the engine's stream: the last one lives on the device)"""
        return self._stats(self.lib.sactd3_readout_stats, ("batch_readouts", "row_readouts", "rows_requested", "rows_refused"))

    def rb_len(self) -> int:
        return int(self._ck(self.lib.sactd3_rb_len(self._h)))

    def batch_generation(self) -> int:
        """sactd3_batch_generation: grows with every call that puts new rows into the batch slot; the engine is its only writer"""
        return int(self._ck(self.lib.sactd3_batch_generation(self._h)))

    def rb_sample(self) -> None:
        self._ck(self.lib.sactd3_rb_sample(self._h))

    def rb_sample_with_indices(self, idx) -> None:
        idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int64).reshape(-1))
        if idx.size != self.cfg.batch_size:
            raise ValueError(f"expected {self.cfg.batch_size} indices, got {idx.size}")
        self._ck(self.lib.sactd3_rb_sample_with_indices(self._h, idx.ctypes.data_as(C.POINTER(C.c_int64)), idx.size))

    def load_batch(self, obs, act, rew, nobs, done) -> None:
        obs, act, rew, nobs, done, n = self._rows(obs, act, rew, nobs, done)
        self._ck(self.lib.sactd3_load_batch(self._h, _fp(obs), _fp(act), _fp(rew), _fp(nobs),
                                            done.ctypes.data_as(C.POINTER(C.c_uint8)), n))

    def read_batch(self) -> Dict[str, np.ndarray]:
        B, o, a = self.cfg.batch_size, self.cfg.ob_dim, self.cfg.ac_dim
        obs, act = np.empty((B, o), np.float32), np.empty((B, a), np.float32)
        rew, nobs = np.empty(B, np.float32), np.empty((B, o), np.float32)
        done, idx = np.empty(B, np.uint8), np.empty(B, np.int64)
        self._ck(self.lib.sactd3_read_batch(self._h, _fp(obs), _fp(act), _fp(rew), _fp(nobs),
                                            done.ctypes.data_as(C.POINTER(C.c_uint8)),
                                            idx.ctypes.data_as(C.POINTER(C.c_int64))))
        return dict(observations=obs, actions=act, rewards=rew, next_observations=nobs, dones=done.astype(bool), index=idx)

    def rb_fill_synthetic(self, n: int, seed: int = 0) -> None:
        self._ck(self.lib.sactd3_rb_fill_synthetic(self._h, int(n), int(seed)))

    # -- noise
    def set_noise(self, site: int, eps) -> None:
        eps = _f32(eps).reshape(-1, self.cfg.ac_dim)
        self._ck(self.lib.sactd3_set_noise(self._h, site, _fp(eps), eps.shape[0]))

    def clear_noise(self, site: int = -1) -> None:
        self._ck(self.lib.sactd3_clear_noise(self._h, site))

    def read_noise(self, site: int, n: Optional[int] = None) -> np.ndarray:
        n = self.cfg.batch_size if n is None else n
        out = np.empty((n, self.cfg.ac_dim), np.float32)
        self._ck(self.lib.sactd3_read_noise(self._h, site, _fp(out), n))
        return out

    # -- updates
    def update_qnets(self) -> None:
        self._ck(self.lib.sactd3_update_qnets(self._h))

    def update_actor(self) -> None:
        self._ck(self.lib.sactd3_update_actor(self._h))

    def update_targ_nets(self, qnet_updates_so_far: int) -> None:
        self._ck(self.lib.sactd3_update_targ_nets(self._h, int(qnet_updates_so_far)))

    def step(self, do_actor: bool) -> None:
        self._ck(self.lib.sactd3_step(self._h, int(bool(do_actor))))

    def step_sampled(self, do_actor: bool, *, beta: Optional[float] = None, n_step: int = 1, stride: int = 1,
                     prior_rows: Optional[int] = None, hindsight: bool = False) -> None:
        """sactd3_step_sampled: step() with a prioritised draw (`beta`: the exponent of the importance weights; None: the uniform
        draw) and / or `n_step` returns chained at `stride` rows per env step -- sample, weighted critic update, priority write-back,
        actor updates and target update as one graph launch, replayed while the ring grows and beta anneals.
        `prior_rows`: the mixed draw instead -- that many batch rows from the pinned rows (rb_pin), the others from the live rows;
        rb_set_mix is issued only when the value changed.  It has no prioritised and no n-step form.
        `hindsight=True`: rb_sample_hindsight's draw and relabelling instead (needs hindsight_configure), inside the same launch.  It
        excludes `beta`, n_step > 1 and `prior_rows`."""
        if hindsight:
            if beta is not None or int(n_step) != 1 or prior_rows is not None:
                raise ValueError("hindsight (the relabelling draw) excludes beta, n_step > 1 and prior_rows")
            sm = _lib.CSampling(_lib.DRAW_HINDSIGHT, 1, 1, 0.0)
        elif prior_rows is not None:
            if beta is not None or int(n_step) != 1:
                raise ValueError("prior_rows (the mixed draw) excludes beta and n_step > 1")
            if int(prior_rows) != getattr(self, "_mix_rows", None):
                self.rb_set_mix(int(prior_rows))
            sm = _lib.CSampling(_lib.DRAW_MIXED, 1, 1, 0.0)
        else:
            sm = _lib.CSampling(_lib.DRAW_UNIFORM if beta is None else _lib.DRAW_PRIORITIZED, int(n_step), int(stride),
                                0.0 if beta is None else float(beta))
        self._ck(self.lib.sactd3_step_sampled(self._h, int(bool(do_actor)), C.byref(sm)))

    def step_sampled_stats(self) -> Dict[str, int]:
        """host counters of step_sampled (sactd3_step_sampled_stats): calls issued, graphs captured for them"""
        st = self._stats(self.lib.sactd3_step_sampled_stats, ("launches", "graph_captures", "reserved0", "reserved1"))
        return {k: st[k] for k in ("launches", "graph_captures")}

    def step_prefix(self, m: int) -> None:
        """the first m iterations of a period (the one with the actor updates + m - 1 critic-only ones) in one graph launch"""
        self._ck(self.lib.sactd3_step_prefix(self._h, int(m)))

    def step_period(self) -> None:
        """actor_update_delay + 1 iterations (actor updates in the first) as one graph launch."""
        self._ck(self.lib.sactd3_step_period(self._h))

    def step_periods(self, k: int) -> None:
        """sactd3_step_periods: k whole periods, bit for bit k step_period() calls; where the period graph is pipelined, runs of
        several periods go out as one graph launch each."""
        self._ck(self.lib.sactd3_step_periods(self._h, int(k)))

    def step_periods_stats(self) -> Dict[str, int]:
        """host counters of step_periods (sactd3_step_periods_stats)"""
        return self._stats(self.lib.sactd3_step_periods_stats, ("calls", "run_launches", "single_period_launches", "run_graphs_captured"))

    def instantiate_graphs(self) -> None:
        """capture + instantiate the step / period graphs now instead of at their first use (nothing is launched)."""
        self._ck(self.lib.sactd3_instantiate_graphs(self._h))

    def run_iterations(self, i0: int, n: int) -> int:
        """iterations i0 .. i0 + n - 1 of the loop (orchestrator.py:337-352 schedule: actor updates when i % (delay + 1) == 0),
        whole periods as one graph launch each -- two or more of them in a row through step_periods(), where the engine has it --
        the rest one by one.  Returns i0 + n."""
        period = self.cfg.actor_update_delay + 1
        many = getattr(self, "step_periods", None)
        can = self.cfg.actor_update_delay > 0 and (self.cfg.prefer_td3_over_sac or self.cfg.crit_targ_update_freq == 1)
        i, end = i0, i0 + n
        while i < end:
            if can and i % period == 0 and i + 2 * period <= end and many is not None:
                many((end - i) // period)
                i += (end - i) // period * period
            elif can and i % period == 0 and i + period <= end:
                self.step_period()
                i += period
            elif can and i % period == 0:          # what is left behind the last whole period: its first end - i iterations, one launch
                self.step_prefix(end - i)
                i = end
            else:
                self.step(i % period == 0)
                i += 1
        return i

    def predict(self, obs, explore: bool) -> np.ndarray:
        obs = np.asarray(obs)
        n = obs.size // self.cfg.ob_dim
        if 0 < n <= self._st_n and obs.size == n * self.cfg.ob_dim:
            self._st[5][:n] = obs.reshape(n, -1)
            self._ck(self.lib.sactd3_predict(self._h, self._st_p[5], n, 1 if explore else 0, self._st_p[6]))
            return self._st[6][:n].copy()
        obs = _f32(obs).reshape(-1, self.cfg.ob_dim)
        out = np.empty((obs.shape[0], self.cfg.ac_dim), np.float32)
        self._ck(self.lib.sactd3_predict(self._h, _fp(obs), obs.shape[0], int(bool(explore)), _fp(out)))
        return out

    def predict_begin(self, obs, explore: bool, after_all: bool = False) -> None:
        """sactd3_predict_begin: stage `obs` and issue the acting kernels on the engine's acting stream, then return; the calls
        made until predict_end() overlap with them.  `after_all` orders them behind everything issued so far, as predict() does;
        otherwise they wait for the learner stream only behind a call that writes the actor (include/sactd3.h)."""
        obs = np.asarray(obs)
        n = obs.size // self.cfg.ob_dim
        flags = _flag(_lib.ACT_AFTER_ALL, after_all)
        if 0 < n <= self._st_n and obs.size == n * self.cfg.ob_dim:
            self._st[5][:n] = obs.reshape(n, -1)
            self._ck(self.lib.sactd3_predict_begin(self._h, self._st_p[5], n, 1 if explore else 0, flags))
        else:
            obs = _f32(obs).reshape(-1, self.cfg.ob_dim)
            n = obs.shape[0]
            self._ck(self.lib.sactd3_predict_begin(self._h, _fp(obs), n, int(bool(explore)), flags))   # (staged inside the call)
        self._act_n = n

    def predict_end(self) -> np.ndarray:
        """sactd3_predict_end: wait for the kernels of the call begun with predict_begin() (for them only) -> actions [n, ac_dim]."""
        n = getattr(self, "_act_n", 0)
        if 0 < n <= self._st_n:
            self._ck(self.lib.sactd3_predict_end(self._h, self._st_p[6]))
            self._act_n = 0
            return self._st[6][:n].copy()
        out = np.empty((max(n, int(self.cfg.max_envs), 1), self.cfg.ac_dim), np.float32)      # (n == 0: the engine reports the state error)
        self._ck(self.lib.sactd3_predict_end(self._h, _fp(out)))
        self._act_n = 0
        return out[:n].copy()

    def predict_device(self, obs_ptr: int, obs_ld: int, n: int, explore: bool, out_ptr: int, out_ld: int,
                       caller_stream: int = 0, ordered: bool = True) -> None:
        """sactd3_predict_device: act on n observation rows that live in this device's memory (`obs_ptr`: device address, `obs_ld`: row
        stride in elements) and write the actions to device memory (`out_ptr`, `out_ld`) -- asynchronous, stream-ordered behind the
        updates issued so far, no host wait.  `ordered`: the engine orders its read and the caller's next use of both arrays against
        `caller_stream` (a hipStream_t as an integer; 0 = the default stream) on the GPU; otherwise the caller has synchronised and
        leaves both arrays alone until sync()."""
        self._ck(self.lib.sactd3_predict_device(self._h, _vp(obs_ptr), int(obs_ld), int(n), 1 if explore else 0,
                                                _vp(out_ptr), int(out_ld), _vp(caller_stream), _flag(_lib.SRC_ORDERED, ordered)))

    def predict_device_stats(self) -> Dict[str, int]:
        """host counters of the device acting route (sactd3_predict_device_stats)"""
        return self._stats(self.lib.sactd3_predict_device_stats, ("calls", "rows", "ordered_calls", "multi_block_tails"))

    def q_values(self, obs, act=None, target: bool = False) -> np.ndarray:
        """sactd3_qvalues: Q_k(obs_i, act_i) of the twin critics -- the target pair with `target` -- for host rows -> [2, n] float32.
        `act` None: the pairs are (s, pi(s)), pi(s) = what predict(explore=False) returns.  Waits for the result; bit for bit the
        values q_values_device() leaves on the device, and training does not see the call."""
        obs = _f32(obs).reshape(-1, self.cfg.ob_dim)
        n = obs.shape[0]
        if act is not None:
            act = _f32(act).reshape(-1, self.cfg.ac_dim)
            if act.shape[0] != n:
                raise ValueError(f"observations and actions disagree on the number of rows: {n}, {act.shape[0]}")
        out = np.empty((2, n), np.float32)
        self._ck(self.lib.sactd3_qvalues(self._h, _fp(obs), _fp(act), n, _lib.Q_TARGET if target else _lib.Q_ONLINE, _fp(out)))
        return out

    def q_values_device(self, obs_ptr: int, obs_ld: int, act_ptr: int, act_ld: int, n: int, target: bool, q_ptr: int, q_ld: int,
                        q_ns: int, stream: int = 0, ordered: bool = True) -> None:
        """sactd3_qvalues_device: score n rows that live in this device's memory -- `obs_ptr` / `act_ptr`: device addresses, `*_ld`: row
        strides in elements; `act_ptr` 0: the policy form, (s, pi(s)) -- with the online or (`target`) the target critics; critic k's
        value of row i goes to the float32 at `q_ptr` + 4 (k `q_ns` + i `q_ld`).  Asynchronous on the engine's stream behind the updates
        issued so far, no host wait, invisible to training.  `ordered`: the engine orders its reads and its write against `stream` (a
        hipStream_t as an integer; 0 = the default stream) on the GPU; otherwise the caller has synchronised and calls sync()."""
        self._ck(self.lib.sactd3_qvalues_device(self._h, _vp(obs_ptr), int(obs_ld), _vp(act_ptr), int(act_ld), int(n),
                                                _lib.Q_TARGET if target else _lib.Q_ONLINE, _vp(q_ptr), int(q_ld), int(q_ns), _vp(stream),
                                                _flag(_lib.SRC_ORDERED, ordered)))

    def qvalues_stats(self) -> Dict[str, int]:
        """host counters of the scoring route (sactd3_qvalues_stats)"""
        return self._stats(self.lib.sactd3_qvalues_stats, ("calls", "rows", "ordered_calls", "policy_calls"))

    def policy_outputs(self, sample: bool = False, actions: bool = False):
        """the outputs of sactd3_policy_io a query of this engine's policy fills: `mode`; SAC also `mean`, `log_std`; with a sample
        `sample`, `sample_logp`, `eps_out`; with given actions `action_logp`"""
        if self.cfg.prefer_td3_over_sac:
            return ("mode",)
        return ("mode", "mean", "log_std") + (("sample", "sample_logp", "eps_out") if sample else ()) + (("action_logp",) if actions else ())

    def policy_device(self, obs_ptr: int, obs_ld: int, n: int, fields, target: bool = False, stream: int = 0, ordered: bool = True) -> None:
        """sactd3_policy_device: ask the actor about n observation rows that live in this device's memory.  `fields`: {name of a
        sactd3_policy_io field: (device address, row stride in elements)} -- the inputs `actions` / `eps` and whichever outputs are
        wanted (`mode`, `mean`, `log_std`, `sample`, `sample_logp`, `action_logp`, `eps_out`); a field left out is NULL.  `target`: the
        target actor (TD3).  Asynchronous on the engine's stream behind the updates issued so far, no host wait, invisible to training
        and acting.  `ordered` / `stream` as for q_values_device."""
        io = _lib.CPolicyIO()
        names = {f for f, _ in _lib.POLICY_IO_FIELDS}
        for name, (ptr, ld) in dict(fields).items():
            if name not in names:
                raise ValueError(f"policy_device: unknown field `{name}` (expected a subset of {sorted(names)})")
            setattr(io, name, int(ptr) or None)
            setattr(io, name + "_ld", int(ld))
        self._ck(self.lib.sactd3_policy_device(self._h, _vp(obs_ptr), int(obs_ld), int(n), _lib.PI_TARGET if target else _lib.PI_ONLINE,
                                               C.byref(io), _vp(stream), _flag(_lib.SRC_ORDERED, ordered)))

    def policy(self, obs, actions=None, eps=None, sample: bool = False, target: bool = False) -> Dict[str, np.ndarray]:
        """sactd3_policy: the same for host rows -> {output name: float32 array}, [n, ac_dim] or [n] (the log-probs) -- the outputs
        policy_outputs(sample or eps given, actions given) names.  Waits for the result; bit for bit what policy_device() leaves on
        the device."""
        obs = _f32(obs).reshape(-1, self.cfg.ob_dim)
        n, a = obs.shape[0], self.cfg.ac_dim
        io, keep = _lib.CPolicyIO(), {}
        for name, x in (("actions", actions), ("eps", eps)):
            if x is None:
                continue
            x = _f32(x).reshape(-1, a)
            if x.shape[0] != n:
                raise ValueError(f"observations and {name} disagree on the number of rows: {n}, {x.shape[0]}")
            keep[name] = x
            setattr(io, name, x.ctypes.data)
            setattr(io, name + "_ld", a)
        out = {}
        for name in self.policy_outputs(bool(sample) or eps is not None, actions is not None):
            out[name] = np.empty((n,) if name.endswith("_logp") else (n, a), np.float32)
            setattr(io, name, out[name].ctypes.data)
            setattr(io, name + "_ld", 1 if name.endswith("_logp") else a)
        self._ck(self.lib.sactd3_policy(self._h, _fp(obs), n, _lib.PI_TARGET if target else _lib.PI_ONLINE, C.byref(io)))
        return out

    def policy_stats(self) -> Dict[str, int]:
        """counters of the policy queries (sactd3_policy_stats); the last two are counted on the device: the call waits"""
        return self._stats(self.lib.sactd3_policy_stats, ("calls", "rows", "rows_clamped", "rows_nan"))

    def eval_rollout(self, env_handle, outputs, *, steps: int = 0, sample: bool = False, reset: bool = True, soft: bool = False,
                     gamma: Optional[float] = None, seed: int = 0, stream: int = 0, ordered: bool = True) -> None:
        """sactd3_eval_rollout (include/sactd3_eval.h): roll the envs of a native env (`env_handle`: its sactd3_env*) for `steps` steps
        (0: its horizon) under the online actor in ONE kernel launch on the engine's stream -- greedy actions, or (`sample`, SAC) sampled
        ones with their log-probs -- and leave the trajectory, the returns-to-go and the per-env summary in device memory.  `outputs`:
        {name of a sactd3_eval_out field: device address}, a field left out is NULL; every array time-major and contiguous.  `reset`:
        sactd3_env_reset(seed) first.  `soft`: entropy terms in the returns-to-go.  `gamma` None: the engine's.  No host wait; invisible
        to training and acting.  `ordered` / `stream` as for q_values_device."""
        cfg = _lib.CEvalConfig(int(steps), _lib.EVAL_SAMPLE if sample else _lib.EVAL_GREEDY, 1 if reset else 0, 1 if soft else 0,
                               float(self.cfg.gamma if gamma is None else gamma), int(seed) & 0xFFFFFFFFFFFFFFFF)
        out = _lib.CEvalOut()
        names = {f[0] for f in _lib.EVAL_OUT_FIELDS}
        for name, ptr in dict(outputs).items():
            if name not in names:
                raise ValueError(f"eval_rollout: unknown output `{name}` (expected a subset of {sorted(names)})")
            setattr(out, name, int(ptr) or None)
        self._ck(self.lib.sactd3_eval_rollout(self._h, env_handle, C.byref(cfg), C.byref(out), _vp(stream), _flag(_lib.SRC_ORDERED, ordered)))

    def eval_stats(self) -> Dict[str, int]:
        """counters of eval_rollout (sactd3_eval_stats); the last one is the device word that numbers its draws: the call waits"""
        return self._stats(self.lib.sactd3_eval_stats, ("calls", "env_steps", "calls_that_drew", "eval_ctr"))

    def rb_sample_indices_device(self, idx_ptr: int, idx_ld: int, w_ptr: int, w_ld: int, n: int, stream: int = 0, ordered: bool = True) -> None:
        """sactd3_rb_sample_indices_device: fill the batch slot with the ring records a device int64 array names (`idx_ptr`, stride
        `idx_ld` elements; n == batch_size) and the slot's loss weights from a device float32 array (`w_ptr`, `w_ld`; address 0: all 1).
        One launch, no host wait.  An index outside [0, rb_len) gives a zero record with slot index -1 and weight 0; a weight that is
        negative, NaN or infinite is staged as 0; both are counted in priority_stats()["rows_refused"]."""
        self._ck(self.lib.sactd3_rb_sample_indices_device(self._h, _vp(idx_ptr), int(idx_ld), _vp(w_ptr), int(w_ld), int(n), _vp(stream),
                                                          _flag(_lib.SRC_ORDERED, ordered)))

    def batch_weights_device(self, w_ptr: int, w_ld: int, n: int, stream: int = 0, ordered: bool = True) -> None:
        """sactd3_batch_weights_device: loss weights (device float32, `w_ptr` / `w_ld`, n == batch_size) for whatever the batch slot
        holds; address 0 drops the weights.  While the slot carries weights update_qnets() minimises (1 / B) sum_i w_i err_i^2."""
        self._ck(self.lib.sactd3_batch_weights_device(self._h, _vp(w_ptr), int(w_ld), int(n), _vp(stream), _flag(_lib.SRC_ORDERED, ordered)))

    def td_errors_device(self, td_ptr: int, td_ld: int, td_ns: int, stream: int = 0, ordered: bool = True) -> None:
        """sactd3_td_errors_device: Q_k(s_i, a_i) - y_i of the most recent critic update to the float32 at `td_ptr` + 4 (k `td_ns` +
        i `td_ld`), in this device's memory.  One launch, no host wait; EngineError (SACTD3_ESTATE) when no critic update has run on
        the rows now in the batch slot."""
        self._ck(self.lib.sactd3_td_errors_device(self._h, _vp(td_ptr), int(td_ld), int(td_ns), _vp(stream), _flag(_lib.DST_ORDERED, ordered)))

    def priority_stats(self) -> Dict[str, int]:
        """counters of the prioritised route (sactd3_priority_stats; waits for the engine's stream: the last one lives on the device)"""
        return self._stats(self.lib.sactd3_priority_stats, ("index_stagings", "weight_stagings", "td_readouts", "rows_refused"))

    # -- prioritised replay the engine owns (include/sactd3.h: sactd3_prio_*)
    def prio_enable(self, alpha: float = 0.6, eps: float = 1e-6) -> None:
        """sactd3_prio_enable: one priority per ring slot and their group sums, in device memory; rows already held enter at priority
        1, every later append at the running maximum."""
        self._ck(self.lib.sactd3_prio_enable(self._h, float(alpha), float(eps)))

    def rb_sample_prioritized(self, beta: float) -> None:
        """sactd3_rb_sample_prioritized: the batch slot filled by priority (three launches, no host wait), with the importance
        weights (N p_i^alpha / T)^(-beta) over the batch's largest as the slot's loss weights."""
        self._ck(self.lib.sactd3_rb_sample_prioritized(self._h, float(beta)))

    def prio_set_uniforms(self, u=None) -> None:
        """sactd3_prio_set_uniforms: batch_size uniforms in [0, 1) to draw with instead of the Philox stream (sticky); None: native."""
        if u is None:
            self._ck(self.lib.sactd3_prio_set_uniforms(self._h, None, 0))
            return
        u = np.ascontiguousarray(np.asarray(u, dtype=np.float32).reshape(-1))
        self._ck(self.lib.sactd3_prio_set_uniforms(self._h, _fp(u), int(u.size)))

    def prio_update_from_td(self) -> None:
        """sactd3_prio_update_from_td: the batch rows' priorities from the TD errors of the critic update that just ran on them."""
        self._ck(self.lib.sactd3_prio_update_from_td(self._h))

    def prio_update_device(self, idx_ptr: int, idx_ld: int, prio_ptr: int, prio_ld: int, n: int, stream: int = 0, ordered: bool = True) -> None:
        """sactd3_prio_update_device: unscaled priorities (device float32 at `prio_ptr`, stride `prio_ld`) for the ring slots a device
        int64 array names; a bad index or priority is refused on the device and counted in prio_stats()["rows_refused"]."""
        self._ck(self.lib.sactd3_prio_update_device(self._h, _vp(idx_ptr), int(idx_ld), _vp(prio_ptr), int(prio_ld), int(n), _vp(stream),
                                                    _flag(_lib.SRC_ORDERED, ordered)))

    def prio_stats(self) -> Dict[str, int]:
        """counters of the engine-owned priorities (sactd3_prio_stats; waits for the engine's stream)"""
        return self._stats(self.lib.sactd3_prio_stats, ("samples", "write_backs", "rows_refused", "rows_entered_at_max"))

    # -- n-step returns staged by the engine (include/sactd3.h: sactd3_rb_sample_nstep*)
    def rb_sample_nstep_device(self, idx_ptr: int, idx_ld: int, w_ptr: int, w_ld: int, n: int, steps: int, stride: int, stream: int = 0,
                               ordered: bool = True) -> None:
        """sactd3_rb_sample_nstep_device: rb_sample_indices_device with the chain -- per row the batch slot gets [s|a] of the start
        slot, the discounted return of up to `steps` consecutive rows of its env (`stride` = rows appended per env step), the s' of the
        chain's last row and the mask 1 - (1 - d_last) gamma^(k-1), so that update_qnets() computes the k-step target.  One launch."""
        self._ck(self.lib.sactd3_rb_sample_nstep_device(self._h, _vp(idx_ptr), int(idx_ld), _vp(w_ptr), int(w_ld), int(n), int(steps),
                                                        int(stride), _vp(stream), _flag(_lib.SRC_ORDERED, ordered)))

    def rb_sample_nstep(self, steps: int, stride: int) -> None:
        """sactd3_rb_sample_nstep: rb_sample() with the chain (the same uniform draw, one counter tick, no weights)."""
        self._ck(self.lib.sactd3_rb_sample_nstep(self._h, int(steps), int(stride)))

    def rb_sample_prioritized_nstep(self, beta: float, steps: int, stride: int) -> None:
        """sactd3_rb_sample_prioritized_nstep: rb_sample_prioritized() with the chain started at every drawn slot."""
        self._ck(self.lib.sactd3_rb_sample_prioritized_nstep(self._h, float(beta), int(steps), int(stride)))

    def nstep_info_device(self, k_ptr: int, k_ld: int, last_ptr: int, last_ld: int, stream: int = 0, ordered: bool = True) -> None:
        """sactd3_nstep_info_device: the chain length k and the ring slot of the chain's last row of every row of an n-step batch slot,
        to int32 arrays in this device's memory (address 0: not wanted).  EngineError (SACTD3_ESTATE) on a slot that is not n-step."""
        self._ck(self.lib.sactd3_nstep_info_device(self._h, _vp(k_ptr), int(k_ld), _vp(last_ptr), int(last_ld), _vp(stream),
                                                   _flag(_lib.DST_ORDERED, ordered)))

    def nstep_stats(self) -> Dict[str, int]:
        """counters of the n-step route (sactd3_nstep_stats; waits for the engine's stream: the last two live on the device)"""
        return self._stats(self.lib.sactd3_nstep_stats, ("stagings", "rows_staged", "rows_cut_short", "rows_refused"))

    # -- prior data under an online run (include/sactd3.h: sactd3_rb_pin, sactd3_rb_set_mix, sactd3_rb_sample_mixed)
    def rb_pin(self, n: int) -> None:
        """sactd3_rb_pin: ring slots [0, n) become rows no append overwrites; appends go round-robin over the slots behind them.
        Allowed before the ring has wrapped; 0 unpins.  Not saved in checkpoints."""
        self._ck(self.lib.sactd3_rb_pin(self._h, int(n)))

    def rb_pinned(self) -> int:
        return int(self._ck(self.lib.sactd3_rb_pinned(self._h)))

    def rb_set_mix(self, prior_rows: int) -> None:
        """sactd3_rb_set_mix: how many rows of a mixed batch come from the pinned rows (0 .. batch_size)."""
        self._ck(self.lib.sactd3_rb_set_mix(self._h, int(prior_rows)))
        self._mix_rows = int(prior_rows)

    def rb_sample_mixed(self) -> None:
        """sactd3_rb_sample_mixed: the batch slot filled with rb_set_mix's share of pinned rows and live rows for the rest -- the
        index stream of rb_sample(), one counter tick, two launches, no weights."""
        self._ck(self.lib.sactd3_rb_sample_mixed(self._h))

    def mix_stats(self) -> Dict[str, int]:
        """host counters of the mixed draw and the pinned ring (sactd3_mix_stats)"""
        return self._stats(self.lib.sactd3_mix_stats, ("mixed_draws", "prior_rows_drawn", "live_rows_drawn", "pinned_wraps"))

    # -- hindsight relabelling at staging (include/sactd3.h: sactd3_hindsight_configure, sactd3_rb_sample_hindsight*)
    def hindsight_configure(self, achieved: int, desired: int, dim: int, threshold: float, ratio: float, window: int, stride: int) -> None:
        """sactd3_hindsight_configure: where an observation keeps its achieved and its desired goal, when a goal counts as reached, the
        share of rows relabelled, how many rows ahead a goal may lie and the rows appended per env step.  Host state: no launch."""
        cfg = _lib.CHindsightConfig(int(achieved), int(desired), int(dim), int(window), int(stride), float(threshold), float(ratio))
        self._ck(self.lib.sactd3_hindsight_configure(self._h, C.byref(cfg)))

    def rb_sample_hindsight(self) -> None:
        """sactd3_rb_sample_hindsight: rb_sample()'s draw (one counter tick), then one launch that relabels goals while it stages."""
        self._ck(self.lib.sactd3_rb_sample_hindsight(self._h))

    def rb_sample_hindsight_device(self, idx_ptr: int, idx_ld: int, choice_ptr: int, choice_ld: int, n: int, stream: int = 0,
                                   ordered: bool = True) -> None:
        """sactd3_rb_sample_hindsight_device: the caller's start slots (int64) and, optionally, its choices (int32; address 0: the
        native draw) -- below 0 not relabelled, otherwise the offset of the goal's row, cut to the episode's rest.  One launch."""
        self._ck(self.lib.sactd3_rb_sample_hindsight_device(self._h, _vp(idx_ptr), int(idx_ld), _vp(choice_ptr), int(choice_ld), int(n),
                                                            _vp(stream), _flag(_lib.SRC_ORDERED, ordered)))

    def hindsight_info_device(self, offset_ptr: int, offset_ld: int, slot_ptr: int, slot_ld: int, stream: int = 0, ordered: bool = True) -> None:
        """sactd3_hindsight_info_device: per row of a hindsight batch slot the offset j (-1: not relabelled or refused) and the goal's ring
        slot (-1), to int32 arrays in this device's memory (address 0: not wanted).  EngineError (SACTD3_ESTATE) on any other slot."""
        self._ck(self.lib.sactd3_hindsight_info_device(self._h, _vp(offset_ptr), int(offset_ld), _vp(slot_ptr), int(slot_ld), _vp(stream),
                                                       _flag(_lib.DST_ORDERED, ordered)))

    def hindsight_stats(self) -> Dict[str, int]:
        """counters of the hindsight route (sactd3_hindsight_stats; waits for the engine's stream: the last three live on the device)"""
        return self._stats(self.lib.sactd3_hindsight_stats, ("native_draws", "rows_relabelled", "rows_refused", "rows_reward_zero"))

    def acting_stats(self) -> Dict[str, int]:
        """host counters of the two-stream ordering policy (sactd3_acting_stats)"""
        return self._stats(self.lib.sactd3_acting_stats, ("begun", "begin_waited_for_learner", "learner_waited_for_acting", "ended_by_spin"))

    # -- TD3+BC (include/sactd3.h: sactd3_set_bc)
    def set_bc(self, alpha: float, weight: float = 1.0) -> None:
        """sactd3_set_bc: new (bc_alpha, bc_weight) of an engine created with cfg.bc_alpha > 0 -- one small launch on the engine's
        stream, no graph capture, the run-ahead chain of step_period(s) stays intact.  bc_weight is run-time state: not saved."""
        self._ck(self.lib.sactd3_set_bc(self._h, float(alpha), float(weight)))

    def bc(self):
        """sactd3_get_bc: (bc_alpha, bc_weight) as the device holds them (waits for the engine's stream)"""
        out = np.empty(2, np.float32)
        self._ck(self.lib.sactd3_get_bc(self._h, _fp(out)))
        return float(out[0]), float(out[1])

    def read_metrics(self) -> Dict[str, float]:
        m = np.empty(_lib.NUM_METRICS, np.float32)
        self._ck(self.lib.sactd3_read_metrics(self._h, _fp(m)))
        out = {"loss/qf_loss": float(m[0]), "loss/actor_loss": float(m[1]), "loss/alpha_loss": float(m[2]),
               "vitals/alpha": float(m[3])}
        if self.cfg.bc_alpha > 0:      # (an engine without BC never writes these two slots)
            out["loss/bc_loss"], out["vitals/bc_lambda"] = float(m[_lib.M_BC_LOSS]), float(m[_lib.M_BC_LAMBDA])
        return out

    def sync(self) -> None:
        self._ck(self.lib.sactd3_sync(self._h))

    def device_handles(self):
        """(hipStream_t of the engine, device address of the float32 metrics slots) as integers."""
        st, mp = C.c_void_p(), C.c_void_p()
        self._ck(self.lib.sactd3_device_handles(self._h, C.byref(st), C.byref(mp)))
        return int(st.value or 0), int(mp.value or 0)

    # -- introspection
    def debug_read(self, name: str) -> np.ndarray:
        n = int(self._ck(self.lib.sactd3_debug_read(self._h, name.encode(), None, 0)))
        out = np.empty(n, np.float32)
        self._ck(self.lib.sactd3_debug_read(self._h, name.encode(), _fp(out), n))
        return out

    def graph_kernel_count(self, which: int) -> int:
        return int(self._ck(self.lib.sactd3_graph_kernel_count(self._h, which)))

    def time_kernel(self, name: str, iters: int = 200) -> float:
        us = C.c_float(0)
        self._ck(self.lib.sactd3_time_kernel(self._h, name.encode(), iters, C.byref(us)))
        return float(us.value)

    def time_nodes(self, which, iters: int = 200):
        """[{name, us, flops, bytes, threads}] for every kernel node of: 0 / False a critic-only fused iteration, 1 / True one with
        the actor updates, 2 a whole period of the schedule as sactd3_step_period captures it (consumes the learner's state)."""
        cap = 128
        us, fl, by, th = np.zeros(cap, np.float32), np.zeros(cap, np.float64), np.zeros(cap, np.float64), np.zeros(cap, np.int64)
        names = C.create_string_buffer(cap * 128)
        dp = C.POINTER(C.c_double)
        n = self._ck(self.lib.sactd3_time_nodes(self._h, int(which), iters, cap, names, len(names), _fp(us),
                                                fl.ctypes.data_as(dp), by.ctypes.data_as(dp), th.ctypes.data_as(C.POINTER(C.c_int64))))
        labels = names.value.decode().split("\n")[:n]
        return [dict(name=labels[k], us=float(us[k]), flops=float(fl[k]), bytes=float(by[k]), threads=int(th[k])) for k in range(n)]

    def time_gather_sweep(self, batch: int, iters: int = 50):
        us, nbytes = C.c_float(0), C.c_double(0)
        self._ck(self.lib.sactd3_time_gather_sweep(self._h, batch, iters, C.byref(us), C.byref(nbytes)))
        return float(us.value), float(nbytes.value)
