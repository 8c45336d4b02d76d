"""Drop-in mirror of the reference's learner object (agents/agent.py:21-331) on top of the HIP engine.

Same constructor, method names, argument meaning, counters and error behaviour (asserts / exceptions) as the
reference `Agent`, so orchestrator.py:258-412 can drive it unchanged; see INTEGRATION.md for the two-line
change in main.py.  Nothing here computes on the CPU: every method is a call into libsactd3_hip.so.
"""
from __future__ import annotations

import sys
from pathlib import Path
from typing import Any, Dict, Mapping, Optional, Tuple

import numpy as np

from . import _lib, schema
from .engine import Config, Engine


def _np(x) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def _cai(x):
    """the __cuda_array_interface__ of a device array (None: a host array, or a dtype the interface cannot describe)"""
    try:
        return getattr(x, "__cuda_array_interface__", None)
    except (TypeError, RuntimeError, ValueError):
        return None


def _cai_field(cai, width: int, item: int):
    """(address, rows, row stride in elements) of a device array [n, width] -- or [n] when width == 1 -- of `item`-byte elements
    with a contiguous inner dimension, from its __cuda_array_interface__; None when the layout needs a copy first."""
    shape, strides = tuple(cai["shape"]), cai.get("strides")
    if not ((len(shape) == 2 and shape[1] == width) or (len(shape) == 1 and width == 1)):
        raise ValueError(f"expected [n, {width}]" + (" or [n]" if width == 1 else "") + f", got {list(shape)}")
    n, ld = int(shape[0]), width
    if strides is not None:
        if len(shape) == 2 and width > 1 and strides[1] != item:      # (whatever n is: one row with an inner stride is not a row)
            return None
        if n > 1:                                                     # (one row: whatever its row stride is reported as, the width will do)
            if strides[0] % item or strides[0] // item < width:
                return None
            ld = strides[0] // item
    return int(cai["data"][0]), n, int(ld)


def _on_engine_device(engine: Engine, x) -> bool:
    dev = getattr(x, "device", None)
    ordinal = getattr(dev, "index", getattr(dev, "id", None))
    return ordinal is None or int(ordinal) == int(engine.cfg.device_id)


def _detached(x):
    return x.detach() if hasattr(x, "detach") else x


_ITEM = {"f4": 4, "b1": 1, "i8": 8}      # the element kinds of a field -- float32, flags, int64 -- and their sizes in bytes


def _is_kind(typestr: str, kind: str) -> bool:
    return typestr[1:] == kind or (kind == "b1" and typestr[2:] == "1")      # (flags: any one-byte type)


def _read_input(engine: Engine, x, width: int, kind: str, cai=None):
    """THE reader of an array the caller hands in.  -> (array to keep alive across the call, address, rows, row stride in elements),
    or None when `x` is not an array in the memory of the engine's device: the host route, an upload or a TypeError is the caller's.
    Pointer, shape and strides come from __cuda_array_interface__, read once unless the array is converted; a caller that has read it
    already and routed on it passes it as `cai`, with the detached array it belongs to.  A field that is not float32 (flags: not
    1-byte), or whose inner dimension is not contiguous, is first converted ON the device with the array library's own ops
    (.to(float32), != 0, .contiguous()); nothing converts to int64: an index of another dtype is None too."""
    if cai is None:
        x = _detached(x)
        cai = _cai(x)
        if cai is None or not _on_engine_device(engine, x):
            return None
    if not _is_kind(cai["typestr"], kind):
        if kind == "i8":
            return None
        if kind == "b1":
            x = x != 0
        else:
            lib = sys.modules.get(type(x).__module__.partition(".")[0])
            x = x.to(getattr(lib, "float32", "float32"))
        cai = _cai(x)
    got = _cai_field(cai, width, _ITEM[kind])
    if got is None:
        x = x.contiguous()
        got = _cai_field(_cai(x), width, _ITEM[kind])
    return x, got[0], got[1], got[2]


def _output_cai(engine: Engine, x, kind: str, name: str):
    """the __cuda_array_interface__ of an array the engine is to write, which cannot be converted the way an input can: anything but
    elements of `kind` in the memory of the engine's device is a TypeError"""
    cai = _cai(_detached(x))
    if cai is None or not _on_engine_device(engine, x):
        raise TypeError(f"{name} must be an array in the memory of the engine's device")
    if not _is_kind(cai["typestr"], kind):
        raise TypeError(f"{name} must be " + {"f4": "float32", "b1": "bool (one byte per flag)", "i8": "int64"}[kind] + f", got {cai['typestr']}")
    return cai


def _read_output(engine: Engine, x, width: int, kind: str, name: str, n: int, more_rows: bool = False):
    """THE reader of an array the engine is to write.  -> (address, rows, row stride in elements) of n rows -- `more_rows`: or more
    -- as _cai_field reads them; a wrong shape, an inner stride or a wrong row count is a ValueError.  `name` opens every message."""
    cai = _output_cai(engine, x, kind, name)
    try:
        got = _cai_field(cai, width, _ITEM[kind])
    except ValueError as ex:
        raise ValueError(f"{name}: {ex}") from None
    if got is None:
        raise ValueError(f"{name} needs a contiguous inner dimension and a row stride of at least its width")
    if got[1] < n or (got[1] > n and not more_rows):
        raise ValueError(f"{name} has {got[1]} rows, expected {'at least ' if more_rows else ''}{n}")
    return got


def _torch_alloc(engine: Engine, what: str):
    """alloc(shape, kind) of an output nobody passed: torch.empty on the engine's device"""
    try:
        import torch
    except ImportError:
        raise TypeError(f"{what}: without torch the caller passes `out`") from None
    dev = torch.device("cuda", int(engine.cfg.device_id))
    kinds = {"f4": torch.float32, "b1": torch.bool, "i8": torch.int64}
    return lambda shape, kind: torch.empty(shape, dtype=kinds[kind], device=dev)


def _device_route(engine: Engine, obs, act, rew, nobs, done):
    """The one place that decides how five arrays reach the engine.  -> (fields, n, keep) for Engine.rb_extend_fields_device /
    load_batch_device when ALL of them are arrays on the engine's device (`keep` holds converted copies alive across the call),
    None for the host route (numpy, a mix of host and device, another device, `engine.device_inputs` off).  It is _read_input for
    five arrays that go one way together: where all of them live is settled first, then each field is read."""
    if not getattr(engine, "device_inputs", False):
        return None
    xs = [_detached(x) for x in (obs, act, rew, nobs, done)]
    cais = [_cai(x) for x in xs]      # (read once per array: building the dictionary is the expensive part of this function)
    if any(c is None for c in cais):
        return None
    if not all(_on_engine_device(engine, x) for x in xs):      # another GPU's arrays take the host route (the C side refuses them too)
        return None
    o, a = engine.cfg.ob_dim, engine.cfg.ac_dim
    got = [_read_input(engine, x, width, kind, cai) for x, cai, width, kind in zip(xs, cais, (o, a, 1, o, 1), ("f4", "f4", "f4", "f4", "b1"))]
    rows = [n for _, _, n, _ in got]
    if len(set(rows)) != 1:
        raise ValueError(f"fields disagree on the number of rows: {rows}")
    if rows[0] == 0:
        return None      # (nothing to read: the host route's n == 0 case)
    return [(ptr, ld) for _, ptr, _, ld in got], rows[0], [x for x, _, _, _ in got]


# the six destinations of a read-out, in the order of sactd3_device_fields_out: (key, width -- "o" / "a" = the engine's dims --, kind)
_OUT_FIELDS = (("observations", "o", "f4"), ("actions", "a", "f4"), ("rewards", 1, "f4"), ("next_observations", "o", "f4"),
               ("dones", 1, "b1"), ("index", 1, "i8"))


def _device_outputs(engine: Engine, n: int, out: Optional[Mapping[str, Any]] = None, alloc=None):
    """The one place that decides where a read-out lands.  -> (tensors, fields): `tensors` has the reference's keys -- observations
    [n, o], actions [n, a], rewards [n, 1], next_observations [n, o] float32; dones [n, 1] bool, terminations (the same array, as the
    reference stores it); index [n] int64 -- and `fields` the six (device address, row stride in elements) pairs for
    Engine.read_batch_device / rb_read_rows_device.  Arrays come from `alloc(shape, kind)` (default: torch.empty on the engine's
    device); `out` may replace any of them with a preallocated array or view (rewards / dones / index as [n, 1] or [n]; `terminations`
    names the dones array).  Each is read by _read_output: a wrong dtype or another device's array is a TypeError, a wrong shape, an
    inner stride or another row count a ValueError."""
    out = dict(out) if out else {}
    known = {k for k, _, _ in _OUT_FIELDS} | {"terminations"}
    if set(out) - known:
        raise ValueError(f"unknown output key(s) {sorted(set(out) - known)}: expected a subset of {sorted(known)}")
    if "terminations" in out:
        if "dones" in out and out["dones"] is not out["terminations"]:
            raise ValueError("`dones` and `terminations` are one array (the reference stores the same flags under both keys)")
        out["dones"] = out.pop("terminations")
    dims = {"o": int(engine.cfg.ob_dim), "a": int(engine.cfg.ac_dim)}
    tensors, fields = {}, []
    for key, width, kind in _OUT_FIELDS:
        width = dims.get(width, width)
        x = out.get(key)
        if x is None:
            if alloc is None:
                alloc = _torch_alloc(engine, "device read-out")
            x = alloc((n,) if key == "index" else (n, width), kind)
        ptr, _, ld = _read_output(engine, x, width, kind, f"`{key}`", n)
        tensors[key] = x
        fields.append((ptr, ld))
    tensors["terminations"] = tensors["dones"]
    return tensors, fields


def _index_field(engine: Engine, index):
    """-> (index, address, n, stride in elements) of a ring-slot index for Engine.rb_read_rows_device / rb_sample_indices_device: an
    int64 array on the engine's device is taken where it is (made contiguous on the device if its stride is not whole elements);
    anything else goes through torch.as_tensor and is uploaded first."""
    got = _read_input(engine, index, 1, "i8")
    if got is None:
        import torch
        got = _read_input(engine, torch.as_tensor(index, dtype=torch.int64).to(torch.device("cuda", int(engine.cfg.device_id))), 1, "i8")
    return got


def _weight_field(engine: Engine, weights, n: int, what: str):
    """-> (array kept alive, address, stride in elements) of per-row loss weights for Engine.rb_sample_indices_device /
    batch_weights_device: [n] or [n, 1] on the engine's device; converted ON the device when not float32 or not strided in whole
    elements, as _device_route does for its fields.  Not an array of that device: TypeError; another row count: ValueError."""
    try:
        got = _read_input(engine, weights, 1, "f4")
    except ValueError as ex:
        raise ValueError(f"{what}: weights: {ex}") from None
    if got is None:
        raise TypeError(f"{what}: the weights must be an array in the memory of the engine's device")
    if got[2] != n:
        raise ValueError(f"{what}: expected {n} weights (one per batch row), got {got[2]}")
    return got[0], got[1], got[3]


def _critic_major_out(engine: Engine, n: int, out, what: str):
    """Where a [2, n, 1] float32 result of the twin critics lands (Agent.q_values, Agent.td_errors).  -> (out, address, row stride,
    critic stride in elements, rows of `out`).  `out` None: torch.empty on the engine's device; otherwise a preallocated float32
    [2, >= n, 1] array or view of that device with positive strides in whole elements -- a wrong dtype or another device's array is a
    TypeError, a wrong shape or stride a ValueError."""
    if out is None:
        out = _torch_alloc(engine, what)((2, n, 1), "f4")
    ocai = _output_cai(engine, out, "f4", f"{what}: `out`")
    shape, strides = tuple(ocai["shape"]), ocai.get("strides")
    if len(shape) != 3 or shape[0] != 2 or shape[2] != 1 or shape[1] < n:
        raise ValueError(f"{what}: `out` must be [2, >= {n}, 1], got {list(shape)}")
    q_ns, q_ld = int(shape[1]), 1
    if strides is not None:                              # (the inner dimension has one element: its stride does not matter)
        if strides[0] % 4 or strides[1] % 4 or strides[0] < 4 or (shape[1] > 1 and strides[1] < 4):
            raise ValueError(f"{what}: `out` needs positive strides in whole elements")
        q_ns, q_ld = strides[0] // 4, (strides[1] // 4 if shape[1] > 1 else 1)
    return out, int(ocai["data"][0]), q_ld, q_ns, int(shape[1])


def _producer_stream(x, device_id: int) -> int:
    """the stream the caller's arrays were written on, as far as the array library tells: torch's current stream of the device"""
    if type(x).__module__.partition(".")[0] == "torch":
        import torch
        return int(torch.cuda.current_stream(device_id).cuda_stream)
    return 0      # the default stream


class LazyMetric:
    """A loss value that stays on the device until somebody looks at it (the reference returns 0-dim device
    tensors from update_* and only materialises them at eval time, orchestrator.py:383)."""

    def __init__(self, agent: "Agent", key: str):
        self._agent, self._key = agent, key

    def item(self) -> float:
        return self._agent.engine.read_metrics()[self._key]

    __float__ = item

    def numpy(self):
        return np.float32(self.item())

    def __repr__(self):
        return f"LazyMetric({self._key})"


class _DeviceScalar:
    """__cuda_array_interface__ view of ONE float32 in the engine's device memory (a metrics slot)."""

    def __init__(self, ptr: int):
        self.__cuda_array_interface__ = {"shape": (), "typestr": "<f4", "data": (int(ptr), False), "version": 3, "strides": None}


_METRIC_SLOT = {"loss/qf_loss": 0, "loss/actor_loss": 1, "loss/alpha_loss": 2, "vitals/alpha": 3,
                "loss/bc_loss": 4, "vitals/bc_lambda": 5}   # SACTD3_M_* (the last two: written by a TD3+BC engine only)


class StaleBatchError(RuntimeError):
    """A BatchHandle names THE batch slot of the engine, not a copy: once any later engine call has refilled the slot (the engine
    counts them: Engine.batch_generation), an older handle no longer stands for the rows it was made for.  The reference's loop never keeps one
    (orchestrator.py:338-348 samples, updates, drops); a caller that does gets this error instead of a silent update on the
    newest sample."""


class BatchHandle(dict):
    """What `rb.sample()` returns: the batch lives in the engine's HBM batch slot; indexing a key reads it back
    (host sync) as the reference's TensorDict keys would (observations, actions, rewards, next_observations,
    terminations, dones, index).  `on_device()` -- and key access on a handle of ReplayBuffer(..., device_batches=True) -- hands
    the same keys out as device tensors instead, as the reference's rb.sample() does (main.py:167-171, orchestrator.py:338)."""

    def __init__(self, engine: Engine, generation: int = 0, device: bool = False):
        super().__init__()
        self._engine = engine
        self._generation = generation      # Engine.batch_generation() when this handle was made (see StaleBatchError)
        self._device = device              # key access: device tensors (one read-out launch, cached) instead of numpy arrays
        self._cache: Optional[Dict[str, Any]] = None

    def _is_current(self) -> bool:
        return self._engine.batch_generation() == self._generation

    def on_device(self, out: Optional[Mapping[str, Any]] = None) -> Dict[str, Any]:
        """The batch as a dict of tensors on the engine's device (include/sactd3.h: sactd3_read_batch_device), all keys filled by ONE
        launch on the engine's stream: nothing goes through the host and the host does not wait.  The write is ordered on the GPU
        against torch's current stream, which may use the tensors at once.  `out`: preallocated tensors or views (any subset of the
        keys) to write into.  Raises StaleBatchError where the host read-back does."""
        if not self._is_current():
            raise StaleBatchError("this batch handle is older than the engine's batch slot: a later rb.sample() / staged batch replaced its rows")
        eng = self._engine
        tensors, fields = _device_outputs(eng, int(eng.cfg.batch_size), out)
        eng.read_batch_device(fields, _producer_stream(tensors["observations"], eng.cfg.device_id))
        return tensors

    def __missing__(self, key):
        if self._cache is None and self._device:
            self._cache = self.on_device()
        if self._cache is None:
            if not self._is_current():
                raise StaleBatchError("this batch handle is older than the engine's batch slot: a later rb.sample() / staged batch replaced its rows")
            self._cache = self._engine.read_batch()
            self._cache["terminations"] = self._cache["dones"]
            for k in ("rewards", "dones", "terminations"):
                self._cache[k] = self._cache[k].reshape(-1, 1)
        return self._cache[key]

    def n_step_info(self) -> Dict[str, Any]:
        """{"steps": int32 [B], "last_index": int32 [B]} on the engine's device, for a handle made with n_step > 1: the chain length k
        of every row (0: the row was refused) and the ring slot of the chain's last row (-1), written by one launch ordered against
        torch's current stream (include/sactd3.h: sactd3_nstep_info_device).  On such a handle `rewards` is the n-step return,
        `next_observations` the state the target bootstraps from, and `dones` is (mask != 0) with mask = 1 - (1 - d_last) gamma^(k-1):
        for k > 1 that is NOT the termination flag -- the mask is exactly 1.0 iff the chain's last row terminated.  StaleBatchError
        when the handle is not current, RuntimeError on a handle that is not n-step."""
        if not self._is_current():
            raise StaleBatchError("this batch handle is older than the engine's batch slot: a later rb.sample() / staged batch replaced its rows")
        if not getattr(self, "_n_step", False):
            raise RuntimeError("n_step_info: this batch was not sampled with n_step > 1")
        import torch
        eng = self._engine
        dev = torch.device("cuda", int(eng.cfg.device_id))
        steps = torch.empty(int(eng.cfg.batch_size), dtype=torch.int32, device=dev)
        last = torch.empty_like(steps)
        eng.nstep_info_device(steps.data_ptr(), 1, last.data_ptr(), 1, _producer_stream(steps, eng.cfg.device_id))
        return {"steps": steps, "last_index": last}

    def hindsight_info(self) -> Dict[str, Any]:
        """{"offset": int32 [B], "goal_index": int32 [B]} on the engine's device, for a handle made by sample_hindsight /
        sample_hindsight_at: how many env steps behind the row its new goal was achieved (0: the row's own arrival; -1: the row was not
        relabelled, or refused) and the ring slot the goal was taken from (-1), written by one launch ordered against torch's current
        stream (include/sactd3.h: sactd3_hindsight_info_device).  On such a handle the desired goal inside `observations` and
        `next_observations` and the `rewards` of the relabelled rows are the relabelled ones; `dones` is the stored flag.
        StaleBatchError when the handle is not current, RuntimeError on a handle that is not a hindsight one."""
        if not self._is_current():
            raise StaleBatchError("this batch handle is older than the engine's batch slot: a later rb.sample() / staged batch replaced its rows")
        if not getattr(self, "_hindsight", False):
            raise RuntimeError("hindsight_info: this batch was not sampled with sample_hindsight / sample_hindsight_at")
        import torch
        eng = self._engine
        dev = torch.device("cuda", int(eng.cfg.device_id))
        offset = torch.empty(int(eng.cfg.batch_size), dtype=torch.int32, device=dev)
        goal = torch.empty_like(offset)
        eng.hindsight_info_device(offset.data_ptr(), 1, goal.data_ptr(), 1, _producer_stream(offset, eng.cfg.device_id))
        return {"offset": offset, "goal_index": goal}


def _n_step_args(what: str, n_step, stride) -> Tuple[int, int]:
    """(steps, stride) of a sampling call, checked before the engine is touched"""
    n_step = int(n_step)
    if not 1 <= n_step <= 16:
        raise ValueError(f"{what}: n_step must be in [1, 16], got {n_step}")
    if n_step > 1 and stride is None:
        raise ValueError(f"{what}: n_step > 1 needs `stride`, the rows appended per env step (the env count)")
    if stride is not None and int(stride) < 1:
        raise ValueError(f"{what}: stride must be at least 1, got {stride}")
    return n_step, (1 if stride is None else int(stride))


class ReplayBuffer:
    """TensorDictReplayBuffer(storage=LazyTensorStorage(capacity, device)) stand-in (main.py:167-171): built by
    the caller BEFORE the agent, bound to the engine's HBM ring when the agent receives it."""

    def __init__(self, capacity: int, device: Any = None, device_batches: bool = False):
        """`device_batches`: sample() returns handles whose keys are tensors on the engine's device, as the reference's are (the
        first key access fills all of them with one launch); the default keeps the host read-back to numpy arrays."""
        self.capacity, self.device, self.device_batches = int(capacity), device, bool(device_batches)
        self._engine: Optional[Engine] = None
        self._priorities: Optional[Dict[str, float]] = None      # enable_priorities' arguments, once it was called
        self._hindsight: Optional[Dict[str, Any]] = None         # configure_hindsight's arguments, once it was called

    def _bind(self, engine: Engine):
        self._engine = engine
        if self._priorities is not None:      # enabled before the agent existed: the engine learns it now
            engine.prio_enable(**self._priorities)
        if self._hindsight is not None:
            engine.hindsight_configure(**self._hindsight)

    def _need(self) -> Engine:
        assert self._engine is not None, "replay buffer is not attached to an Agent yet"
        return self._engine

    def _new_handle(self, eng: Engine, n_step: bool = False) -> BatchHandle:
        h = BatchHandle(eng, eng.batch_generation(), device=self.device_batches)      # read behind the call that filled the slot
        h._n_step = n_step
        return h

    def _staged(self, eng: Engine, n_step: int, stride: int, one_step: str, chained: str, *args, tail=()) -> BatchHandle:
        """the one place a sampling call forks on n_step: the engine's 1-step call `one_step(*args, *tail)`, or its chained form
        `chained(*args, n_step, stride, *tail)`; then the handle of the freshly filled slot"""
        if n_step == 1:
            getattr(eng, one_step)(*args, *tail)
        else:
            getattr(eng, chained)(*args, n_step, stride, *tail)
        return self._new_handle(eng, n_step > 1)

    def extend(self, td: Mapping[str, Any]) -> None:
        """orchestrator.py:100-113: keys observations, next_observations, actions, rewards, terminations, dones."""
        done = td["dones"] if "dones" in td else td["terminations"]
        eng = self._need()
        five = (td["observations"], td["actions"], td["rewards"], td["next_observations"], done)
        dev = _device_route(eng, *five)
        if dev is not None:      # device tensors stay where they are: one pack kernel, ordered against the caller's stream on the GPU
            eng.rb_extend_fields_device(dev[0], dev[1], _producer_stream(five[0], eng.cfg.device_id))
            return
        eng.rb_extend(*[_np(x) for x in five])

    def extend_records(self, records) -> None:
        """extend() with rows that are ALREADY ring records: a float32 [n, record_floats] array in the memory of the engine's device,
        contiguous and 16-byte aligned, in the layout of Engine.rb_layout() -- what `envs.NativeVecEnv.step_records` writes
        (`envs.pack_records` states the layout).  One ingest launch per ring region, ordered on the GPU behind what torch's current
        stream has queued (the producer of the slab) and in front of what it queues next: the caller neither waits nor keeps the slab
        untouched (include/sactd3.h: sactd3_rb_extend_records_device).  The ring, its length, a pinned prefix and the priorities end
        as extend() of the same rows leaves them."""
        eng = self._need()
        width = eng.rb_layout()["record_floats"]
        x = _detached(records)
        cai = _cai(x)
        if cai is None or not _on_engine_device(eng, x):
            raise TypeError("extend_records: `records` must be an array in the memory of the engine's device (extend() takes host rows)")
        got = _cai_field(cai, width, 4) if _is_kind(cai["typestr"], "f4") else None      # (nothing is converted: a copy would not be the slab)
        if got is None or got[2] != width:
            raise ValueError(f"extend_records: `records` must be float32 [n, {width}] with contiguous rows")
        eng.rb_extend_records_device(got[0], got[1], _producer_stream(records, eng.cfg.device_id))

    def sample(self, batch_size: int, *, n_step: int = 1, stride: Optional[int] = None) -> BatchHandle:
        """`n_step` > 1: every drawn row starts a chain of up to n_step consecutive rows of its env (`stride` = the rows appended per
        env step, i.e. the env count), cut where an episode ends or the ring does; the slot holds the discounted return, the last
        row's next observation and the mask that make the critic update the n-step one, staged by one launch
        (include/sactd3.h: sactd3_rb_sample_nstep).  For SAC the entropy terms of the intermediate steps are not added.  The start rows
        are those sample() would draw; BatchHandle.n_step_info() gives the chain lengths."""
        n_step, stride = _n_step_args("sample", n_step, stride)
        eng = self._need()
        assert batch_size == eng.cfg.batch_size, "the engine is built for one batch size (hps.batch_size)"
        return self._staged(eng, n_step, stride, "rb_sample", "rb_sample_nstep")

    def sample_at(self, index, weights=None, *, n_step: int = 1, stride: Optional[int] = None) -> BatchHandle:
        """sample() with the caller's rows: the ring records `index` names (batch_size ring slots: an int64 tensor on the engine's
        device, or anything torch can turn into one, as for rows()) become the batch, staged by ONE launch on the engine's stream
        (include/sactd3.h: sactd3_rb_sample_indices_device) -- no copy out and back in, no host wait.  `weights`: per-row loss
        weights, float32 [batch_size] or [batch_size, 1] on the engine's device (converted on the device if not float32 or not
        contiguous) -- the importance-sampling weights of a prioritised sampler; None: all 1.  The critic update on the returned
        handle minimises (1 / B) sum_i w_i (Q(s_i, a_i) - y_i)^2; Agent.td_errors() then gives the rows' TD errors.  A slot outside
        [0, len(rb)) becomes a zero record with index -1 and weight 0, a weight that is negative, NaN or infinite becomes 0: neither
        reaches the parameters.  The handle is a sample()'s in every other respect (generation, device_batches).  `n_step`, `stride`:
        as for sample(), the chains starting at `index` (sactd3_rb_sample_nstep_device)."""
        n_step, stride = _n_step_args("sample_at", n_step, stride)
        eng = self._need()
        B = int(eng.cfg.batch_size)
        index, ptr, n, ld = _index_field(eng, index)
        if n != B:
            raise ValueError(f"sample_at: expected {B} indices (the engine is built for one batch size), got {n}")
        keep, w_ptr, w_ld = (None, 0, 1) if weights is None else _weight_field(eng, weights, B, "sample_at")
        h = self._staged(eng, n_step, stride, "rb_sample_indices_device", "rb_sample_nstep_device", ptr, ld, w_ptr, w_ld, n,
                         tail=(_producer_stream(index, eng.cfg.device_id),))
        del keep      # (the engine's read is ordered against the stream the allocator hands the block out on)
        return h

    def enable_priorities(self, alpha: float = 0.6, eps: float = 1e-6) -> None:
        """Proportional prioritised replay kept by the engine (include/sactd3.h: sactd3_prio_enable): one priority per ring slot in
        device memory.  Rows already held enter at priority 1, every later extend() at the running maximum -- the engine sees its own
        appends, there is no cursor to mirror.  Before the buffer is attached to an Agent the call is remembered and made then."""
        if not (alpha >= 0.0 and eps > 0.0):
            raise ValueError("enable_priorities: alpha >= 0 and eps > 0 required")
        if self._engine is not None:
            self._engine.prio_enable(alpha, eps)
        self._priorities = dict(alpha=float(alpha), eps=float(eps))

    def sample_prioritized(self, batch_size: int, beta: float, *, n_step: int = 1, stride: Optional[int] = None) -> BatchHandle:
        """sample() by priority (sactd3_rb_sample_prioritized): P(i) ~ p_i^alpha, with replacement, drawn, staged and weighted on the
        device by three launches; the slot carries the importance weights (N P(i))^(-beta) over the batch's largest, so the critic
        update on the returned handle is the weighted one.  The handle is a sample()'s in every other respect.  `n_step`, `stride`: as
        for sample(), the chains starting at the drawn slots (sactd3_rb_sample_prioritized_nstep); update_priorities() afterwards
        writes to the start slots."""
        n_step, stride = _n_step_args("sample_prioritized", n_step, stride)
        if self._priorities is None:
            raise RuntimeError("sample_prioritized: call enable_priorities() first")
        eng = self._need()
        assert batch_size == eng.cfg.batch_size, "the engine is built for one batch size (hps.batch_size)"
        return self._staged(eng, n_step, stride, "rb_sample_prioritized", "rb_sample_prioritized_nstep", beta)

    def configure_hindsight(self, *, achieved: int, desired: int, dim: int, threshold: float, ratio: float = 0.8, window: int = 50,
                            stride: Optional[int] = None) -> None:
        """Hindsight relabelling kept by the engine (hindsight experience replay, the "future" strategy; include/sactd3.h:
        sactd3_hindsight_configure).  `achieved`, `desired`, `dim`: floats [achieved, achieved + dim) of an observation are the goal it
        has reached, floats [desired, desired + dim) the goal it is after (envs.NativeVecEnv.goal_layout names them for a native task);
        `threshold`: a goal counts as reached, and pays 0 instead of -1, within this distance; `ratio`: the share of a batch's rows
        that get a goal their own episode reached at or after the row; `window`: how many env steps ahead that goal may lie (the env's
        horizon); `stride`: the rows appended per env step, i.e. the env count (None: the engine's max_envs).  Host state only.  Before
        the buffer is attached to an Agent the call is remembered and made then.  Not saved in checkpoints."""
        args = dict(achieved=int(achieved), desired=int(desired), dim=int(dim), threshold=float(threshold), ratio=float(ratio), window=int(window),
                    stride=None if stride is None else int(stride))
        if self._engine is not None:
            if args["stride"] is None:
                args["stride"] = int(self._engine.cfg.max_envs)
            self._engine.hindsight_configure(**args)
        elif args["stride"] is None:
            raise ValueError("configure_hindsight: before the buffer is attached to an Agent `stride` (the env count) must be given")
        self._hindsight = args

    def _hindsight_handle(self, eng: Engine) -> BatchHandle:
        h = self._new_handle(eng)
        h._hindsight = True
        return h

    def sample_hindsight(self, batch_size: int) -> BatchHandle:
        """sample() with goals relabelled while the rows are staged (sactd3_rb_sample_hindsight): the start rows are those sample() would
        draw (one counter tick); a `ratio` share of them receives, in place of its desired goal, a goal achieved later in its own
        episode, with the reward that goal pays -- two launches, no torch arithmetic, no copy out and back in.  The handle is a
        sample()'s in every other respect; BatchHandle.hindsight_info() says which rows were relabelled and from where.  Needs
        configure_hindsight(); excludes priorities, n-step chains and pinned rows."""
        if self._hindsight is None:
            raise RuntimeError("sample_hindsight: call configure_hindsight() first")
        eng = self._need()
        assert batch_size == eng.cfg.batch_size, "the engine is built for one batch size (hps.batch_size)"
        eng.rb_sample_hindsight()
        return self._hindsight_handle(eng)

    def sample_hindsight_at(self, index, choice=None) -> BatchHandle:
        """sample_hindsight() with the caller's start rows (`index`: batch_size ring slots, as for sample_at) and, optionally, the
        caller's choices (`choice`: int32 [batch_size]; below 0: the row keeps its goal; otherwise the number of env steps behind the
        row its new goal is taken from, cut to what is left of the episode).  None: the engine draws (sactd3_rb_sample_hindsight_device).
        A slot outside [0, len(rb)) becomes a zero record with index -1."""
        if self._hindsight is None:
            raise RuntimeError("sample_hindsight_at: call configure_hindsight() first")
        eng = self._need()
        B = int(eng.cfg.batch_size)
        index, ptr, n, ld = _index_field(eng, index)
        if n != B:
            raise ValueError(f"sample_hindsight_at: expected {B} indices (the engine is built for one batch size), got {n}")
        c_ptr = 0
        if choice is not None:
            import torch
            choice = torch.as_tensor(choice, dtype=torch.int32).to(torch.device("cuda", int(eng.cfg.device_id))).reshape(-1).contiguous()
            if choice.numel() != B:
                raise ValueError(f"sample_hindsight_at: expected {B} choices (one per batch row), got {choice.numel()}")
            c_ptr = choice.data_ptr()
        eng.rb_sample_hindsight_device(ptr, ld, c_ptr, 1, n, _producer_stream(index, eng.cfg.device_id))
        del choice      # (the engine's read is ordered against the stream the allocator hands the block out on)
        return self._hindsight_handle(eng)

    def pin(self, n: Optional[int] = None) -> None:
        """Protect the first `n` rows (None: every row held now) from eviction: a dataset loaded before the online run starts
        (include/sactd3.h: sactd3_rb_pin).  extend() then goes round-robin over the slots behind them.  Allowed before the buffer has
        wrapped; pin(0) unpins.  Excludes enable_priorities() and n_step > 1 for now.  Not saved in checkpoints."""
        eng = self._need()
        eng.rb_pin(eng.rb_len() if n is None else int(n))

    @property
    def pinned(self) -> int:
        return 0 if self._engine is None else self._engine.rb_pinned()

    def sample_mixed(self, batch_size: int, prior_rows: int) -> BatchHandle:
        """sample() with a fixed share of prior data: the first `prior_rows` rows of the batch are drawn from the pinned rows, the
        others from the rows behind them (sactd3_rb_sample_mixed) -- the index stream of sample(), one counter tick, no weights.  The
        handle is a sample()'s in every respect: older handles go stale."""
        eng = self._need()
        assert batch_size == eng.cfg.batch_size, "the engine is built for one batch size (hps.batch_size)"
        if int(prior_rows) != getattr(eng, "_mix_rows", None):
            eng.rb_set_mix(int(prior_rows))
        return self._staged(eng, 1, 1, "rb_sample_mixed", "rb_sample_mixed")

    def update_priorities(self, index=None, priorities=None) -> None:
        """The write-back.  No arguments: the rows of the batch slot get |TD error| (the larger of the twin critics') + eps of the
        critic update that just ran on them (sactd3_prio_update_from_td).  Both arguments: ring slots (int64, as for rows()) and their
        unscaled priorities (float32 [n] or [n, 1] on the engine's device), taken where they are (sactd3_prio_update_device)."""
        if self._priorities is None:
            raise RuntimeError("update_priorities: call enable_priorities() first")
        if (index is None) != (priorities is None):
            raise ValueError("update_priorities: pass both `index` and `priorities`, or neither")
        eng = self._need()
        if index is None:
            eng.prio_update_from_td()
            return
        index, ptr, n, ld = _index_field(eng, index)
        keep, p_ptr, p_ld = _weight_field(eng, priorities, n, "update_priorities")
        eng.prio_update_device(ptr, ld, p_ptr, p_ld, n, _producer_stream(index, eng.cfg.device_id))
        del keep

    def rows(self, index, out: Optional[Mapping[str, Any]] = None) -> Dict[str, Any]:
        """The ring records `index` names (ring slots: what `index` of a sample holds), as a dict of tensors on the engine's device
        with the keys of a batch -- for a sampler of the caller's own (prioritised, n-step, hindsight) that reads the rows it relabels
        or chains where they are (include/sactd3.h: sactd3_rb_read_rows_device).  `index`: an int64 tensor on the engine's device, any
        length >= 1, or anything torch can turn into one (uploaded first).  A slot outside [0, len(rb)) yields a zero row with flag
        False.  `out` as for BatchHandle.on_device."""
        eng = self._need()
        index, ptr, n, ld = _index_field(eng, index)
        tensors, fields = _device_outputs(eng, n, out)
        eng.rb_read_rows_device(ptr, ld, n, fields, _producer_stream(index, eng.cfg.device_id))
        return tensors

    def __len__(self) -> int:
        return 0 if self._engine is None else self._engine.rb_len()


RESET_NAMES = {"actor": _lib.INIT_ACTOR, "critics": _lib.INIT_CRITICS, "alpha": _lib.INIT_ALPHA}


def _init_what(what, td3: bool) -> int:
    """names of RESET_NAMES (a sequence, or one comma-separated string) -> the bits of sactd3_init_params; TD3 drops "alpha";
    ValueError for an unknown name or nothing left to initialise"""
    names = [w.strip() for w in what.split(",")] if isinstance(what, str) else list(what)
    bad = [w for w in names if w not in RESET_NAMES]
    if bad or not names:
        raise ValueError(f"networks to initialise: a non-empty choice of {sorted(RESET_NAMES)}, got {what!r}")
    bits = 0
    for w in names:
        if not (td3 and w == "alpha"):
            bits |= RESET_NAMES[w]
    if not bits:
        raise ValueError("a TD3 agent has no temperature: nothing left to initialise")
    return bits


class Agent:
    """agents/agent.py:Agent, MI355X-native."""

    def __init__(self, net_shapes: Dict[str, tuple], min_ac: np.ndarray, max_ac: np.ndarray, device: Any,
                 hps: Any, rb: Optional[ReplayBuffer] = None, *, seed: Optional[int] = None,
                 init_params: bool = True, use_graphs: Optional[bool] = None, metrics: str = "tensor", init: str = "torch"):
        """`init`: who produces the initial parameters (with `init_params`).  "torch" (the default): the reference's own, torch's
        orthogonal_ on the host under the caller's torch seed, installed through set_params.  "engine": the engine's, on the device
        (include/sactd3_init.h) -- a pure function of the engine's seed, no torch, no copy; not torch's stream, so not the
        reference's values.
        `use_graphs`: None = the engine's own hipGraphs ON (whatever `hps.cudagraphs` says: that key steers the reference
        loop's CudaGraphModule wrappers, orchestrator.py:313-315, which must stay off around these methods).
        `metrics`: "tensor" = update_* return 0-dim float32 CUDA tensors that alias the engine's metrics slots (zero copy; what
        `tlog.update(...)` of orchestrator.py:302,341,348 expects -- a TensorDict takes them as is, and they are only read at
        evaluation time, :383); "lazy" = host-side LazyMetric handles (no torch needed)."""
        if init not in ("torch", "engine"):
            raise ValueError(f'init is "torch" or "engine", not {init!r}')
        ob_dim, ac_dim = int(net_shapes["ob_shape"][-1]), int(net_shapes["ac_shape"][-1])
        self.device, self.hps = device, hps
        self.resets_so_far = 0      # reset_networks() calls: run-time state, not part of a checkpoint
        self.min_ac, self.max_ac = np.asarray(min_ac, np.float32), np.asarray(max_ac, np.float32)
        self.timesteps_so_far = 0
        self.actor_updates_so_far = 0
        self.qnet_updates_so_far = 0
        self.best_eval_ep_ret = -float("inf")  # updated by the orchestrator (orchestrator.py:376-379)
        dev_index = getattr(device, "index", None)
        over = dict(device_id=int(dev_index or 0))
        if seed is not None:
            over["seed"] = int(seed)
        if rb is not None:
            over["rb_capacity"] = rb.capacity
        if use_graphs is not None:
            over["use_graphs"] = bool(use_graphs)
        cfg = Config.from_hps(hps, ob_dim, ac_dim, **over)
        assert getattr(hps, "segment_len", 1) <= cfg.batch_size  # agents/agent.py:47
        self.ob_dim, self.ac_dim, self.td3, self.ln = ob_dim, ac_dim, cfg.prefer_td3_over_sac, cfg.layer_norm
        self.engine = Engine(cfg, self.min_ac, self.max_ac)
        self._metric_tensors: Optional[Dict[str, Any]] = None
        self._ext_stream = None
        if metrics != "lazy":   # 0-dim device tensors over the engine's metrics slots (what the reference's update_* return)
            try:
                import torch
                if torch.cuda.is_available():
                    st, mp = self.engine.device_handles()
                    dev = torch.device("cuda", cfg.device_id)
                    self._metric_tensors = {k: torch.as_tensor(_DeviceScalar(mp + 4 * i), device=dev) for k, i in _METRIC_SLOT.items()}
                    self._ext_stream = torch.cuda.ExternalStream(st, device=dev)
            except Exception:   # noqa: BLE001 -- no torch / no cuda array interface: the lazy host-side handles remain
                self._metric_tensors = None
        self.rb = rb
        if rb is not None:
            rb._bind(self.engine)
        if init_params and init == "engine":
            self.engine.init_params(_init_what(("actor", "critics", "alpha"), self.td3), epoch=0)
        elif init_params:  # agents/nets.py:34-49 under the caller's torch seed (main.py:146)
            actor, critics = schema.reference_initial_params(ob_dim, ac_dim, self.td3, self.ln)
            self.load_flat(actor, critics)

    def reset_networks(self, what=("actor", "critics", "alpha")) -> int:
        """Start the networks `what` names over and keep the replay ring (Nikishin et al. 2022; D'Oro et al. 2023): the engine's own
        initialiser at epoch resets_so_far + 1 under the engine's seed -- fresh orthogonal weights, targets a copy, optimiser state
        cleared; "alpha" puts the temperature back to alpha_init (a TD3 agent has none: the name is dropped silently).  One call on
        the engine's stream; nothing waits, no captured graph is dropped.  -> resets_so_far, which counts these calls.  Like the
        pinned rows of a replay buffer, resets_so_far is run-time state and is NOT saved in a checkpoint: a resumed run starts its
        epochs at 1 again."""
        bits = _init_what(what, self.td3)
        self.engine.init_params(bits, epoch=self.resets_so_far + 1)
        self.resets_so_far += 1
        return self.resets_so_far

    # -- parameters
    def load_flat(self, actor: np.ndarray, critics: np.ndarray, also_targets: bool = True) -> None:
        e = self.engine
        e.set_params(_lib.ACTOR, actor)
        e.set_params(_lib.CRITICS, critics)
        if also_targets:  # agents/agent.py:64,107: targets start as clones
            e.set_params(_lib.ACTOR_TARGET, actor)
            e.set_params(_lib.CRITICS_TARGET, critics)

    def _nh(self) -> int:
        return self.ac_dim if self.td3 else 2 * self.ac_dim

    def state_dicts(self) -> Dict[str, Dict[str, np.ndarray]]:
        """{"actor", "qnet1", "qnet2"} with the reference's key names (agents/agent.py:346-348), LIVE weights."""
        e = self.engine
        scale, bias = (self.max_ac - self.min_ac) / 2.0, (self.max_ac + self.min_ac) / 2.0
        actor = schema.flat_to_dict(e.get_params(_lib.ACTOR), self.ob_dim, self._nh(), self.ln)
        actor["action_scale"], actor["action_bias"] = np.broadcast_to(scale, (self.ac_dim,)).copy(), np.broadcast_to(bias, (self.ac_dim,)).copy()
        if self.td3:   # agents/nets.py:139-141: the TD3 actor registers its exploration sigma as a third buffer
            actor["exploration_noise"] = np.asarray(e.cfg.actor_noise_std, np.float32)
        q = e.get_params(_lib.CRITICS).reshape(2, -1)
        return {"actor": actor,
                "qnet1": schema.flat_to_dict(q[0], self.ob_dim + self.ac_dim, 1, self.ln),
                "qnet2": schema.flat_to_dict(q[1], self.ob_dim + self.ac_dim, 1, self.ln)}

    @property
    def alpha(self) -> Optional[float]:  # agents/agent.py:165-170
        return None if self.td3 else float(np.exp(self.engine.get_params(_lib.LOG_ALPHA)[0]))

    # -- the hot path
    def _stage(self, batch) -> None:
        if batch is None:
            return  # whatever is in the engine's batch slot
        if isinstance(batch, BatchHandle):
            if batch._engine is not self.engine:
                raise StaleBatchError("this batch handle belongs to another agent's replay buffer")
            if not batch._is_current():
                raise StaleBatchError("update called with an old batch handle: the engine's batch slot holds a later sample "
                                      "(keep the rows, e.g. dict(handle), to train on them again)")
            return  # already in the engine's batch slot (a device-backed handle too: its tensors are copies OF the slot)
        five = (batch["observations"], batch["actions"], batch["rewards"], batch["next_observations"], batch["dones"])
        dev = _device_route(self.engine, *five)
        if dev is not None:
            self.engine.load_batch_device(dev[0], dev[1], _producer_stream(five[0], self.engine.cfg.device_id))
            return
        self.engine.load_batch(*[_np(x) for x in five])      # (either call replaces the slot's rows: older handles go stale)

    def predict(self, in_td: Mapping[str, Any], *, explore: bool) -> np.ndarray:
        """agents/agent.py:172-181 -> np.ndarray[n, ac_dim] float32 on the host."""
        return self.engine.predict(_np(in_td["observations"]), explore)

    def predict_device(self, in_td: Mapping[str, Any], *, explore: bool, out: Any = None):
        """Acting for an environment that lives on the GPU (include/sactd3.h: sactd3_predict_device): observations [n, ob_dim] in
        the memory of the engine's device -> actions [n, ac_dim], float32, on that device.  Nothing goes through the host and the
        host does not wait: the kernels run on the engine's stream, ordered on the GPU behind what the caller's current stream has
        queued, and that stream is made to wait for them -- the result can be used there at once and the observations may be
        overwritten there next.  The action is, bit for bit, what predict() returns for the same rows at this point of the call
        sequence.  `out`: a preallocated float32 array or view with at least n rows of ac_dim (contiguous inner dimension) to
        write into -- its rows [0, n) are returned; otherwise torch.empty on the current stream.  An observation that is not
        float32, or whose inner dimension is not contiguous, is converted on the device first."""
        eng = self.engine
        o, a = eng.cfg.ob_dim, eng.cfg.ac_dim
        obs = in_td["observations"]
        if not getattr(eng, "device_inputs", False):
            raise TypeError("predict_device: engine.device_inputs is off (predict() takes host data)")
        got = _read_input(eng, obs, o, "f4")
        if got is None:
            raise TypeError("predict_device: the observations are not an array in the memory of the engine's device (predict() takes host data)")
        obs, ptr, n, ld = got
        if out is None:
            out = _torch_alloc(eng, "predict_device")((n, a), "f4")
        out_ptr, out_rows, out_ld = _read_output(eng, out, a, "f4", "predict_device: `out`", n, more_rows=True)
        eng.predict_device(ptr, ld, n, explore, out_ptr, out_ld, _producer_stream(obs, eng.cfg.device_id))
        return out[:n] if out_rows > n else out

    def q_values(self, in_td: Mapping[str, Any], *, target: bool = False, out: Any = None):
        """What the critics think of these rows: vmap(batched_qf) of the reference (agents/agent.py:146-163) on `observations`
        [n, ob_dim] and `actions` [n, ac_dim] -> [2, n, 1] float32, from the online critics or (`target`) the target pair, computed
        by the engine's own kernels (include/sactd3.h: sactd3_qvalues_device), any n.  Without an `actions` key the pairs are
        (s, pi(s)): pi(s) is what predict(explore=False) returns, scored without leaving the device.
        Routed by where the data lives, as ReplayBuffer.extend is.  Arrays in the memory of the engine's device give a tensor on
        that device: nothing is copied, the host does not wait; the kernels run on the engine's stream, ordered on the GPU behind
        what the caller's current stream has queued, and that stream is made to wait for them.  `out`: a preallocated float32
        [2, >= n, 1] array or view of that device to write into -- its rows [:, :n] are returned; otherwise torch.empty.  A field
        that is not float32, or whose inner dimension is not contiguous, is converted on the device first.  Host arrays give a
        numpy array (and wait for it).  A mix of host and device arrays is a TypeError, as is everything predict_device refuses.
        Training does not see the call: no sample is drawn, no counter moves, a BatchHandle stays current across it."""
        eng = self.engine
        o, a = eng.cfg.ob_dim, eng.cfg.ac_dim
        given = [("observations", in_td["observations"], o)] + ([("actions", in_td["actions"], a)] if "actions" in in_td else [])
        given = [(k, _detached(x), w) for k, x, w in given]
        cais = [_cai(x) for _, x, _ in given]
        if all(c is None for c in cais):                     # host data: numpy out
            if out is not None:
                raise TypeError("q_values: `out` is for arrays in the memory of the engine's device (host arrays return a numpy array)")
            got = eng.q_values(_np(given[0][1]), _np(given[1][1]) if len(given) > 1 else None, target)
            return got.reshape(2, -1, 1)
        if any(c is None for c in cais):
            raise TypeError("q_values: observations and actions must both be host arrays or both be arrays in the memory of the engine's device")
        if not getattr(eng, "device_inputs", False):
            raise TypeError("q_values: engine.device_inputs is off (pass host arrays)")
        got = []
        for (key, x, width), cai in zip(given, cais):
            if not _on_engine_device(eng, x):
                raise TypeError(f"q_values: `{key}` is not an array in the memory of the engine's device")
            got.append(_read_input(eng, x, width, "f4", cai))
        rows = [n for _, _, n, _ in got]
        if len(set(rows)) != 1:
            raise ValueError(f"q_values: observations and actions disagree on the number of rows: {rows}")
        n = rows[0]
        out, q_ptr, q_ld, q_ns, out_rows = _critic_major_out(eng, n, out, "q_values")
        (keep, obs_ptr, _, obs_ld), (_, act_ptr, _, act_ld) = got[0], (got[1] if len(got) > 1 else (None, 0, n, a))
        eng.q_values_device(obs_ptr, obs_ld, act_ptr, act_ld, n, target, q_ptr, q_ld, q_ns, _producer_stream(keep, eng.cfg.device_id))
        return out[:, :n] if out_rows > n else out

    # Agent.policy's keys and the sactd3_policy_io outputs they are: (key, field, width: "a" = ac_dim)
    _POLICY_KEYS = (("mode", "mode", "a"), ("mean", "mean", "a"), ("log_std", "log_std", "a"), ("sample", "sample", "a"),
                    ("sample_log_prob", "sample_logp", 1), ("eps", "eps_out", "a"), ("log_prob", "action_logp", 1))

    def policy(self, in_td: Mapping[str, Any], *, sample: bool = False, target: bool = False, eps: Any = None, out: Any = None) -> Dict[str, Any]:
        """What the actor thinks of these rows (include/sactd3.h: sactd3_policy_device), any n, computed by the engine's own kernels
        on `observations` [n, ob_dim] -> a dict of float32 arrays:
            mode [n, ac_dim]                      the exploit action (what predict(explore=False) computes), always
            mean, log_std [n, ac_dim]             the SAC head's pre-squash mean and log-std (SAC)
            sample [n, ac_dim], sample_log_prob [n, 1], eps [n, ac_dim]
                                                  with `sample=True` or `eps`: a sample, its log-density and the draws it used -- the
                                                  given `eps`, or a stream of the query's own that no training or acting draw shares
            log_prob [n, 1]                       with an `actions` key in `in_td`: log pi(a | s) of those actions under the policy
        `target`: TD3's target actor.  Routed by where the data lives, as q_values is: arrays in the memory of the engine's device give
        tensors on that device, nothing is copied and the host does not wait (ordered on the GPU against the caller's current stream);
        host arrays give numpy arrays; a mix is a TypeError.  `out`: a mapping of preallocated float32 arrays or views of that device
        under the keys above (the log-probs as [n, 1] or [n]).  Training and acting do not see the call."""
        eng = self.engine
        o, a = eng.cfg.ob_dim, eng.cfg.ac_dim
        given = [("observations", in_td["observations"], o)] + ([("actions", in_td["actions"], a)] if "actions" in in_td else [])
        given += [("eps", eps, a)] if eps is not None else []
        given = [(k, _detached(x), w) for k, x, w in given]
        names = {k for k, _, _ in given}
        fields = eng.policy_outputs(bool(sample) or "eps" in names, "actions" in names)
        keys = [(key, f, a if w == "a" else 1) for key, f, w in self._POLICY_KEYS if f in fields]
        cais = [_cai(x) for _, x, _ in given]
        if all(c is None for c in cais):                     # host data: numpy out
            if out is not None:
                raise TypeError("policy: `out` is for arrays in the memory of the engine's device (host arrays return numpy arrays)")
            host = {k: _np(x) for k, x, _ in given}
            got = eng.policy(host["observations"], host.get("actions"), host.get("eps"), sample, target)
            return {key: got[f].reshape(-1, w) for key, f, w in keys}
        if any(c is None for c in cais):
            raise TypeError("policy: observations, actions and eps must all be host arrays or all be arrays in the memory of the engine's device")
        if not getattr(eng, "device_inputs", False):
            raise TypeError("policy: engine.device_inputs is off (pass host arrays)")
        got = {}
        for (key, x, width), cai in zip(given, cais):
            if not _on_engine_device(eng, x):
                raise TypeError(f"policy: `{key}` is not an array in the memory of the engine's device")
            got[key] = _read_input(eng, x, width, "f4", cai)
        rows = [g[2] for g in got.values()]
        if len(set(rows)) != 1:
            raise ValueError(f"policy: observations, actions and eps disagree on the number of rows: {rows}")
        n = rows[0]
        out = dict(out) if out else {}
        if set(out) - {k for k, _, _ in keys}:
            raise ValueError(f"policy: unknown output key(s) {sorted(set(out) - {k for k, _, _ in keys})}: this call fills {[k for k, _, _ in keys]}")
        io = {k: (got[k][1], got[k][3]) for k in ("actions", "eps") if k in got}
        res = {}
        for key, f, w in keys:
            x = out.get(key)
            if x is None:
                x = _torch_alloc(eng, "policy")((n, w), "f4")
            ptr, _, ld = _read_output(eng, x, w, "f4", f"policy: `{key}`", n)
            io[f], res[key] = (ptr, ld), x
        keep = got["observations"][0]
        eng.policy_device(got["observations"][1], got["observations"][3], n, io, target, _producer_stream(keep, eng.cfg.device_id))
        return res

    def td_errors(self, out: Any = None):
        """The per-row TD errors of the most recent critic update (include/sactd3.h: sactd3_td_errors_device): Q_k(s_i, a_i) - y_i as
        the update itself computed them (its Bellman target, its policy draw), signed, per critic -> [2, batch_size, 1] float32 on
        the engine's device; row i is row i of the batch that update trained on.  What a prioritised sampler turns into the next
        priorities, without a second forward pass.  One launch on the engine's stream, no host wait, ordered on the GPU against the
        caller's current stream; training does not see the call.  `out` as for q_values.  Raises EngineError (SACTD3_ESTATE) when no
        critic update has run on the rows now in the batch slot."""
        eng = self.engine
        n = int(eng.cfg.batch_size)
        out, ptr, ld, ns, out_rows = _critic_major_out(eng, n, out, "td_errors")
        eng.td_errors_device(ptr, ld, ns, _producer_stream(out, eng.cfg.device_id))
        return out[:, :n] if out_rows > n else out

    def predict_begin(self, in_td: Mapping[str, Any], *, explore: bool) -> None:
        """predict() in two halves (include/sactd3.h: sactd3_predict_begin): the acting kernels go out on the engine's acting
        stream, and what is issued until predict_end() -- the iteration's update -- overlaps with them."""
        self.engine.predict_begin(_np(in_td["observations"]), explore)

    def predict_end(self) -> np.ndarray:
        """-> np.ndarray[n, ac_dim] float32: the actions of the call begun with predict_begin()."""
        return self.engine.predict_end()

    def _results(self, keys) -> Dict[str, Any]:
        if self._metric_tensors is None:
            return {k: LazyMetric(self, k) for k in keys}
        # the tensors alias memory the engine's stream writes: whoever reads them on torch's current stream does so after the
        # work enqueued so far (an event wait between two streams, no host synchronisation)
        import torch
        torch.cuda.current_stream(self._ext_stream.device).wait_event(self._ext_stream.record_event())
        return {k: self._metric_tensors[k] for k in keys}

    def update_qnets(self, batch) -> Dict[str, Any]:
        """agents/agent.py:183-242.  A mapping batch with a "_weight" key (what torchrl's prioritised sampler adds: float32
        [batch_size] or [batch_size, 1] on the engine's device) is trained on with those per-row loss weights, staged behind the batch
        (include/sactd3.h: sactd3_batch_weights_device); a handle of ReplayBuffer.sample_at() carries its weights already.  The
        weights are never dropped silently: a "_weight" that is not an array on the engine's device (a host array, another GPU's) is a
        TypeError, whichever route the batch's five fields take; a wrong row count is a ValueError."""
        self._stage(batch)
        if batch is not None and not isinstance(batch, BatchHandle) and "_weight" in batch.keys():      # (a TensorDict refuses `key in td`)
            eng = self.engine
            keep, w_ptr, w_ld = _weight_field(eng, batch["_weight"], int(eng.cfg.batch_size), "update_qnets")
            eng.batch_weights_device(w_ptr, w_ld, int(eng.cfg.batch_size), _producer_stream(keep, eng.cfg.device_id))
        self.engine.update_qnets()
        return self._results(["loss/qf_loss"])

    def update_actor(self, batch) -> Dict[str, Any]:
        self._stage(batch)
        self.engine.update_actor()
        keys = ["loss/actor_loss"]
        if not self.td3:  # agents/agent.py:288-318
            if self.engine.cfg.autotune:
                keys.append("loss/alpha_loss")
            keys.append("vitals/alpha")
        if self.engine.cfg.bc_alpha > 0:      # TD3+BC (hps.bc_alpha): the unweighted BC term and lambda of this update
            keys += ["loss/bc_loss", "vitals/bc_lambda"]
        return self._results(keys)

    def update_targ_nets(self) -> None:
        self.engine.update_targ_nets(self.qnet_updates_so_far)

    def iteration(self, i: int, *, beta: Optional[float] = None, n_step: int = 1, stride: Optional[int] = None,
                  prior_rows: Optional[int] = None, hindsight: bool = False) -> None:
        """orchestrator.py:337-352 as ONE graph launch (sample, critic, delayed actor x N, Polyak); keeps the
        reference's counters.  `beta` (needs ReplayBuffer.enable_priorities): the sample is drawn by priority, the critic update is
        weighted by the importance weights of exponent beta and its TD errors go back into the priorities; `n_step`, `stride`: as for
        ReplayBuffer.sample -- all inside the same launch (include/sactd3.h: sactd3_step_sampled), equal to the call sequence
        sample_prioritized / sample -> update_qnets -> update_priorities -> update_actor x N -> update_targ_nets bit for bit.
        `prior_rows` (needs ReplayBuffer.pin): the sample is ReplayBuffer.sample_mixed's, inside the same launch; it excludes
        `beta` and n_step > 1.
        `hindsight=True` (needs ReplayBuffer.configure_hindsight): the sample is ReplayBuffer.sample_hindsight's, drawn and relabelled
        inside the same launch; it excludes `beta`, n_step > 1 and `prior_rows`."""
        do_actor = i % (self.engine.cfg.actor_update_delay + 1) == 0
        if hindsight:
            if beta is not None or n_step != 1 or prior_rows is not None:
                raise ValueError("iteration: hindsight (the relabelling draw) excludes beta, n_step > 1 and prior_rows")
            self.engine.step_sampled(do_actor, hindsight=True)
        elif prior_rows is not None:
            if beta is not None or n_step != 1:
                raise ValueError("iteration: prior_rows (the mixed draw) excludes beta and n_step > 1")
            self.engine.step_sampled(do_actor, prior_rows=int(prior_rows))
        elif beta is None and n_step == 1 and stride is None:
            self.engine.step(do_actor)
        else:
            n_step, stride = _n_step_args("iteration", n_step, stride)
            self.engine.step_sampled(do_actor, beta=None if beta is None else float(beta), n_step=n_step, stride=stride)
        self.qnet_updates_so_far += 1
        if do_actor:
            self.actor_updates_so_far += self.engine.cfg.actor_update_delay

    # -- checkpoints (agents/agent.py:333-371): the reference's .pth schema, with LIVE critic weights
    def _plain_hps(self) -> Dict[str, Any]:
        """`hps` as a plain mapping of builtin scalars (the reference stores its DictConfig object, agents/agent.py:343:
        only a pickling loader can read that back; a plain dict also loads with torch.load(weights_only=True))."""
        h = self.hps
        try:
            items = dict(h).items() if hasattr(h, "keys") else vars(h).items()
        except TypeError:
            items = {}
        return {str(k): v for k, v in items if isinstance(v, (bool, int, float, str)) or v is None}

    def _adam_state_dict(self, which: int, shapes, lr: float, stacked: int):
        """torch.optim.Adam.state_dict() of the optimiser that owns `which`, in the reference's form: parameters in
        `module.parameters()` order (= state_dict order), the twin critics as the dense-stacked [2, ...] tensors of
        agents/agent.py:106-119 under ONE Adam instance, per-parameter `step` / `exp_avg` / `exp_avg_sq`, torch's own
        `param_groups`.  Built by filling a real torch.optim.Adam, so the layout is whatever this torch version writes."""
        import torch
        m, v, step = self.engine.get_adam_state(which)
        m, v = m.reshape(max(stacked, 1), -1), v.reshape(max(stacked, 1), -1)
        params, off = [], 0
        mv = []
        for _, shp in shapes:
            n = int(np.prod(shp))
            full = ((stacked,) if stacked else ()) + tuple(shp)
            params.append(torch.nn.Parameter(torch.zeros(full)))
            take = (lambda a: a[:, off:off + n].reshape(full)) if stacked else (lambda a: a[0, off:off + n].reshape(full))
            mv.append((torch.from_numpy(np.ascontiguousarray(take(m))), torch.from_numpy(np.ascontiguousarray(take(v)))))
            off += n
        opt = torch.optim.Adam(params, lr=lr, betas=(self.engine.cfg.adam_beta1, self.engine.cfg.adam_beta2), eps=self.engine.cfg.adam_eps)
        if step > 0:                                   # torch creates the state lazily, at the first step
            for p_, (m_, v_) in zip(params, mv):
                opt.state[p_] = {"step": torch.tensor(float(step)), "exp_avg": m_, "exp_avg_sq": v_}
        return opt.state_dict()

    def save(self, path: Path, sfx: Optional[str] = None) -> Path:
        """agents/agent.py:333-358 (wandb upload aside): keys `hps`, `timesteps_so_far`, `actor`, `qnet1`, `qnet2`,
        `actor_optimizer`, `q_optimizer` as the reference writes them -- its own `load_from_disk` (:360-371) accepts the file --
        plus `engine_resume` (what the reference does not save: targets, log_alpha and its optimiser, every step count) for
        a bit-exact resume of this engine."""
        import torch
        fname = f"ckpt_{sfx}" if sfx is not None else f".ckpt_{self.timesteps_so_far}ts"
        path = Path(path) / f"{fname}.pth"
        sds = {k: {kk: torch.from_numpy(np.ascontiguousarray(vv)) for kk, vv in v.items()} for k, v in self.state_dicts().items()}
        e, c = self.engine, self.engine.cfg
        ck = {"hps": self._plain_hps(), "timesteps_so_far": self.timesteps_so_far, **sds,
              "actor_optimizer": self._adam_state_dict(_lib.ACTOR, schema.net_keys(self.ob_dim, self._nh(), self.ln), c.actor_lr, 0),
              "q_optimizer": self._adam_state_dict(_lib.CRITICS, schema.net_keys(self.ob_dim + self.ac_dim, 1, self.ln), c.qnets_lr, 2)}
        extra = {}
        for name, which in (("actor", _lib.ACTOR), ("critics", _lib.CRITICS), ("log_alpha", _lib.LOG_ALPHA)):
            m, v, step = e.get_adam_state(which)
            extra[f"adam/{name}"] = {"exp_avg": torch.from_numpy(m), "exp_avg_sq": torch.from_numpy(v), "step": step}
        extra["actor_target"] = torch.from_numpy(e.get_params(_lib.ACTOR_TARGET))
        extra["critics_target"] = torch.from_numpy(e.get_params(_lib.CRITICS_TARGET))
        extra["log_alpha"] = float(e.get_params(_lib.LOG_ALPHA)[0])
        ck["engine_resume"] = extra
        torch.save(ck, path)
        return path

    @staticmethod
    def _adam_from_state_dict(sd, stacked: int):
        """(exp_avg flat, exp_avg_sq flat, step) in the engine's layout from a torch Adam state_dict (see _adam_state_dict)."""
        st = sd["state"]
        if not st:
            return None
        idx = sorted(st)
        f = lambda key: np.concatenate([st[i][key].detach().cpu().numpy().astype(np.float32).reshape(max(stacked, 1), -1) for i in idx], 1).reshape(-1)
        return f("exp_avg"), f("exp_avg_sq"), int(round(float(st[idx[0]]["step"])))

    @staticmethod
    def compare_hps(saved: Mapping[str, Any], current: Mapping[str, Any]) -> Dict[str, Dict[str, Any]]:
        """agents/agent.py:373-401 (`compare_dictconfigs`): depth-1 comparison of two configs -> {"added", "removed", "changed"}
        (`added`: keys only the current config has; `removed`: keys only the saved one has; `changed`: {"from": saved, "to": current})."""
        diff: Dict[str, Dict[str, Any]] = {"added": {}, "removed": {}, "changed": {}}
        k1, k2 = set(saved.keys()), set(current.keys())
        for k in sorted(k2 - k1):
            diff["added"][k] = current[k]
        for k in sorted(k1 - k2):
            diff["removed"][k] = saved[k]
        for k in sorted(k1 & k2):
            if saved[k] != current[k]:
                diff["changed"][k] = {"from": saved[k], "to": current[k]}
        return diff

    def load_from_disk(self, path: Path) -> None:
        """agents/agent.py:360-371.  Reads files written by `save` above and any file in the reference's schema that a
        weights-only loader accepts (state_dicts + optimiser state_dicts of tensors and builtin scalars).  A .pth written
        by the reference itself pickles its OmegaConf DictConfig under `hps`: torch.load(weights_only=True) refuses it,
        and this loader is deliberately not loosened."""
        import torch
        ck = torch.load(path, weights_only=True)
        # the reference compares the saved run's config with the current one and reports added / removed / changed keys before
        # it loads (agents/agent.py:411-415, there against the wandb run's config); here against the checkpoint's own `hps`
        self.last_hps_diff = self.compare_hps(ck["hps"], self._plain_hps()) if isinstance(ck.get("hps"), dict) else None
        if self.last_hps_diff and any(self.last_hps_diff.values()):
            import warnings
            d = self.last_hps_diff
            warnings.warn(f"checkpoint hps differ from this agent's -- added: {d['added']}  removed: {d['removed']}  changed: {d['changed']}")
        if "timesteps_so_far" in ck:
            self.timesteps_so_far = ck["timesteps_so_far"]
        actor = schema.dict_to_flat(ck["actor"], self.ob_dim, self._nh(), self.ln)
        q = [schema.dict_to_flat(ck[k], self.ob_dim + self.ac_dim, 1, self.ln) for k in ("qnet1", "qnet2")]
        ex = ck.get("engine_resume")
        e = self.engine
        n_a, n_c = e.param_count(_lib.ACTOR), e.param_count(_lib.CRITICS)
        if ex:   # validate before touching the engine: a blob from other dims / layer_norm setting must not reach the C side
            for name, n in (("actor", n_a), ("critics", n_c), ("log_alpha", 1)):
                st = ex[f"adam/{name}"]
                if st["exp_avg"].numel() != n or st["exp_avg_sq"].numel() != n:
                    raise ValueError(f"engine_resume: adam/{name} holds {st['exp_avg'].numel()} values, this agent needs {n}")
            if ex["actor_target"].numel() != n_a or ex["critics_target"].numel() != n_c:
                raise ValueError("engine_resume: target networks of another shape")
        self.load_flat(actor, np.concatenate(q), also_targets=not ex)
        if ex:
            e.set_params(_lib.ACTOR_TARGET, ex["actor_target"].numpy())
            e.set_params(_lib.CRITICS_TARGET, ex["critics_target"].numpy())
            e.set_params(_lib.LOG_ALPHA, np.array([ex["log_alpha"]], np.float32))
            for name, which in (("actor", _lib.ACTOR), ("critics", _lib.CRITICS), ("log_alpha", _lib.LOG_ALPHA)):
                st = ex[f"adam/{name}"]
                e.set_adam_state(which, st["exp_avg"].numpy(), st["exp_avg_sq"].numpy(), int(st["step"]))
        else:    # the reference's own keys only (agents/agent.py:368-369): optimiser moments and step counts
            for key, which, stacked in (("actor_optimizer", _lib.ACTOR, 0), ("q_optimizer", _lib.CRITICS, 2)):
                got = self._adam_from_state_dict(ck[key], stacked) if key in ck else None
                if got is not None:
                    e.set_adam_state(which, *got)
