"""Shared synthetic-data helpers for the tests (shapes from SURVEY.md section 8d)."""
import os
from types import SimpleNamespace

import numpy as np
import torch

# CPU numerics that do not depend on the host.  MKL and ATen pick their GEMM / vector kernels by CPU vendor and instruction set,
# and the number of threads decides how a product or a reduction is split, so fp32 results differ in the last bits from machine
# to machine.  tests/golden/ holds bit-exact vectors, and the sign-like first Adam steps the oracle tests compare hinge on those
# bits: those tests (in_pinned_cpu_process) and the fixture generator (tests/golden/make_golden.py) compute with MKL's
# conditional numerical reproducibility on its COMPATIBLE code path, ATen's AVX2 kernels and one thread.  (MKL's AVX2 branch
# gives the same GEMMs on Intel and AMD processors but not the same vector exp / log, which torch takes from MKL.)  MKL and
# ATen read these variables at their first computation, so they are set before any.  The rest of the suite keeps the host's
# defaults: the GPU parity tolerances were measured against the oracle computed that way.
PINNED_CPU_ENV = {"MKL_CBWR": "COMPATIBLE", "ATEN_CPU_CAPABILITY": "avx2", "OMP_NUM_THREADS": "1", "MKL_NUM_THREADS": "1"}
_PINNED_FLAG = "SACTD3_TESTS_PINNED_CPU"


def pin_cpu_numerics():
    os.environ.update(PINNED_CPU_ENV)
    torch.set_num_threads(1)


def in_pinned_cpu_process(request):
    """True in a test process started with PINNED_CPU_ENV.  Anywhere else: run the calling test (request.node) again in a fresh
    pytest process with PINNED_CPU_ENV, require it to pass, and return False -- the caller then returns."""
    if os.environ.get(_PINNED_FLAG) == "1":
        assert torch.backends.cpu.get_cpu_capability() == "AVX2" and torch.get_num_threads() == 1, (
            "CPU numerics not pinned", torch.backends.cpu.get_cpu_capability(), torch.get_num_threads())
        return True
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "pytest", "-q", "-p", "no:cacheprovider", request.node.nodeid]
    out = subprocess.run(cmd, cwd=root, env=dict(os.environ, **PINNED_CPU_ENV, **{_PINNED_FLAG: "1"}), capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    return False


DIMS = {"hopper": (11, 3, 1.0), "halfcheetah": (17, 6, 1.0), "humanoid": (376, 17, 0.4),
        # not environments of BASELINE.json: shapes that take the remaining branches of the narrow-head kernels (4 actions under SAC:
        # an 8-wide head with 16-float dQ/da partials in 8 tiles; 2 actions under TD3: 8-float partials in 16 tiles; 7 actions: the widest
        # action vector the folded dQ/da takes)
        "sac4": (9, 4, 1.0), "td3_2": (5, 2, 2.0), "td3_7": (13, 7, 1.0),
        # the widest head (nh = 64 under SAC) and odd widths on both sides of the fused first layer's 64 inputs, at large batch
        "o3a32": (3, 32, 0.7), "o48a17": (48, 17, 0.7),
        # tests/test_gpu_tail_edges.py: 5 actions under SAC (nh = 10: the general tail and head backward below the large-batch
        # threshold); 8 actions under TD3 (the narrow head without the folded dQ/da)
        "sac5": (7, 5, 1.0), "td3_8": (10, 8, 1.0)}


def synth_transitions(n, o, a, bound, seed=0):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(n, o, generator=g)
    nobs = torch.randn(n, o, generator=g)
    act = (torch.rand(n, a, generator=g) * 2 - 1) * bound
    rew = torch.randn(n, generator=g)
    done = (torch.rand(n, generator=g) < 0.01)
    return obs, act, rew, nobs, done


def randomize_ln(agent, seed=1):
    """LN gamma/beta start at 1/0; perturb them (and biases) so their gradients are exercised."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        nets = [agent.actor, *agent.qnets]
        for net in nets:
            for k, p in net.named_parameters():
                if k.endswith("ln.weight") or k.endswith("bias"):
                    p.add_(0.1 * torch.randn(p.shape, generator=g))
        agent.actor_target.load_state_dict(agent.actor.state_dict())
        agent.qnets_target.load_state_dict(agent.qnets.state_dict())
        # make targets differ from online nets
        for net in [agent.actor_target, *agent.qnets_target]:
            for p in net.parameters():
                p.add_(0.01 * torch.randn(p.shape, generator=g))


class FakeDeviceArray:
    """a stand-in for a device array on the CPU -- what the mirror's routing helper may rely on: __cuda_array_interface__
    (version 3), detach(), and the array library's own conversions"""
    _next = 0x7F0000000000

    def __init__(self, shape, typestr="<f4", strides=None, device_index=0, log=None):
        FakeDeviceArray._next += 1 << 20
        self.ptr, self.shape, self.typestr, self.strides = FakeDeviceArray._next, tuple(shape), typestr, strides
        self.device = SimpleNamespace(index=device_index)
        self.log = [] if log is None else log

    @property
    def __cuda_array_interface__(self):
        return {"shape": self.shape, "typestr": self.typestr, "data": (self.ptr, False), "version": 3, "strides": self.strides}

    def detach(self):
        return self

    def to(self, dtype):
        return FakeDeviceArray(self.shape, "<f4", None, self.device.index, self.log + [("to", str(dtype))])

    def contiguous(self):
        return FakeDeviceArray(self.shape, self.typestr, None, self.device.index, self.log + ["contiguous"])

    def __ne__(self, other):
        assert other == 0
        return FakeDeviceArray(self.shape, "|b1", None, self.device.index, self.log + ["!= 0"])

    def cpu(self):
        raise AssertionError("the device route must not copy to the host")


def five(n=8, o=11, a=3, **over):
    """[obs, act, rew, nobs, done] as FakeDeviceArrays of n rows; `over` replaces fields by name"""
    d = dict(obs=FakeDeviceArray((n, o)), act=FakeDeviceArray((n, a)), rew=FakeDeviceArray((n,)), nobs=FakeDeviceArray((n, o)),
             done=FakeDeviceArray((n,), "|b1"))
    d.update(over)
    return [d[k] for k in ("obs", "act", "rew", "nobs", "done")]


class SlotGeneration:
    """a fake engine's share of the engine's rule (include/sactd3.h: sactd3_batch_generation): it calls slot_refilled() from every
    method that puts new rows into the batch slot, and from no other"""
    _generation = 5

    def batch_generation(self):
        return self._generation

    def slot_refilled(self):
        self._generation += 1


# ---- observed parity deltas: tests report what they measured, the session writes it out (tests/conftest.py), and the
# tolerances in the tests are set from these records (<= 2x the observed value, never above north_star's 1e-5 per step)
OBSERVED = {}


def observe(test, key, value):
    """keep the LARGEST value seen for (test, key)"""
    d = OBSERVED.setdefault(test, {})
    d[key] = max(float(value), d.get(key, 0.0))


def param_keys(in_dim, nh, ln, nets=1):
    """[(name, start, stop)] over a flat parameter vector of `nets` networks back to back (sac-td3..._amd/schema.py order)"""
    from sac_td3_cudagraphs_pytorch_amd import schema
    out, off = [], 0
    for n in range(nets):
        for k, shp in schema.net_keys(in_dim, nh, ln):
            size = int(np.prod(shp))
            out.append((f"net{n}.{k}" if nets > 1 else k, off, off + size))
            off += size
    return out


def assert_params_close(got, want, lr, steps, name="", atol=2e-5, rtol=1e-5, max_bad_frac=1e-3, layout=None, vec_bad=1, record=None, max_lr_steps=None):
    """Post-Adam parameter parity.

    Adam's early steps are sign-like (p -= lr * g / (|g| + eps')), so an element whose gradient
    sits below the fp32 noise floor of its reduction (|g| <~ 1e-6 * max|g|) moves by +-lr in a
    direction that depends on summation order.  Those elements are legitimately unpredictable across
    implementations; everything else must agree tightly.  So: at most `max_bad_frac` of the elements
    may exceed (atol, rtol), and none may differ by more than 2 * lr * steps (+ atol).

    With `layout` = (in_dim, n_head, layer_norm, nets) the check is made PER state_dict KEY: a weight matrix may
    have `max_bad_frac` of its elements off, a vector (bias, LayerNorm affine, 1-row head) at most `vec_bad`
    elements -- a global fraction would let every bias and LN vector of a net (about 1 % of its elements) step
    the wrong way unnoticed.  `record` = test name: report the observed worst fractions (helpers.observe).
    `max_lr_steps`: the cap on any single element's difference in units of lr (default 2 x steps: every step the other way).
    """
    got = torch.as_tensor(got, dtype=torch.float32).reshape(-1).cpu()
    want = torch.as_tensor(want, dtype=torch.float32).reshape(-1).cpu()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    diff = (got - want).abs()
    bad = diff > (atol + rtol * want.abs())
    cap = (2.0 * steps if max_lr_steps is None else max_lr_steps) * lr + atol
    assert diff.max().item() <= cap, f"{name}: max diff {diff.max().item():.3e} > {cap:.3e}"
    if layout is None:
        frac = bad.float().mean().item()
        assert frac <= max_bad_frac, f"{name}: {frac:.2e} of elements off (max diff {diff.max().item():.3e})"
        return
    keys = param_keys(*layout)
    assert keys[-1][2] == got.numel(), (name, keys[-1][2], got.numel())
    worst_mat, worst_vec = 0.0, 0
    for k, lo, hi in keys:
        nbad, n = int(bad[lo:hi].sum()), hi - lo
        is_vec = k.endswith(("bias", "ln.weight")) or n <= 512
        if is_vec:
            worst_vec = max(worst_vec, nbad)
            assert nbad <= vec_bad, f"{name} {k}: {nbad} of {n} elements off (max diff {diff[lo:hi].max().item():.3e})"
        else:
            worst_mat = max(worst_mat, nbad / n)
            assert nbad / n <= max_bad_frac, f"{name} {k}: {nbad / n:.2e} of elements off (max diff {diff[lo:hi].max().item():.3e})"
    if record:
        observe(record, f"{name}: max diff / lr", diff.max().item() / lr)
        observe(record, f"{name}: worst matrix bad fraction", worst_mat)
        observe(record, f"{name}: worst vector bad count", worst_vec)
