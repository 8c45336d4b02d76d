"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  A plain restatement of the dormant-neuron scan and of ReDo's redraw
(include/sactd3_dormant.h, csrc/dormant_kernels.h), in torch at a dtype of the caller's choice (float64: the reference; float32 on the
CPU: the yardstick of the tolerance).  Used by tests/test_gpu_dormant.py.

This is not a test module, so pytest does not rewrite its asserts: every assert here carries its own message."""
import numpy as np
import torch

from oracle import replay_ref
from tests import bounds, init_model, noise_model

HID, STREAM_REDO = 256, 0xA00


def hidden(flat, K, nh, ln, x, dtype):
    """[h1, h2], each [n, 256]: h = relu(LN(W x + b)) of one net's two hidden layers on the leading K columns of x; LN two-pass, eps
    inside the root, the identity without layer_norm"""
    p = {(kind, layer): torch.as_tensor(np.array(v), dtype=dtype) for kind, layer, v in init_model.split(flat, K, nh, ln)}
    h, out = torch.as_tensor(np.asarray(x)[:, :K], dtype=dtype), []
    for layer in (0, 1):
        z = h @ p[("weight", layer)].T + p[("bias", layer)]
        if ln:
            d = z - z.mean(1, keepdim=True)
            z = d / torch.sqrt((d * d).mean(1, keepdim=True) + 1e-5) * p[("ln_weight", layer)] + p[("ln_bias", layer)]
        h = torch.relu(z)
        out.append(h)
    return out


def scores(params, o, a, td3, ln, x, dtype):
    """[6, 256] float64 numpy: eq. 1 of Sokar et al. for the six (net, layer) pairs over the rows x = [s | a], computed in `dtype`"""
    out = []
    for _, K, nh, flat in init_model.nets_of(params, o, a, td3):
        for h in hidden(flat, K, nh, ln, x, dtype):
            m = h.mean(0)
            mean = m.mean()
            out.append((m / mean if mean > 0 else torch.zeros_like(m)).double().numpy())
    return np.stack(out)


def redraw64(seed, mat, epoch, i, K):
    """(w, bound) [K] float64: row i of matrix `mat` as sactd3_redo draws it -- z (c / |z|), z_j lane e & 3, e = i K + j, of the block
    (epoch, mat, 0xA00, e >> 2) -- and its a-priori bound: the per-draw bound of tests/noise_model.py carried through the scale, plus
    one rounding per fp32 operation of the normalisation (K products and K sums of the squares, the root, the division, the product)"""
    e = (i * K + np.arange(K)).astype(np.uint64)
    r = replay_ref.philox4x32_10(np.full(K, epoch & 0xFFFFFFFF), mat, STREAM_REDO, e >> np.uint64(2), seed & 0xFFFFFFFF, seed >> 32)
    k = (e & np.uint64(3)).astype(np.int64)
    u1, u2 = noise_model.u01(np.where(k < 2, r[0], r[2])), noise_model.u01(np.where(k < 2, r[1], r[3]))
    z, b = noise_model.bound(u1, u2, (k & 1).astype(bool))
    nrm, c = np.sqrt(z @ z), np.sqrt(min(1.0, K / HID))
    w = z * (c / nrm)
    rel_scale = np.sqrt(b @ b) / nrm + (2 * K + 3) * bounds.U      # d|z| / |z| <= |b| / |z|; then the roundings
    return w, b * (c / nrm) + np.abs(w) * (rel_scale + bounds.U), c
