"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  A float64 model of the engine's parameter initialiser (include/sactd3_init.h,
csrc/param_init_kernels.h): the Philox counter words -> Box-Muller -> Gram-Schmidt with the positive-diagonal convention.  Used by
tests/test_gpu_param_init.py.

The draw: element e = i n + j of the Gaussian G [m, n] (m = max(rows, cols), n = min(rows, cols)) behind weight matrix `mat` in
reset epoch E is lane e & 3 of the Philox block with counter words (E, mat | attempt << 16, 0x700, e >> 2) keyed by the seed; the
block's words v0 .. v3 give two Box-Muller pairs exactly as for the engine's noise (tests/noise_model.py: the uniforms are the exact
fp32 values, everything behind them is float64).  The orthogonalisation: classical Gram-Schmidt applied twice in float64, a column
divided by its norm -- the Q of the QR factorisation whose R has a positive diagonal, torch.nn.init.orthogonal_'s convention at gain 1
(agents/nets.py:35-47).  W = Q for rows >= cols, else Q^T.  Matrix ids: actor layers 0, 1, 2; critic net n, layer l: 3 + 3 n + l.

This is not a test module, so pytest does not rewrite its asserts: every assert here carries its own message."""
import functools

import numpy as np

from oracle import replay_ref
from tests import noise_model

STREAM_INIT = 0x700
HID = 256
INIT_ACTOR, INIT_CRITICS, INIT_ALPHA = 1, 2, 4      # include/sactd3_init.h


def matrices(o, a, td3):
    """mat -> (rows, cols) of every weight matrix of an engine, and the net it belongs to: [(mat, net, layer, rows, cols)], net 0 = the
    actor, 1 / 2 = the critics"""
    nh = a if td3 else 2 * a
    out = []
    for net in range(3):
        K, head = (o, nh) if net == 0 else (o + a, 1)
        for layer, (rows, cols) in enumerate(((HID, K), (HID, HID), (head, HID))):
            out.append((3 * net + layer, net, layer, rows, cols))
    return out


def gaussian64(seed, mat, epoch, rows, cols, attempt=0):
    """G [max(rows, cols), min(rows, cols)] float64: the normals of the exact fp32 uniforms"""
    m, n = max(rows, cols), min(rows, cols)
    e = np.arange(m * n, dtype=np.uint64)
    r = replay_ref.philox4x32_10(np.full(m * n, epoch & 0xFFFFFFFF), mat | (attempt << 16), STREAM_INIT, e >> np.uint64(2),
                                 seed & 0xFFFFFFFF, seed >> 32)
    k = (e & np.uint64(3)).astype(np.int64)
    u1, u2 = noise_model.u01(np.where(k < 2, r[0], r[2])), noise_model.u01(np.where(k < 2, r[1], r[3]))
    z, _ = noise_model.bound(u1, u2, (k & 1).astype(bool))
    return z.reshape(m, n)


def gram_schmidt64(G):
    """Q of G = Q R with diag(R) > 0, by classical Gram-Schmidt applied twice, in float64"""
    G = np.asarray(G, np.float64)
    Q = np.zeros_like(G)
    for j in range(G.shape[1]):
        v = G[:, j].copy()
        for _ in range(2):
            v -= Q[:, :j] @ (Q[:, :j].T @ v)
        nrm = np.sqrt(v @ v)
        assert nrm > 0.0 and np.isfinite(nrm), ("gram_schmidt64", "a column vanished", j)
        Q[:, j] = v / nrm
    return Q


@functools.lru_cache(maxsize=64)
def weight64(seed, mat, epoch, rows, cols):
    """(W [rows, cols] float64, its G): read-only, computed once"""
    G = gaussian64(seed, mat, epoch, rows, cols)
    Q = gram_schmidt64(G)
    W = Q if rows >= cols else Q.T
    W = np.ascontiguousarray(W)
    W.setflags(write=False)
    G.setflags(write=False)
    return W, G


def net_keys(in_dim, n_head, ln):
    """the state_dict order of one net: [(kind, layer, shape)], kind in weight / bias / ln_weight / ln_bias (include/sactd3.h)"""
    keys = []
    for layer, n_in in ((0, in_dim), (1, HID)):
        keys += [("weight", layer, (HID, n_in)), ("bias", layer, (HID,))]
        if ln:
            keys += [("ln_weight", layer, (HID,)), ("ln_bias", layer, (HID,))]
    return keys + [("weight", 2, (n_head, HID)), ("bias", 2, (n_head,))]


def split(flat, in_dim, n_head, ln):
    """one net's flat parameter vector -> [(kind, layer, array)]"""
    flat = np.asarray(flat).reshape(-1)
    out, off = [], 0
    for kind, layer, shape in net_keys(in_dim, n_head, ln):
        n = int(np.prod(shape))
        out.append((kind, layer, flat[off:off + n].reshape(shape)))
        off += n
    assert off == flat.size, ("split", "the vector is not one net of this shape", off, flat.size)
    return out


def nets_of(params, o, a, td3):
    """{"actor": flat, "critics": flat} (get_params) -> [(net, in_dim, n_head, flat of that net)]"""
    nh = a if td3 else 2 * a
    q = np.asarray(params["critics"]).reshape(2, -1)
    return [(0, o, nh, np.asarray(params["actor"])), (1, o + a, 1, q[0]), (2, o + a, 1, q[1])]
