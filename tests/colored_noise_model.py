"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  The float64 restatement of include/sactd3_noise.h's process and the a-priori bound of the
device's fp32 result around it.  Checked on the CPU by tests/test_colored_noise_model.py; used by tests/test_gpu_colored_noise.py.

Philox words from oracle/replay_ref.py, uniforms, normals and their per-element device bound from tests/noise_model.py.  The amplitude
table is the fp32-rounded one the product uploads, recomputed here in float64 (never read from the product); the signal is numpy's irfft.

The bound on |x^[t] - x[t]| for the pair of sequences (2b, 2b + 1) that share a transform is the sum of
  1. the draw error, elementwise: sum_k a_k (b_{2k} + b_{2k+1}), b the noise_model bound of each normal, the unused imaginary parts of
     k = 0 and k = L / 2 left out;
  2. the transform's rounding, normwise (Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2): s eta / (1 - s eta) times
     ||(x_A, x_B)||_2, with s = log2 L + 2 levels (the coefficient scaling and the A + iB packing are the two extra ones; the constants
     inside a radix-8 / radix-16 butterfly are twiddle levels inside log2 L), eta = mu + gamma_4 (sqrt 2 + mu), gamma_4 = 4u / (1 - 4u),
     u = 2^-24 and mu = u: the twiddles are float64 values rounded once.
Nothing in it is observed on the engine.  Not a test module: every assert carries its own message."""
import numpy as np

from oracle import replay_ref
from tests import bounds, noise_model

STREAM_COLORED = 0xB00


def amplitudes(beta, L):
    """a_0 .. a_{L/2} [L/2 + 1] as uploaded: float64, rounded once to fp32 (returned as the exact float64 values of those)"""
    k = np.arange(1, L // 2 + 1, dtype=np.float64)
    v = np.concatenate([[np.sqrt(2.0)], 2.0 * k ** (-0.5 * float(np.float32(beta)))])
    v[-1] /= np.sqrt(2.0)
    return bounds.f64((v / np.sqrt((v * v).sum())).astype(np.float32))


def normals(seed, epoch, chunk, q, L):
    """(g*, bound) [L + 2] of sequence q: normal m is lane m & 3 of the block (chunk, q, 0xB00, (m >> 2) | (epoch << 16))"""
    m = np.arange(L + 2, dtype=np.uint64)
    r = replay_ref.philox4x32_10(np.full(L + 2, chunk & 0xFFFFFFFF), q, STREAM_COLORED, (m >> np.uint64(2)) | np.uint64(epoch << 16),
                                 seed & 0xFFFFFFFF, seed >> 32)
    k = (m & np.uint64(3)).astype(np.int64)
    return noise_model.bound(noise_model.u01(np.where(k < 2, r[0], r[2])), noise_model.u01(np.where(k < 2, r[1], r[3])), (k & 1).astype(bool))


def sequence(a, g):
    """x[0 .. L - 1] of amplitudes a [L/2 + 1] and normals g [L + 2], by irfft"""
    L = 2 * (len(a) - 1)
    Z = 0.5 * L * a * (g[0:L + 2:2] + 1j * g[1:L + 2:2])
    Z[0], Z[-1] = L * a[0] * g[0], L * a[-1] * g[L]
    return np.fft.irfft(Z, n=L)


def chunk(seed, beta, L, S, chunk=0, epoch=0):
    """(x*, bound) [L, S] float64 of one generated chunk"""
    a = amplitudes(beta, L)
    x, draw = np.zeros((L, S)), np.zeros(S)
    for q in range(S):
        g, b = normals(int(seed), int(epoch), int(chunk), q, L)
        x[:, q] = sequence(a, g)
        pair = b[0:L + 2:2] + b[1:L + 2:2]
        pair[0], pair[-1] = b[0], b[L]
        draw[q] = (a * pair).sum()
    u = bounds.U
    assert u == 2.0 ** -24, ("colored_noise_model", "bounds.U is not the fp32 unit roundoff", u)
    g4 = 4 * u / (1 - 4 * u)
    s_eta = (np.log2(L) + 2) * (u + g4 * (np.sqrt(2.0) + u))
    pad = np.concatenate([x, np.zeros((L, S & 1))], 1)
    norm = np.sqrt((pad ** 2).reshape(L, -1, 2).sum((0, 2)))            # per pair
    return x, draw[None, :] + (s_eta / (1 - s_eta)) * np.repeat(norm, 2)[None, :S] + np.zeros((L, 1))
