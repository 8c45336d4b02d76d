"""CPU: tests/colored_noise_model.py against the definition of include/sactd3_noise.h written out as the O(L^2) sum, and the unit
variance the normalisation promises."""
import numpy as np
import pytest

from tests import colored_noise_model as M

L, SEED = 64, 11


def test_beta_zero_is_the_direct_cosine_and_sine_sum():
    a = M.amplitudes(0.0, L)
    g, _ = M.normals(SEED, 2, 3, 5, L)
    t, k = np.arange(L)[:, None], np.arange(1, L // 2)[None, :]
    th = 2.0 * np.pi * k * t / L
    want = a[0] * g[0] + (a[k] * (g[2 * k] * np.cos(th) - g[2 * k + 1] * np.sin(th))).sum(1) + a[L // 2] * g[L] * (-1.0) ** np.arange(L)
    assert np.abs(M.sequence(a, g) - want).max() <= 1e-12
    assert np.allclose(a[1:-1], a[1]) and np.isclose(a[0] * np.sqrt(2.0), a[1], rtol=1e-6)      # white: a flat spectrum


@pytest.mark.parametrize("beta", [0.0, 1.0, 2.0])
def test_amplitudes_are_normalised_and_the_samples_have_unit_variance(beta):
    k = np.arange(1, L // 2 + 1, dtype=np.float64)
    v = np.concatenate([[np.sqrt(2.0)], 2.0 * k ** (-0.5 * beta)])
    v[-1] /= np.sqrt(2.0)
    exact = v / np.sqrt((v * v).sum())                          # before the rounding to fp32
    assert abs((exact ** 2).sum() - 1.0) <= 1e-15 and np.abs(M.amplitudes(beta, L) - exact).max() <= 2.0 ** -24
    x, _ = M.chunk(SEED, beta, L, 4096)
    m = (x ** 2).mean(0)                                        # one figure per sequence: the samples inside one are correlated
    se = m.std(ddof=1) / np.sqrt(m.size)
    assert abs(m.mean() - 1.0) <= 5.0 * se, (beta, m.mean(), se)
