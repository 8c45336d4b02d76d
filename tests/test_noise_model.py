"""The checker checked (CPU): tests/noise_model.py -- the float64 model of the engine's normal draws, its a-priori bound and its
schedule -- accepts an fp32 emulation of philox_normal4 and refuses every defect the GPU tests (tests/test_gpu_noise_streams.py) are
there to catch; the constants of the bound are tied to the exhaustive measurement they come from (profiles/libm_ulp.json)."""
import json
import math
import os

import numpy as np
import pytest

from oracle import replay_ref
from tests import bounds, noise_model as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x1234_5678_9ABC


def test_the_measured_record_lies_under_the_constants():
    """every constant is the measured figure rounded up to the next power of two: the figure is at most the constant and above half
    of it; the library functions' ulp figures (re-measured by the same run) stay under LIBM_ULP with the 1 ulp of the comparison"""
    rec = json.load(open(os.path.join(ROOT, "profiles", "libm_ulp.json")))
    nz = rec["noise"]
    assert nz["points"] == 1 << 24
    figures = {"rad_rel": nz["rad"]["max_rel"]["max"], "rad_libm_rel": nz["rad_libm"]["max_rel"]["max"],
               "trig_rev_abs": max(nz["sin_rev"]["max_abs"]["max"], nz["cos_rev"]["max_abs"]["max"]),
               "sinf_abs": nz["sinf"]["max_abs"]["max"], "cosf_abs": nz["cosf"]["max_abs"]["max"]}
    assert set(figures) == set(bounds.NOISE)
    for k, v in figures.items():
        c = bounds.NOISE[k]
        assert math.log2(c) == round(math.log2(c)) and 0.5 * c < v <= c, (k, v, c)
    for k in ("rad", "rad_libm"):
        assert nz[k]["exact_zero_at_one"] and nz[k]["nan"] == 0 and nz[k]["negative"] == 0, k
        assert nz[k]["largest_at_u"] == 2.0 ** -25 and abs(nz[k]["largest"] - math.sqrt(50.0 * math.log(2.0))) < 1e-6, k
    assert nz["u_max"] == 1.0 and nz["u_min"] == 2.0 ** -25
    assert nz["logf"]["max_ulp"] + 1.0 <= bounds.LIBM_ULP["logf"]
    for k, c in bounds.LIBM_ULP.items():
        assert rec["functions"][k]["max_ulp"] + 1.0 <= c, k


def test_model_words_are_the_stream_of_the_fp32_restatement():
    """normals64 and oracle/replay_ref.py: normals read the same Philox words in the same order: the fp32 restatement lies within
    1e-5 of the model everywhere (it forms the angle in fp32 radians, which costs it the bound near 2 pi: see emulate32)"""
    z, b = nm.normals64(77, 3, 16, 4099)
    assert np.abs(replay_ref.normals(77, 3, 16, 4099) - z).max() < 1e-5 and (b > 0).all() and b.max() < 4e-6
    assert nm.u01(np.uint32(0xFFFFFFFF)) == np.float32(1.0) and nm.u01(np.uint32(0)) == np.float32(2.0 ** -25)


def test_fp32_emulation_passes_the_bound_on_a_million_elements():
    rows, a = 62500, 16
    worst = 0.0
    for ctr, code in ((0, 0), (5, 16), (2 ** 31 + 1, 32), (9, 48)):
        worst = max(worst, nm.check(f"emulation ({ctr}, {code})", nm.emulate32(SEED, ctr, code, rows // 4, a), SEED, ctr, code))
    assert 0.0 < worst <= 1.0
    print("fp32 emulation: worst |err| / bound", worst)


# rows x a per defect: the smallest shape at which the defect shows
SHAPES = {"swap_codes": (17, 3), "stuck_counter": (17, 3), "row_a4": (17, 3), "swap_sin_cos": (17, 3), "pairs_02_13": (17, 3),
          "tail_zero": (61, 17), "tail_stale": (61, 17), "second_half": (61, 17)}


@pytest.mark.parametrize("defect", nm.DEFECTS)
def test_every_defect_is_refused(defect):
    rows, a = SHAPES[defect]
    ctr, code = 4, 16
    prev = nm.emulate32(SEED, ctr - 1, code, rows, a)
    good = nm.emulate32(SEED, ctr, code, rows, a)
    assert nm.check("sound", good, SEED, ctr, code) <= 1.0
    bad = nm.emulate32(SEED, ctr, code, rows, a, defect=defect, prev=prev)
    assert not np.array_equal(bad, good)
    with pytest.raises(bounds.Violation) as err:
        nm.check(defect, bad, SEED, ctr, code)
    msg = str(err.value)
    assert "expected (ctr 4, code 16)" in msg
    if defect == "stuck_counter":
        assert "this buffer is (ctr 0, code 16)" in msg
    if defect == "swap_codes":
        assert "this buffer is (ctr 4, code 32)" in msg
    if defect in ("tail_zero", "tail_stale"):
        assert "(ctr 4, code 16) up to element 1024" in msg
    assert nm.label(bad, SEED, code, range(16)) is None or defect == "stuck_counter"


def test_label_names_the_counter_among_sixteen_and_none_for_a_wrong_code():
    buf = nm.emulate32(SEED, 11, 32, 61, 17)
    assert nm.label(buf, SEED, 32, range(16)) == 11
    assert nm.label(buf, SEED, 16, range(16)) is None and nm.label(buf, SEED, 0, range(16)) is None
    assert nm.label(buf, SEED + 1, 32, range(16)) is None
    assert nm.label(buf[:1, :1], SEED, 32, range(11, 12)) == 11              # (one element: still a label of its own)


def test_codes_of_one_counter_are_pairwise_uncorrelated():
    """the model stream itself, 200 000 elements at one counter: the four site codes pairwise within 5 / sqrt(n); each one standard"""
    n = 200_000
    z = {k: nm.normals64(SEED, 7, k, n)[0] for k in (0, 16, 32, 48)}
    for k, v in z.items():
        assert abs(v.mean()) < 5.0 / math.sqrt(n) and abs(v.std() - 1.0) < 5.0 / math.sqrt(2 * n), k
    codes = sorted(z)
    for i, k in enumerate(codes):
        for m in codes[i + 1:]:
            assert abs(np.corrcoef(z[k], z[m])[0, 1]) < 5.0 / math.sqrt(n), (k, m)


def test_schedule_uses_no_pair_twice_and_matches_its_table():
    s = nm.Schedule(sac=True, autotune=True, delay=2)
    s.iteration(True)
    assert s.holds == {0: (0, 0), 1: (1, 16), 2: (2, 16), 3: (1, 32), 4: (2, 32), 5: None} and s.ctr == 3
    s.iteration(False)
    s.iteration(False)
    assert s.holds[0] == (4, 0) and s.ctr == 5
    s.period(pipelined=True)
    assert s.ctr == 10 and s.holds == {0: (9, 0), 1: (11, 16), 2: (7, 16), 3: (6, 32), 4: (7, 32), 5: None}
    s.iteration(True)                                                       # the single step behind draws where the schedule says
    assert s.holds[1] == (11, 16) and s.holds[0] == (10, 0)
    t = nm.Schedule(sac=False, smoothing=False, delay=2)
    t.iteration(True)
    t.predict(False)
    t.predict(True)
    assert t.ctr == 3 and t.predict_ctr == 1 and t.holds == {0: None, 1: None, 2: None, 3: None, 4: None, 5: (0, 48)}
    u = nm.Schedule(sac=True, autotune=False, delay=3)
    u.iteration(True)
    assert u.holds == {0: (0, 0), 1: (3, 16), 2: (2, 16), 3: None, 4: None, 5: None} and u.ctr == 4
    assert len(set(s.drawn)) == len(s.drawn)
    v = nm.Schedule(sac=True, autotune=True, delay=2)
    v.iteration(True, api=True)                                             # update_actor on its own: always ACTOR0 / ALPHA0
    assert v.holds == {0: (0, 0), 1: (2, 16), 2: None, 3: (2, 32), 4: None, 5: None} and v.ctr == 3 and v.drawn == s.drawn[:5]


def test_fill_model_done_rate_and_action_range():
    """10^5 rows of the synthetic fill's model: dones at 1 % within 5 sigma, actions inside [min, max] and filling it, unit normals"""
    n, o, a = 100_000, 3, 5
    lo, hi = [-1.0, -0.4, 0.0, -2.0, 0.5], [1.0, 0.4, 3.0, -1.0, 0.75]
    m = nm.fill_model(5, n, o, a, lo, hi)
    rate = m["done"].mean()
    assert abs(rate - 0.01) < 5.0 * math.sqrt(0.01 * 0.99 / n), rate
    alo, ahi = m["act"]
    assert (alo <= ahi).all() and (ahi - alo).max() <= 2.4e-7
    assert (alo >= np.float32(lo) - 1e-7).all() and (ahi <= np.float32(hi) + 1e-7).all()
    span = np.float32(hi) - np.float32(lo)
    assert ((ahi.max(0) - alo.min(0)) > 0.999 * span).all()
    for k in ("obs", "nobs"):
        v, b = m[k]
        assert v.shape == (n, o) and abs(v.mean()) < 5.0 / math.sqrt(n * o) and abs(v.std() - 1.0) < 0.01 and b.max() < 2e-6, k
    assert abs(np.corrcoef(m["obs"][0][:, 0], m["nobs"][0][:, 0])[0, 1]) < 5.0 / math.sqrt(n)
