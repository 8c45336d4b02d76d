"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  A float64 model of the engine's normal draws, the a-priori bound of the device's fp32
result around it, and the schedule of which (counter, site code) every draw of a call sequence uses.  Checked
on the CPU by tests/test_noise_model.py; used by tests/test_gpu_noise_streams.py, tests/test_gpu_engine.py and tests/test_gpu_policy.py.

The stream (csrc/philox.h, csrc/kernels.h: philox_normal / philox_normal4): element e of the draw (ctr, code) comes from the Philox
block with counter words (ctr, 0, code, e >> 2) keyed by the seed; its four words v0..v3 give two Box-Muller pairs, (v0, v1) and
(v2, v3); u = philox_u01(v) in fp32; the even element of a pair is sqrt(-2 ln u1) cos(2 pi u2), the odd one ... sin(2 pi u2).
The model takes the Philox words from oracle/replay_ref.py (pinned by Random123's known-answer vectors), u1 and u2 as the exact fp32
values, and everything behind them in float64.

The bound: the device computes fl(rad trig) with rad = R* (1 + r), |r| <= rho = NOISE["rad_rel"], trig = T* + d, |d| <= delta =
NOISE["trig_rev_abs"] -- both measured exhaustively over the 2^24 values of philox_u01 on the device's own units
(profiles/libm_ulp.json) -- and one rounding of the product:
    |z - z*| <= R* delta (1 + rho) + |z*| (rho + 2^-24).
Nothing in it is observed on the engine.

This is not a test module, so pytest does not rewrite its asserts: every assert here carries its own message."""
import functools

import numpy as np

from oracle import replay_ref
from tests import bounds

CODE = {"critic": 0, "actor": 16, "alpha": 32, "predict": 48}
STREAM_POLICY = 0x400
# the noise buffers (include/sactd3.h: SACTD3_SITE_*) and the code each one's draws carry
SITE_CRITIC, SITE_ACTOR0, SITE_ACTOR1, SITE_ALPHA0, SITE_ALPHA1, SITE_PREDICT = range(6)
SITE_CODE = {SITE_CRITIC: 0, SITE_ACTOR0: 16, SITE_ACTOR1: 16, SITE_ALPHA0: 32, SITE_ALPHA1: 32, SITE_PREDICT: 48}
TRAIN_SITES = (SITE_CRITIC, SITE_ACTOR0, SITE_ACTOR1, SITE_ALPHA0, SITE_ALPHA1)
TWO_PI_F32 = np.float32(6.283185307179586)


def u01(x):
    """csrc/philox.h: philox_u01 in numpy float32 -- the add rounds to nearest even as on the device, so the top value is exactly 1"""
    return ((np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def pair_uniforms(seed, ctr, code, n):
    """(u1, u2, odd) of elements 0 .. n - 1 of the draw (ctr, code): fp32 uniforms of the element's Box-Muller pair, and whether it
    is the pair's sine"""
    e = np.arange(n, dtype=np.uint64)
    r = replay_ref.philox4x32_10(np.full(n, ctr & 0xFFFFFFFF), 0, code, e >> np.uint64(2), seed & 0xFFFFFFFF, seed >> 32)
    k = (e & np.uint64(3)).astype(np.int64)
    return u01(np.where(k < 2, r[0], r[2])), u01(np.where(k < 2, r[1], r[3])), (k & 1).astype(bool)


def bound(u1, u2, odd):
    """(z*, bound): the float64 normals of the pairs' fp32 uniforms and the a-priori per-element bound of the module docstring"""
    u1, u2 = bounds.f64(u1), bounds.f64(u2)
    R = np.sqrt(-2.0 * np.log(u1))
    z = R * np.where(odd, np.sin(2.0 * np.pi * u2), np.cos(2.0 * np.pi * u2))
    rho, delta = bounds.NOISE["rad_rel"], bounds.NOISE["trig_rev_abs"]
    return z, R * delta * (1.0 + rho) + np.abs(z) * (rho + bounds.U)


@functools.lru_cache(maxsize=256)
def _model(seed, ctr, code, n):
    z, b = bound(*pair_uniforms(seed, ctr, code, n))
    z.setflags(write=False)
    b.setflags(write=False)
    return z, b


def normals64(seed, ctr, code, n):
    """z* of elements 0 .. n - 1 of the draw (ctr, code) [n] float64, and, alongside, their bound"""
    return _model(int(seed), int(ctr), int(code), int(n))


def ratio(buf, seed, ctr, code):
    """worst |buf - z*| / bound over EVERY element of buf (any shape, element e = its flat index); NaN counts as infinitely far"""
    got = bounds.f64(buf).reshape(-1)
    z, b = normals64(seed, ctr, code, got.size)
    r = np.abs(got - z) / b
    return float(np.where(np.isnan(r), np.inf, r).max()) if got.size else 0.0


def label(buf, seed, code, ctr_range):
    """the counter in ctr_range whose model normals (at `code`) hold every element of buf inside the bound, or None"""
    hits = [c for c in ctr_range if ratio(buf, seed, c, code) <= 1.0]
    assert len(hits) <= 1, ("label", "more than one counter matches", code, hits)
    return hits[0] if hits else None


def describe(buf, seed, ctr_range, codes=(0, 16, 32, 48)):
    """for failure messages: which (ctr, code) a buffer is, among ctr_range x codes"""
    got = [(c, k) for k in codes for c in ctr_range if ratio(buf, seed, c, k) <= 1.0]
    if got:
        return " / ".join(f"(ctr {c}, code {k})" for c, k in got)
    flat = np.asarray(buf).reshape(-1)
    for k in codes:      # a buffer that is one draw in front and another (or nothing) behind
        for c in ctr_range:
            z, b = normals64(seed, c, k, flat.size)
            ok = np.abs(flat - z) <= b
            if ok[:4].all() and not ok.all():
                return f"(ctr {c}, code {k}) up to element {int(np.argmin(ok))}, something else behind"
    return "no draw of counters %d..%d" % (min(ctr_range), max(ctr_range))


def check(name, buf, seed, ctr, code, around=4):
    """every element of buf inside the bound of the draw (ctr, code) -> the worst |err| / bound; the failure names what the buffer is"""
    r = ratio(buf, seed, ctr, code)
    if not r <= 1.0:
        rng = range(max(0, ctr - around), ctr + around + 1)
        raise bounds.Violation(f"{name}: this buffer is {describe(buf, seed, rng)}, expected (ctr {ctr}, code {code}); worst |err| / bound {r:.3g}")
    return r


# ---------------------------------------------------------------------------------------------------- the fp32 emulation and its defects
def emulate32(seed, ctr, code, rows, a, defect=None, prev=None):
    """philox_normal4 / the tails' indexing in numpy float32 [rows, a], with one of the defects the checker has to refuse.  The
    hardware's trig units take the angle in revolutions, so their argument reduction is exact; the emulation reduces u2 by whole
    quarter revolutions (exact in fp32: u2 is a multiple of 2^-25) before it multiplies by 2 pi -- with the angle 2 pi_f32 u2 formed
    first (oracle/replay_ref.py: normals) the rounding of an angle near 2 pi alone, 2.4e-7 + 1.7e-7, is above the device's measured
    trig error, and that is the emulation's property, not the stream's."""
    n = rows * a
    row, j = np.divmod(np.arange(n), a)
    e = np.arange(n)
    if defect == "row_a4":
        e = row * (4 * ((a + 3) // 4)) + j
    if defect == "second_half":
        e = np.where(j >= 16, row * a + j - 16, e)
    if defect == "swap_codes":
        code = {16: 32, 32: 16}.get(code, code)
    if defect == "stuck_counter":
        ctr = 0
    m = int(e.max()) + 1
    r = replay_ref.philox4x32_10(np.full(m, ctr), 0, code, np.arange(m, dtype=np.uint64) >> np.uint64(2), seed & 0xFFFFFFFF, seed >> 32)
    k = np.arange(m) & 3
    if defect == "pairs_02_13":      # (v0, v2) and (v1, v3)
        w1, w2, odd = np.where(k < 2, r[0], r[1]), np.where(k < 2, r[2], r[3]), (k & 1).astype(bool)
    else:
        w1, w2, odd = np.where(k < 2, r[0], r[2]), np.where(k < 2, r[1], r[3]), (k & 1).astype(bool)
    if defect == "swap_sin_cos":
        odd = ~odd
    u1, u2 = u01(w1), u01(w2)
    rad = np.sqrt(np.float32(-2.0) * np.log(u1))
    q = np.floor(u2 * np.float32(4.0) + np.float32(0.5))                   # nearest quarter revolution, 0 .. 4
    t = TWO_PI_F32 * (u2 - q * np.float32(0.25))                            # |t| <= pi / 4
    s, c = np.sin(t), np.cos(t)
    qi = q.astype(np.int64) & 3
    sin_ = np.choose(qi, [s, c, -s, -c])
    cos_ = np.choose(qi, [c, -s, -c, s])
    z = (rad * np.where(odd, sin_, cos_)).astype(np.float32)[e]
    assert z.dtype == np.float32 and rad.dtype == np.float32 and t.dtype == np.float32, ("emulate32", "not computed in float32")
    if defect == "tail_zero":
        z[1024:] = 0.0
    if defect == "tail_stale":
        z[1024:] = np.asarray(prev, np.float32).reshape(-1)[1024:]
    return z.reshape(rows, a)


DEFECTS = ("swap_codes", "stuck_counter", "row_a4", "swap_sin_cos", "pairs_02_13", "tail_zero", "tail_stale", "second_half")


# ---------------------------------------------------------------------------------------------------- the schedule
class Schedule:
    """Which (counter, code) each draw of a call sequence uses, and which draw every noise buffer therefore holds (DESIGN.md section 4,
    derived from csrc/engine.hip: enqueue_opening_pair, enqueue_update_actor, enqueue_predict).

    noise_ctr starts at 0 and ticks once per critic update and once per actor update, whatever the algorithm and whether or not the
    update draws.  A critic update draws code 0 at the current value into the batch slot's critic buffer (SAC always, TD3 only with
    targ_actor_smoothing).  SAC's actor update j of an iteration draws code 16 into ACTOR0 / ACTOR1 (j even / odd) and, with autotune,
    code 32 into ALPHA0 / ALPHA1, both at the current value; TD3's draws nothing.  predict(explore=True) -- predict, predict_begin/_end,
    predict_device alike -- draws code 48 at predict_ctr into the predict buffer and ticks predict_ctr; a non-exploring call does
    neither.  Element e = row * ac_dim + j.

    `holds[site]` is the (counter, code) read_noise(site) shows, None while nothing was drawn there.  The run-ahead entry points
    consume exactly the draws of the iterations they stand for; what differs is what is left in ACTOR0 behind a whole PIPELINED period:
    its last actor update has already produced the opening pair of the next period, so ACTOR0 holds the next period's first policy
    draw, (counter behind the period + 1, 16).  The critic site reads the buffer of the batch slot the last iteration trained on."""

    def __init__(self, sac=True, autotune=True, smoothing=True, delay=2):
        self.sac, self.autotune, self.smoothing, self.delay = sac, autotune, smoothing, delay
        self.ctr = self.predict_ctr = 0
        self.holds = {s: None for s in SITE_CODE}
        self.drawn = []      # every (counter, code) used so far, in order: no pair may occur twice

    def _draw(self, site, ctr, code):
        assert (ctr, code) not in self.drawn, ("Schedule", "a (counter, code) pair is used by two draws", ctr, code)
        self.drawn.append((ctr, code))
        self.holds[site] = (ctr, code)

    def critic(self):
        if self.sac or self.smoothing:
            self._draw(SITE_CRITIC, self.ctr, CODE["critic"])
        self.ctr += 1

    def actor(self, j, api=False):
        """actor update j of an iteration; api: update_actor() called on its own, which has no place in an iteration and always
        draws into ACTOR0 / ALPHA0 (the counters and codes are those of the fused iteration)"""
        k = 0 if api else (j & 1)
        if self.sac:
            self._draw(SITE_ACTOR0 + k, self.ctr, CODE["actor"])
            if self.autotune:
                self._draw(SITE_ALPHA0 + k, self.ctr, CODE["alpha"])
        self.ctr += 1

    def iteration(self, do_actor, api=False):
        """step(do_actor) -- or, api: the call sequence update_qnets, update_actor x delay, update_targ_nets, and step_sampled in its
        prioritised, n-step and mixed draws, which is that sequence launch for launch (include/sactd3.h: ACTOR1 / ALPHA1 are the
        fused sactd3_step's only)"""
        self.critic()
        if do_actor:
            for j in range(self.delay):
                self.actor(j, api)

    def prefix(self, m):
        """step_prefix(m): the first m iterations of a period; nothing is produced ahead"""
        for i in range(m):
            self.iteration(i == 0)

    def period(self, pipelined):
        """step_period (and each period of step_periods): delay + 1 iterations.  pipelined: see the class docstring"""
        self.prefix(self.delay + 1)
        if pipelined and self.sac:
            self.holds[SITE_ACTOR0] = (self.ctr + 1, CODE["actor"])      # (drawn again, with the same values, if a single step follows)

    def predict(self, explore):
        if explore:
            self.holds[SITE_PREDICT] = (self.predict_ctr, CODE["predict"])
            self.predict_ctr += 1


# ---------------------------------------------------------------------------------------------------- the synthetic ring fill
def fill_model(seed, rows, o, a, min_ac, max_ac):
    """csrc/kernels.h: k_rb_fill in float64, rows 0 .. rows - 1: Philox (row, row >> 32, 0x200, chunk) keyed by the fill seed, one block
    per 16-byte chunk of the record [s | a | pad][s' | pad][reward, done, pad]; normals sqrtf(-2 logf(u)) cosf / sinf(t) with the fp32
    angle t = 2 pi_f32 u -- modelled as sqrt(-2 ln u) cos / sin(t) in float64 AT THAT fp32 t, bound as in the module docstring with the
    library's measured figures (NOISE["rad_libm_rel"], NOISE["cosf_abs"] / ["sinf_abs"]).
    -> {obs, nobs, rew: (value, bound); act: (lo, hi), the hull of the fused and the unfused fp32 form of min + (max - min) u;
        done: bool, exactly uni[1] < 0.01f decided from the integer word}"""
    ldc, ldo = 4 * ((o + a + 3) // 4), 4 * ((o + 3) // 4)
    cx, cn = ldc // 4, ldo // 4
    nch = cx + cn + 1
    row = np.repeat(np.arange(rows, dtype=np.uint64), nch)
    ch = np.tile(np.arange(nch, dtype=np.uint64), rows)
    r = replay_ref.philox4x32_10(row & np.uint64(0xFFFFFFFF), row >> np.uint64(32), replay_ref.STREAM_FILL, ch, seed & 0xFFFFFFFF, seed >> 32)
    words = np.stack(r, 1).reshape(rows, nch, 4)
    u = u01(words)                                                            # [rows, nch, 4] fp32
    u64 = bounds.f64(u)
    R = np.sqrt(-2.0 * np.log(u64[..., 0::2]))                                # [rows, nch, 2]: pairs (0, 1) and (2, 3)
    t = bounds.f64(TWO_PI_F32 * u[..., 1::2])
    nrm = np.stack([R[..., 0] * np.cos(t[..., 0]), R[..., 0] * np.sin(t[..., 0]), R[..., 1] * np.cos(t[..., 1]), R[..., 1] * np.sin(t[..., 1])], -1)
    rho = bounds.NOISE["rad_libm_rel"]
    dtr = np.stack([np.full(R[..., 0].shape, bounds.NOISE["cosf_abs"]), np.full(R[..., 0].shape, bounds.NOISE["sinf_abs"])] * 2, -1)
    Rr = np.repeat(R, 2, -1)
    nb = Rr * dtr * (1.0 + rho) + np.abs(nrm) * (rho + bounds.U)
    x, xb, uni = nrm[:, :cx].reshape(rows, -1), nb[:, :cx].reshape(rows, -1), u[:, :cx].reshape(rows, -1)
    xn, xnb = nrm[:, cx:cx + cn].reshape(rows, -1), nb[:, cx:cx + cn].reshape(rows, -1)
    lo32, hi32 = np.asarray(min_ac, np.float32), np.asarray(max_ac, np.float32)
    d = hi32 - lo32                                                           # fp32, as the kernel forms it
    ua = uni[:, o:o + a]
    unfused = (lo32 + d * ua).astype(np.float32)
    fused = (bounds.f64(lo32) + bounds.f64(d) * bounds.f64(ua)).astype(np.float32)      # (the product of two fp32 values is exact in float64)
    k = (words[:, cx + cn, 1] >> np.uint32(8)).astype(np.float64)
    done = (k + 0.5) < float(np.float32(0.01)) * 16777216.0                   # ((k + 0.5) 2^-24 is exact in fp32 for k < 2^23; above, far from 0.01)
    return {"obs": (x[:, :o], xb[:, :o]), "nobs": (xn[:, :o], xnb[:, :o]), "rew": (nrm[:, cx + cn, 0], nb[:, cx + cn, 0]),
            "act": (np.minimum(unfused, fused), np.maximum(unfused, fused)), "done": done, "uni_act": ua}
