"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

numpy restatement of hindsight relabelling at staging (include/sactd3.h: sactd3_rb_sample_hindsight*; csrc/hindsight_kernels.h), over
host copies of the ring's fields indexed by ring SLOT (obs [cap, o], act [cap, a], nobs [cap, o], rew [cap], done [cap] as float32):

* age(i) = i while length < cap, else (i - cursor) mod cap; slot_j = (i0 + j * stride) mod cap exists iff age(i0) + j * stride < length.
* link j -> j+1 holds iff slot_{j+1} exists, done[slot_j] == 0 and nobs[slot_j] equals obs[slot_{j+1}] as 32-bit patterns.
* L = 1 + the number of leading links that hold among links 0 .. window-2.
* draw: Philox (oracle.replay_ref) counter words (hctr, 0, 0x600, b) keyed by the seed; relabelled iff u01(v0) < ratio, j = (v1 * L) >> 32;
  with `choice`: choice[b] < 0 not relabelled, else j = min(choice[b], L - 1).
* goal = nobs[slot_j][achieved : achieved + dim] as bits; X = [s | a] and Xn = s' of slot_0 with floats [desired, desired + dim) replaced;
  rew = 0 if acc <= thr * thr else -1, acc = sum over c in index order of (ag'_c - g_c) * (ag'_c - g_c), ag' from slot_0's own s', every
  operation a float32 one; done = the stored flag.  Not relabelled: the record's bits.  A start slot outside [0, length): zeros, -1.

`stage(..., defect=...)` is the same with one rule broken (DEFECTS), for the tests that check the checker; `synthetic_ring` makes
episodic records of any shape whose episode bookkeeping is known."""
from __future__ import annotations

import numpy as np

from oracle import replay_ref

F = np.float32
STREAM_HINDSIGHT = 0x600
MAX_WINDOW, MAX_GOAL = 64, 8
DEFECTS = ("goal_from_s", "crosses_truncation", "crosses_newest", "j_over_window", "xn_not_relabelled", "reward_from_s", "lt_at_threshold",
           "pad_touched", "done_recomputed")


class Mismatch(AssertionError):
    pass


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def u01(x):
    return ((np.asarray(x, np.uint32) >> np.uint32(8)).astype(F) + F(0.5)) * F(1.0 / 16777216.0)


def draws(seed: int, hctr: int, B: int):
    """-> (u [B] float32 in (0, 1), v1 [B] uint32): words 0 and 1 of Philox (hctr, 0, 0x600, b)"""
    b = np.arange(B, dtype=np.uint64)
    r = replay_ref.philox4x32_10(np.full(B, hctr, np.uint64), np.zeros(B, np.uint64), np.full(B, STREAM_HINDSIGHT, np.uint64), b,
                                 int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    return u01(r[0]), np.asarray(r[1], np.uint32)


def age(i: int, length: int, cursor: int, cap: int) -> int:
    return i if length < cap else (i - cursor) % cap


def chain_slots(fields, i0, window, stride, length, cursor, cap, defect=None):
    """the ring slots slot_0 .. slot_{L-1} of the row that starts at i0 (accepted: 0 <= i0 < length)"""
    obs, nobs, done = fields["obs"], fields["nobs"], fields["done"]
    a0 = age(i0, length, cursor, cap)
    slots = [i0]
    for j in range(1, window):
        if a0 + j * stride >= length and defect != "crosses_newest":
            break
        nxt = (i0 + j * stride) % cap
        cur = slots[-1]
        if done[cur] != 0:
            break
        if defect != "crosses_truncation" and not np.array_equal(bits(nobs[cur]), bits(obs[nxt])):
            break
        slots.append(nxt)
    return slots


def goal_reward(achieved, goal, thr, lt=False):
    acc = None
    for c in range(len(goal)):
        d = F(F(achieved[c]) - F(goal[c]))
        sq = F(d * d)
        acc = sq if acc is None else F(acc + sq)
    thr2 = F(F(thr) * F(thr))
    on = acc < thr2 if lt else acc <= thr2
    return F(0.0) if on else F(-1.0)


def stage(fields, geom, idx, cfg, seed=0, hctr=0, choice=None, defect=None):
    """fields: dict obs, act, nobs, rew, done by ring slot; geom: dict(length, cursor, cap); cfg: dict(achieved, desired, dim,
    threshold, ratio, window, stride); idx [B] start slots; choice [B] int or None (the native draw at (seed, hctr)).
    -> dict X [B, 4 cx], Xn [B, 4 cn] (the slot's padded rows), obs, act, nobs (their fields), rew, done [B] float32, slot_idx, offset,
    goal_slot, L [B] int32 (L: 0 for a refused row)"""
    assert defect is None or defect in DEFECTS, defect
    o, a = fields["obs"].shape[1], fields["act"].shape[1]
    length, cursor, cap = (int(geom[k]) for k in ("length", "cursor", "cap"))
    ag, dg, G = int(cfg["achieved"]), int(cfg["desired"]), int(cfg["dim"])
    window, stride, ratio, thr = int(cfg["window"]), int(cfg["stride"]), F(cfg["ratio"]), F(cfg["threshold"])
    assert 1 <= G <= MAX_GOAL and 1 <= window <= MAX_WINDOW and stride >= 1 and ag + G <= o and dg + G <= o
    idx = np.asarray(idx).reshape(-1)
    B = len(idx)
    u, v1 = draws(seed, hctr, B)
    cx4, cn4 = -(-(o + a) // 4) * 4, -(-o // 4) * 4
    X, Xn = np.zeros((B, cx4), F), np.zeros((B, cn4), F)
    rew, done = np.zeros(B, F), np.zeros(B, F)
    slot_idx, offset, goal_slot, Ls = (np.full(B, -1, np.int32) for _ in range(4))
    Ls[:] = 0
    for b in range(B):
        i0 = int(idx[b])
        if not 0 <= i0 < length:
            continue
        slots = chain_slots(fields, i0, window, stride, length, cursor, cap, defect)
        L = len(slots)
        Ls[b], slot_idx[b] = L, i0
        X[b, :o], X[b, o:o + a], Xn[b, :o] = fields["obs"][i0], fields["act"][i0], fields["nobs"][i0]
        rew[b], done[b] = fields["rew"][i0], fields["done"][i0]
        if choice is None:
            relabel = bool(u[b] < ratio)
            j = (int(v1[b]) * (window if defect == "j_over_window" else L)) >> 32
            if defect == "j_over_window":
                j = min(j, L - 1)
        else:
            relabel = int(choice[b]) >= 0
            j = min(int(choice[b]), L - 1)
        if not relabel:
            continue
        gs = slots[j]
        src = fields["obs"] if defect == "goal_from_s" else fields["nobs"]
        g = src[gs][ag:ag + G].copy()
        offset[b], goal_slot[b] = j, gs
        X[b, dg:dg + G] = g
        if defect != "xn_not_relabelled":
            Xn[b, dg:dg + G] = g
        if defect == "pad_touched" and dg + G < cn4:
            Xn[b, dg + G] = g[-1]
        achieved = (fields["obs"] if defect == "reward_from_s" else fields["nobs"])[i0][ag:ag + G]
        rew[b] = goal_reward(achieved, g, thr, lt=defect == "lt_at_threshold")
        if defect == "done_recomputed" and rew[b] == 0:
            done[b] = F(1.0)
    return dict(X=X, Xn=Xn, obs=X[:, :o].copy(), act=X[:, o:o + a].copy(), nobs=Xn[:, :o].copy(), rew=rew, done=done, slot_idx=slot_idx,
                offset=offset, goal_slot=goal_slot, L=Ls)


KEYS = ("obs", "act", "nobs", "rew", "done", "slot_idx", "offset", "goal_slot")


def check(want, got, keys=KEYS):
    """every array of `got` named in `keys` against the reference's, bit for bit; Mismatch names the first rows that differ"""
    for k in keys:
        w, g = np.ascontiguousarray(want[k]), np.ascontiguousarray(np.asarray(got[k]).reshape(want[k].shape)).astype(want[k].dtype, copy=False)
        if w.tobytes() != g.tobytes():
            wv, gv = w.view(np.uint32 if w.dtype == F else w.dtype), g.view(np.uint32 if g.dtype == F else g.dtype)
            rows = np.flatnonzero((wv.reshape(len(w), -1) != gv.reshape(len(g), -1)).any(1))
            raise Mismatch(f"{k}: {len(rows)} of {len(w)} rows differ (rows {list(rows[:8])}): got {g[rows[0]]!r} want {w[rows[0]]!r}")


# ---------------------------------------------------------------------------------------------------- rings
def place(rows, cap):
    """rows in append order (dict obs, act, nobs, rew, done [n, ...]) -> (the same fields by ring slot [cap, ...], unfilled slots zero;
    dict(length, cursor, cap); row [cap]: the append-order row each slot holds, -1 where none): row r lands in slot r % cap"""
    n = len(rows["rew"])
    out = {k: np.zeros((cap,) + np.asarray(v).shape[1:], F) for k, v in rows.items()}
    held = np.full(cap, -1, np.int64)
    lo = max(0, n - cap)
    at = np.arange(lo, n)
    for k, v in rows.items():
        out[k][at % cap] = np.asarray(v, F)[lo:n]
    held[at % cap] = at
    return out, dict(length=min(n, cap), cursor=n % cap, cap=cap), held


def synthetic_ring(o, a, n_envs, steps, horizon, seed, term_every=0, achieved=0, dim=1):
    """Episodic records of any shape, `steps` vector steps of `n_envs` envs in append order (row t * n_envs + e): within an episode
    s'_t IS s_{t+1} bit for bit; env e's episodes end every `horizon` steps (shifted by e), by truncation (done 0, the next episode
    starts elsewhere) or, every `term_every`-th of them, by termination (done 1).  The achieved goal moves in steps of 0.03 so that a
    goal a few steps ahead lies on either side of a threshold of 0.1.  -> (rows dict, episode [n] int: a global episode id per row)"""
    rng = np.random.default_rng(seed)
    n = steps * n_envs
    obs, nobs = np.zeros((n, o), F), np.zeros((n, o), F)
    act = rng.uniform(-1, 1, (n, a)).astype(F)
    rew, done, episode = -np.ones(n, F), np.zeros(n, F), np.zeros(n, np.int64)
    cur = rng.standard_normal((n_envs, o)).astype(F)
    ep = np.arange(n_envs)
    count = np.zeros(n_envs, np.int64)
    for t in range(steps):
        r = t * n_envs + np.arange(n_envs)
        nxt = (cur + rng.standard_normal((n_envs, o)).astype(F) * F(0.01)).astype(F)
        nxt[:, achieved:achieved + dim] = cur[:, achieved:achieved + dim] + F(0.03) * rng.choice([-1.0, 1.0], (n_envs, dim)).astype(F)
        obs[r], nobs[r], episode[r] = cur, nxt, ep
        ends = (t + 1 + np.arange(n_envs)) % horizon == 0
        count += ends
        term = ends & (count % term_every == 0) if term_every else np.zeros(n_envs, bool)
        done[r] = term.astype(F)
        fresh = rng.standard_normal((n_envs, o)).astype(F)
        cur = np.where(ends[:, None], fresh, nxt).astype(F)
        ep = np.where(ends, ep + n_envs, ep)
    return dict(obs=obs, act=act, nobs=nobs, rew=rew, done=done), episode


def host_rollout(env, steps, scale=1.0):
    """`steps` vector steps of a gymnasium-protocol host env (reset by the caller's seed; random actions of its own action space, times
    `scale`) as ring rows in append order, with the loop's stored-next rule: the arrival observation where the step was truncated.
    -> (rows dict, episode [n] int: env index + num_envs * the env's episode count)"""
    n = env.num_envs
    obs, _ = env.reset(seed=env.seed)
    out = {k: [] for k in ("obs", "act", "nobs", "rew", "done")}
    episode, count = [], np.zeros(n, np.int64)
    for _ in range(steps):
        act = (env.action_space.sample() * F(scale)).astype(F)
        nxt, rew, term, trunc, infos = env.step(act)
        stored = nxt.copy()
        for k in np.flatnonzero(trunc):
            stored[k] = infos["final_observation"][k]
        for k, v in (("obs", obs), ("act", act), ("nobs", stored), ("rew", rew), ("done", term.astype(F))):
            out[k].append(np.asarray(v, F).copy())
        episode.append(np.arange(n) + n * count)
        count = count + (term | trunc)
        obs = nxt
    return {k: np.concatenate(v) for k, v in out.items()}, np.concatenate(episode)


def true_lengths(episode, done, held, geom, idx, window, stride):
    """L from episode bookkeeping alone: rows of the same episode that follow the start row at `stride` in the ring, up to the newest
    row, a termination or `window`"""
    n_rows = int(held.max()) + 1
    out = []
    for i0 in np.asarray(idx).reshape(-1):
        r = int(held[int(i0)])
        L = 1
        while L < window and r + stride < n_rows and episode[r + stride] == episode[r] and done[r] == 0:
            r += stride
            L += 1
        out.append(L)
    return np.array(out, np.int32)
