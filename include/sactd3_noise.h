/*
 * sactd3_noise.h -- temporally correlated ("coloured") Gaussian exploration noise on the device: a generator of 1/f^beta sequences and
 * the collected rollout segment that explores with them (libsactd3_hip.so; include it beside sactd3.h).  The ABI version stays 1: four
 * functions are added, nothing that existed changes.
 *
 * Eberhard et al., "Pink Noise Is All You Need: Colored Noise Exploration in Deep Reinforcement Learning" (ICLR 2023): for SAC and TD3,
 * action noise with a 1/f spectrum (beta = 1) explores better than white (beta = 0) or red / Ornstein-Uhlenbeck-like (beta = 2) noise.
 *
 * The process.  A SEQUENCE q is one action component of one env, q = i ac_dim + j.  Noise comes in CHUNKS of L steps, L a power of two
 * in [64, 4096].  Chunk c of sequence q is a pure function of (engine seed, epoch, c, q, beta, L):
 *   normals     g_0 .. g_{L+1}: g_m is lane m & 3 of the Box-Muller pairs (csrc/philox.h: philox_box_muller4) over the Philox4x32-10 block
 *               with counter words
 *                   (c, q, 0xB00, (m >> 2) | (epoch << 16))
 *               keyed by the engine's seed (stream code 0xB00 is used by no other draw; epoch < 65536).  Frequency k has the real part
 *               g_{2k} and the imaginary part g_{2k+1}; the imaginary parts of k = 0 and k = L / 2 are drawn and not used.
 *   amplitudes  w_k = k^(-beta / 2) (k >= 1); v_0 = sqrt(2) w_1 (the DC bin takes the weight of the lowest frequency, as in the
 *               `colorednoise` package the paper used), v_k = 2 w_k (0 < k < L / 2), v_{L/2} = sqrt(2) w_{L/2}; a_k = v_k / sqrt(sum v^2).
 *   signal      x[t] = a_0 g_0 + sum_{k=1}^{L/2-1} a_k (g_{2k} cos(2 pi k t / L) - g_{2k+1} sin(2 pi k t / L)) + a_{L/2} g_L (-1)^t.
 * sum a^2 = 1, so every x[t] is N(0, 1); beta = 0 is white, 1 pink, 2 red.  Successive chunks are independent, as in the paper's
 * implementation, which redraws a sequence when it is used up.  The host computes a_k and the twiddles in float64 and rounds them once
 * to fp32; the device evaluates the sum as one inverse FFT per pair of sequences (csrc/noise_kernels.h) and calls no powf, sinf or cosf.
 *
 * Position and epoch of a rollout's process are run-time state: they are not part of a checkpoint, and a restored run explores with
 * the noise of a fresh sactd3_rollout_noise_configure.
 */
#ifndef SACTD3_NOISE_H
#define SACTD3_NOISE_H

#include "sactd3.h"
#include "sactd3_rollout.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The stand-alone generator: chunk `chunk` of sequences 0 .. sequences - 1 at `epoch`, element (t, q) at out[t * out_ld + q], fp32, into
 * the caller's device memory; columns at and behind `sequences` are not written.  One launch on the learner stream; flags:
 * SACTD3_SRC_ORDERED | SACTD3_DST_ORDERED against caller_stream, as sactd3_dormant_scan_device orders its call.  Invisible to training
 * and acting: no counter moves.  The tables of a (beta, length) pair are made at its first use and kept until sactd3_destroy; nothing
 * is allocated after that.  A pair is looked up by the float value of beta, 32 pairs an engine and none is ever given up: a sweep over
 * more values of beta on one engine is refused at the 33rd (SACTD3_ESTATE) -- use an engine per run, or few values.
 * Refusals, all in front of any side effect:
 *   SACTD3_EINVAL  a NULL handle or `out`; `out` not memory of the engine's device; `length` not a power of two in [64, 4096];
 *                  sequences < 1; beta outside [0, 2] or NaN; epoch >= 65536; out_ld < sequences; an unknown flag
 *   SACTD3_ESTATE  a 33rd (beta, length) pair */
int sactd3_colored_noise_device(sactd3_engine* e, float beta, int length, int sequences, uint32_t chunk, uint32_t epoch, float* out,
                                int64_t out_ld, void* caller_stream, int flags);

/* Give the rollout a process: S = num_envs * ac_dim sequences of chunks of `length` steps at `beta`, a two-chunk slab [2][length][S] of
 * its own, the 64-bit position pos = 0, and an epoch that goes up by one with every such call (the first is 1), so that configuring
 * again yields fresh noise.  length = 0 removes the process (beta is not looked at).  The slab is the handle's own allocation, made by
 * this call, never by a collect: it is kept when the process is removed and replaced (hipMalloc, then hipFree, which waits for the device)
 * only by a configure call that needs a larger one; it goes with sactd3_rollout_destroy.  SACTD3_EINVAL: a NULL handle, beta / length as
 * above; SACTD3_ESTATE: the 65536th process of a handle. */
int sactd3_rollout_noise_configure(sactd3_rollout* r, float beta, int length);
/* sactd3_rollout_collect in SACTD3_ROLLOUT_EXPLORE mode with e taken from the process in place of the white draw: step t of the call is
 * global step p = pos + t and reads row p % length of slab slot (p / length) & 1.  In front of the collect launch, on the learner stream,
 * the generator runs for every chunk in [pos / length, (pos + steps - 1) / length] that is not yet in its slot -- two at the most; behind
 * the call pos += steps.  The actions follow the white kernel's arithmetic exactly: SAC tanh(mean + e std) scale + bias, TD3 tanh(u)
 * scale + bias + e (scale actor_noise_std).  Nothing is drawn from stream 0x900 and collect_ctr does not move; `eps`, if given,
 * receives the values used.  Refusals: every one of sactd3_rollout_collect, and
 *   SACTD3_EINVAL  steps > length
 *   SACTD3_ESTATE  the rollout has no process */
int sactd3_rollout_collect_colored(sactd3_rollout* r, int steps, float* records, float* eps);
/* out = {configured length (0: no process), pos, chunks generated, epoch} */
int sactd3_rollout_noise_stats(const sactd3_rollout* r, int64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* SACTD3_NOISE_H */
