/*
 * sactd3_feature_rank.h -- the feature rank of an engine's networks over ring rows, on the device: the spectrum of the Gram matrix of the
 * last hidden layer (libsactd3_hip.so; include it beside sactd3.h and sactd3_dormant.h).  The ABI version stays 1: two functions are
 * added, nothing that existed changes.
 *
 * Kumar et al., "Implicit under-parameterization" (ICLR 2021): the effective rank srank_delta of the penultimate features; Lyle et al.,
 * "Understanding and preventing capacity loss" (ICLR 2022): the feature rank, the number of singular values above a threshold; Roy &
 * Vetterli (2007): the entropy-based effective rank.  The dormant ratio (sactd3_dormant.h) counts dead units; it does not see 256 live
 * units that all encode the same three directions.
 *
 * For one net and the V valid rows of the call let Phi (V x 256) be the output of its second hidden layer,
 * relu(LN(W2 relu(LN(W1 x + b1)) + b2)), LN the identity with layer_norm == 0, two-pass, eps inside the root; online parameters only;
 * the critics read a record's leading [s | a], the actor its leading s.  Then
 *     M = Phi^T Phi / V                       256 x 256, symmetric
 *     lambda_1 >= ... >= lambda_256           its eigenvalues, negative computed values clamped to 0
 *     sigma_i = sqrt(lambda_i) where lambda_i > floor * lambda_1, else 0        the singular values of Phi / sqrt(V)
 *     trace      = sum_i M_ii, summed from the Gram matrix before the solver runs
 *     lambda_sum = sum_i lambda_i, summed behind it: the pair is a built-in invariant
 *     rank       = #{sigma_i > 0}
 *     srank      = min{k : sum_{i <= k} sigma_i >= (1 - delta) sum_i sigma_i}
 *     erank      = exp(-sum_i p_i ln p_i), p = sigma / sum sigma over sigma_i > 0
 *     stable     = lambda_sum / lambda_1
 * V == 0 or lambda_1 == 0 gives zeros throughout.  `floor` is the caller's, in [1e-6, 1): a Gram matrix in fp32 cannot resolve a
 * singular value below about sqrt(256 u) sigma_1 (u = 2^-24: about 4e-3 sigma_1, 1.5e-5 lambda_1) -- forming Phi^T Phi squares the
 * condition number; a float64 SVD of Phi itself would see smaller ones.  The eigenvalues come from a parallel cyclic Jacobi solver in one
 * workgroup's LDS: `sweeps` (at most 16) and `converged` (1: a whole sweep without a rotation) are part of the summary; with
 * converged == 0 the spectrum is that of the last sweep, and the caller decides what it is worth.  The solver leaves an off-diagonal
 * element alone once it is at or below 2^-30 of the trace; up to 255 such couplings can add about 2.4e-7 trace to a small eigenvalue,
 * so with a floor below about 1e-5 (and a trace well above lambda_1) `rank` counts solver noise as well as the Gram matrix's own.
 *
 * `idx`, `idx_ld`, `flags` and the stream ordering mean what they mean in sactd3_dormant_scan_device: a slot outside [0, rb_len) never
 * becomes an address, its row contributes nothing and is counted.  Nets are ordered actor, Q1, Q2; rows of nets `what` does not name are
 * not written.  The three launches are eager, on the learner stream, behind every update issued before; no copy, no host wait.  The call
 * is invisible to training and acting exactly as a dormant scan is (no counter, noise buffer, batch slot or acting scratch is touched, a
 * precomputed opening pair of sactd3_step_period stays valid, allowed while sactd3_predict_begin is in flight), and invisible to the
 * dormant scan: it has device memory of its own, made at its first call, so sactd3_dormant_stats and a pending sactd3_redo mask read the
 * same behind it as before.  The same call on the same state gives the same bits (fixed orders, no atomics).
 */
#ifndef SACTD3_FEATURE_RANK_H
#define SACTD3_FEATURE_RANK_H

#include "sactd3.h"
#include "sactd3_dormant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The spectrum of the nets `what` names (a sum of SACTD3_DORMANT_ACTOR, SACTD3_DORMANT_CRITICS) over the n rows idx[r * idx_ld].
 * spectrum: NULL, or a contiguous device [3][256] (lambda, descending); gram: NULL, or a contiguous device [3][256][256] (M, symmetric
 * by construction).  Refusals, all in front of any side effect:
 *   SACTD3_EINVAL  a NULL handle or idx; n < 1 or n > 4096; idx_ld < 1; `what` empty or with unknown bits; delta outside (0, 1) or floor
 *                  outside [1e-6, 1) or either not finite; a pointer not on the engine's device; an unknown flag
 *   SACTD3_ESTATE  the ring is empty */
int sactd3_feature_rank_device(sactd3_engine* e, const int64_t* idx, int64_t idx_ld, int n, uint32_t what, float delta, float floor,
                               float* spectrum, float* gram, void* caller_stream, int flags);
/* counters = {calls, valid rows of the last call, rows refused so far, rank of actor / Q1 / Q2 at their last call, srank of the three,
 * sweeps of the three, solver runs that did not converge so far, 0 ...}; summary[net] = {trace, lambda_sum, rank, srank, erank, stable,
 * sweeps, converged} of that net's last call.  Device memory: [sync]. */
int sactd3_feature_rank_stats(sactd3_engine* e, int64_t counters[16], float summary[3][8]);

#ifdef __cplusplus
}
#endif
#endif /* SACTD3_FEATURE_RANK_H */
