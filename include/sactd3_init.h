/*
 * sactd3_init.h -- initialise and reset an engine's networks on the device (libsactd3_hip.so; include it beside sactd3.h).  The ABI
 * version stays 1: two functions are added, nothing that existed changes.
 *
 * sactd3_create leaves every weight at zero.  sactd3_init_params gives the chosen networks the reference's initial state
 * (agents/nets.py:35-47: torch.nn.init.orthogonal_ at gain 1 on every weight matrix, biases 0, LayerNorm weights 1, LayerNorm biases
 * 0) without torch, without LAPACK and without a host copy: a C host has a trainable engine from this call alone, and the initial
 * parameters are, as every other piece of the engine's state, a pure function of a Philox key.  The same call, at a later epoch, is the
 * periodic reset of high update-to-data training (Nikishin et al. 2022; D'Oro et al. 2023): the networks start over, the replay ring
 * stays.
 *
 * The draw.  A weight [rows, cols] is made from a Gaussian matrix G [max(rows, cols), min(rows, cols)].  Element (i, j) of the G of
 * matrix `id` in epoch E is lane e & 3, e = i * min(rows, cols) + j, of the Box-Muller pairs (csrc/philox.h: philox_box_muller4, the
 * function of every normal the engine draws) over the Philox4x32-10 block with counter words
 *     (E, id | attempt << 16, 0x700, e >> 2)
 * keyed by `seed`; attempt is 0 (see below).  Stream code 0x700 is used by no other draw.  Matrix ids: actor layers 0, 1, 2 (layer 1,
 * layer 2, head); critic net n (0, 1), layer l: 3 + 3 n + l.  The value is a pure function of (seed, id, i, j, E): initialising a
 * subset of the nets gives them the bits that initialising all of them gives.  This is not torch's stream, and the reference's
 * discarded actor_detach draw has no counterpart.
 *
 * The orthogonalisation.  G's columns are orthonormalised in fp32 by classical Gram-Schmidt applied twice, with one summation order,
 * one workgroup per matrix, every matrix of a call in one launch; the diagonal of the R factor is a column's norm, hence positive, which
 * is torch's sign convention.  W = Q for rows >= cols, else Q^T.  A column whose norm behind the projections is zero or not finite is
 * never divided by it: it is drawn again with attempt + 1 and counted (sactd3_init_stats); behind 8 redraws it is left zero.  The bits
 * depend on nothing but (seed, epoch) and the engine's dimensions -- not on batch_size, max_envs, use_graphs or the other matrices.
 *
 * The fan-out.  For the chosen networks: the targets (TD3's run-ahead target actors too) become a bit copy of the online networks;
 * Adam's exp_avg / exp_avg_sq become 0, the optimiser's step count 0 and its running beta powers {1, 1}; with SACTD3_INIT_ALPHA
 * log_alpha becomes logf(alpha_init) and its two moments 0.  Nothing else in device memory is written: not the ring, not the priority
 * table, no counter, no noise buffer, not the batch slot.
 *
 * Host state.  The call is enqueued on the engine's stream and returns at once: it does not wait and does not copy.  It breaks the
 * run-ahead chain of sactd3_step_period as sactd3_set_params does, marks the gradient arenas of the chosen networks as not held
 * (sactd3_debug_read refuses them until an update rewrites them), and leaves every captured graph valid: no arena moves.  The scratch
 * buffer for G is made at the first call; an engine that never calls holds nothing more than before.
 */
#ifndef SACTD3_INIT_H
#define SACTD3_INIT_H

#include "sactd3.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SACTD3_INIT_ACTOR = 1, SACTD3_INIT_CRITICS = 2, SACTD3_INIT_ALPHA = 4 };

/* Initialise the networks `what` names (a sum of SACTD3_INIT_*) at (seed, epoch).  Refusals, all in front of any side effect:
 *   SACTD3_EINVAL  a NULL handle; what == 0; unknown bits in `what`; SACTD3_INIT_ALPHA on a TD3 engine (it has no temperature);
 *                  ob_dim + ac_dim above 8192 (a column of G has to fit one workgroup's LDS)
 *   SACTD3_ESTATE  an acting call is in flight (sactd3_predict_begin without its end) */
int sactd3_init_params(sactd3_engine* e, uint32_t what, uint64_t seed, uint32_t epoch);
/* out = {calls accepted, weight matrices of the last call, columns redrawn so far, 0}.  The third is a device word: [sync]. */
int sactd3_init_stats(sactd3_engine* e, int64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* SACTD3_INIT_H */
