/*
 * sactd3_dormant.h -- the dormant-neuron ratio of an engine's networks over ring rows, and ReDo recycling of the neurons it finds, on the
 * device (libsactd3_hip.so; include it beside sactd3.h).  The ABI version stays 1: three functions are added, nothing that existed changes.
 *
 * Sokar et al., "The Dormant Neuron Phenomenon in Deep RL" (ICML 2023).  For a hidden layer with activations h = relu(LN(W x + b))
 * (LN the identity with layer_norm == 0; two-pass, eps inside the root), over V ring rows:
 *     m_i = (1 / V) sum_rows h_i,        s_i = m_i / ((1 / 256) sum_k m_k)        (their eq. 1),        neuron i is dormant iff s_i <= tau.
 * Where the layer mean is 0 every score is 0; with V == 0 every score is 0 and nothing is marked dormant.
 *
 * The scan.  `idx` is a device int64 array of ring slots, with the meaning and the checking of sactd3_rb_read_rows_device: a slot
 * outside [0, rb_len) never becomes an address, its row contributes nothing and is counted.  The kernel reads the packed ring records
 * where they are: the critics' input is a record's leading [s | a], the actor's its leading s.  There is no pack kernel and no batch slot.
 * Six (net, layer) pairs, net-major: actor L1, actor L2, Q1 L1, Q1 L2, Q2 L1, Q2 L2; online parameters only.  The launches are eager, on
 * the learner stream, behind every update issued before; no copy, no host wait.  A scan is invisible to training and acting: no counter,
 * noise buffer, batch slot or acting scratch is touched, a precomputed opening pair of sactd3_step_period stays valid, and it is allowed
 * while sactd3_predict_begin is in flight.  The same call on the same state gives the same bits (fixed summation orders, no atomics).
 * It leaves, in device memory of its own (made at the first scan), the scores [6][256], the masks [6][256] and the per-pair counts.
 *
 * sactd3_redo recycles the neurons the last scan marked in the nets of `what`.  For a dormant neuron i of layer l: row i of the incoming
 * weight becomes g (c / |g|), where g_j is lane e & 3, e = i K + j, of the Box-Muller pairs (csrc/philox.h: philox_box_muller4) over the
 * Philox4x32-10 block with counter words
 *     (epoch, matrix id, 0xA00, e >> 2)
 * keyed by `seed` (matrix ids as in sactd3_init.h; stream code 0xA00 is used by no other draw), c = sqrtf(min(1, K / 256)) is the RMS
 * row norm of the orthogonal initialiser, and |g| is summed in fp32 in one fixed order; a norm that is zero or not finite leaves the row
 * zero and is counted.  The neuron's bias becomes 0, its LayerNorm weight 1, its LayerNorm bias 0; column i of the outgoing weight
 * (W2[:, i] for l = 1, every head row's element i for l = 2) becomes 0; where an element is both incoming of a recycled layer-2 neuron and
 * outgoing of a recycled layer-1 neuron, the zero wins.  Adam's exp_avg / exp_avg_sq become 0 at exactly the written elements.  Not
 * touched: the targets (TD3's run-ahead target actors too), step counts, beta powers, log_alpha, the ring -- the targets follow by
 * Polyak averaging, as in the paper.  Host state: as sactd3_init_params, the call breaks the run-ahead chain, orders itself against
 * acting for the actor, marks the chosen nets' gradient arenas stale and drops no graph.  A mask is good for one redo.
 *
 * Caveat.  With layer_norm = 1 a recycled neuron changes its layer's LayerNorm statistics: its pre-activation enters the mean and the
 * variance of every row.  The paper's "the network's output is unchanged by recycling" holds for layer_norm = 0 only.
 * sactd3_set_params between a scan and a redo is not tracked: the masks then describe the parameters of before -- the caller's business.
 */
#ifndef SACTD3_DORMANT_H
#define SACTD3_DORMANT_H

#include "sactd3.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SACTD3_DORMANT_ACTOR = 1, SACTD3_DORMANT_CRITICS = 2 };

/* Scan the n rows idx[r * idx_ld] for the nets `what` names at threshold tau.  scores: NULL, or a contiguous device [6][256]; the rows
 * of the scanned nets are written, the others are not.  flags: SACTD3_SRC_ORDERED | SACTD3_DST_ORDERED against caller_stream (idx is
 * read behind what that stream holds; what it queues next waits for the scores).  Refusals, all in front of any side effect:
 *   SACTD3_EINVAL  a NULL handle or idx; n < 1 or n > 65536; idx_ld < 1; `what` empty or with unknown bits; tau negative or not finite;
 *                  a pointer not on the engine's device; an unknown flag
 *   SACTD3_ESTATE  the ring is empty */
int sactd3_dormant_scan_device(sactd3_engine* e, const int64_t* idx, int64_t idx_ld, int n, uint32_t what, float tau,
                               float* scores, void* caller_stream, int flags);
/* out = {scans, valid rows of the last scan, rows refused so far, dormant count of the six pairs at the last scan (6 values), redo calls,
 * neurons recycled so far, rows left zero, 0 ...}.  Device words: [sync]. */
int sactd3_dormant_stats(sactd3_engine* e, int64_t out[16]);
/* Recycle what the last scan marked in the nets of `what` at (seed, epoch).  Refusals, all in front of any side effect:
 *   SACTD3_EINVAL  a NULL handle; `what` empty or with unknown bits
 *   SACTD3_ESTATE  no scan of those nets since creation or since their last sactd3_redo / sactd3_init_params; an acting call is in
 *                  flight (sactd3_predict_begin without its end) */
int sactd3_redo(sactd3_engine* e, uint32_t what, uint64_t seed, uint32_t epoch);

#ifdef __cplusplus
}
#endif
#endif /* SACTD3_DORMANT_H */
