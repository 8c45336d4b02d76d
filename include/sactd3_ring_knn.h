/*
 * sactd3_ring_knn.h -- the k nearest replay-ring rows of each query, searched on the device (libsactd3_hip.so; include it beside
 * sactd3.h).  The ABI version stays 1: two functions are added, nothing that existed changes.
 *
 * The library's other questions take rows the caller picks; this one asks the ring itself which rows look like a given one.  Three
 * uses: particle-based state entropy and novelty (APT, Liu & Abbeel 2021; RE3, Seo et al. 2021: the k-th-nearest-neighbour distance of
 * a state among the replayed states); the dataset-constraint distance of an offline run (PRDC, Ran et al. 2023: from (beta s, pi(s)) to
 * the nearest (beta s_i, a_i) of the data); coverage and duplicate checks of a loaded dataset.
 *
 * Keys.  A ring record starts with s (ob_dim floats) and a (ac_dim floats).  key == SACTD3_KNN_STATE: D = ob_dim, the key is s;
 * SACTD3_KNN_STATE_ACTION: D = ob_dim + ac_dim, the key is [s | a].  D <= SACTD3_KNN_MAX_D.  Both sides are transformed alike,
 *   key'_d = (key_d - c_d) * w_d        (float32, two roundings; c = `offset`, default 0; w = `scale`, default 1),
 * so `queries` [n, D] are given in the ring's own units.  Any row stride >= D, no alignment beyond 4 bytes.
 *
 * Range.  The search runs over the ring slots [first, first + count) n [0, rb_len); count == 0 means "to rb_len", so a pinned dataset
 * prefix can be searched alone.
 *
 * Selection.  For a (query, slot) pair the selector is
 *   sel = xn - 2 dot,     xn = sum_d x'_d x'_d,     dot = sum_d q'_d x'_d      (float32; |q'|^2, common to a query's pairs, is left out)
 * each summed in one fixed order over d that depends on neither the pair's place in a tile nor the grid: with d = 16 C + 4 g + j
 * (g, j = 0 .. 3; the key zero-extended to a multiple of 16), dot takes the terms in the order (C, j) ascending, the four g of one
 * (C, j) being the four products of one v_mfma_f32_16x16x4f32; xn = (p_0 + p_1) + (p_2 + p_3) with p_g the sum over (C, j) ascending
 * of x'_d x'_d (products rounded, then added).  The k slots with the smallest (sel, slot) win; `exclude` names one slot per query that
 * never does.
 *
 * Reported distance.  For the k winners dist2 = sum_d (q'_d - x'_d)^2 is recomputed directly: d ascending, float32, every operation
 * rounded once, nothing contracted.  The winners are written by (dist2, slot) ascending.  Where fewer than k slots exist the rest of
 * a row is index -1, dist2 +inf, and the query is counted (stats).
 *
 * Determinism.  A query's outputs are the same bits whatever n is, whichever queries stand beside it, and however the ring is cut
 * into slices: the winners are THE k smallest (sel, slot) of the range, and sel is a function of the pair alone.
 *
 * Non-finite values.  A query with a non-finite transformed key yields index -1 and dist2 NaN in all k places and is counted.  A ring
 * row whose sel is not finite is never selected; ring rows of the range whose xn is not finite are counted, once per call.  Neither is
 * ever a fault.
 *
 * Slices.  The range of L rows is cut into slices of R rows, R a multiple of 16, as a function of L alone:
 *   S0 = min(256, max(1, ceil(L / 64))),   R = 16 ceil(ceil(L / S0) / 16),   S = ceil(L / R)  (<= 256).
 * One workgroup scans one slice for one tile of 64 queries and leaves its k best per query; a second kernel merges the S lists.  The
 * partial slab is therefore of a fixed size (256 slices x 1 024 queries x 16), made at the first call.
 *
 * Semantics are those of sactd3_action_gradient_device: eager launches on the learner stream behind every update issued before, any
 * n >= 1 in chunks of at most 1 024 queries, no copy, no host wait; SACTD3_SRC_ORDERED / SACTD3_DST_ORDERED order the caller's arrays
 * both ways against `caller_stream`.  The call is invisible to training and acting: scratch and control words of its own, made at its
 * first use; no batch slot, counter, noise buffer or acting scratch moves, a precomputed opening pair of sactd3_step_period stays
 * valid, and the call is allowed while sactd3_predict_begin is in flight.
 */
#ifndef SACTD3_RING_KNN_H
#define SACTD3_RING_KNN_H

#include "sactd3.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SACTD3_KNN_STATE = 0, SACTD3_KNN_STATE_ACTION = 1 };   /* key = a record's leading s (D = ob_dim) or [s | a] (D = ob_dim + ac_dim) */
#define SACTD3_KNN_MAX_K 16
#define SACTD3_KNN_MAX_D 416   /* key width at most: the 64 queries of a tile stay in one workgroup's LDS */

typedef struct sactd3_ring_knn_io {       /* device pointers; NULL = not given / not wanted */
  const float*   offset;                  /* in  [D]: c_d, default 0                                            */
  const float*   scale;                   /* in  [D]: w_d, default 1      key'_d = (key_d - c_d) * w_d           */
  const int64_t* exclude; int64_t exclude_ld;   /* in [n]: one ring slot per query that is never reported (-1: none) */
  int64_t* index;  int64_t index_ld;      /* out [n, k]: ring slots, by (dist2, slot) ascending; -1 where fewer than k exist */
  float*   dist2;  int64_t dist2_ld;      /* out [n, k]: squared distance; +inf beside an index of -1           */
} sactd3_ring_knn_io;

/* Refusals, all in front of any launch, the engine left usable.  SACTD3_EINVAL: a NULL handle, queries or io; no output set; n < 1;
 * k outside [1, 16]; an unknown key or flag (SACTD3_SRC_ORDERED | SACTD3_DST_ORDERED); first < 0 or count < 0; a stride below its
 * width (exclude_ld < 1 where `exclude` is given); a pointer not on the engine's device; a key wider than SACTD3_KNN_MAX_D.
 * SACTD3_ESTATE: the ring is empty, or the range is empty after clipping. */
int sactd3_ring_knn_device(sactd3_engine* e, const float* queries, int64_t queries_ld, int n, int k, int key,
                           int64_t first, int64_t count, const sactd3_ring_knn_io* io, void* caller_stream, int flags);
/* out = {calls, queries, ring rows scanned (the range lengths, summed over the calls), non-finite queries, non-finite ring keys
 * skipped, short results (< k found), 0, 0}.  Device memory: [sync]. */
int sactd3_ring_knn_stats(sactd3_engine* e, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* SACTD3_RING_KNN_H */
