/*
 * sactd3_returns.h -- Monte-Carlo returns-to-go of replay-ring rows, computed on the device (libsactd3_hip.so; include it beside
 * sactd3.h).  The ABI version stays 1: two functions are added, nothing that existed changes.
 *
 * The library's other questions about ring rows ask the networks; this one asks the data what actually happened after a row: the
 * discounted return from the row to the end of its episode as the ring holds it.  Uses: the critics' bias on the data, Q(s, a) - G;
 * return and length statistics of a loaded dataset; return-filtered behaviour cloning; Monte-Carlo lower bounds on targets.
 *
 * Range.  count == 0 (then first must be 0): the whole ring in age order, n = rb_len, base = rb_len < capacity ? 0 : cursor,
 * slot(age) = (base + age) mod capacity -- the `age` of the n-step staging.  count > 0: the slots [first, first + count) in slot order,
 * base = first, n = count; the range must lie inside [0, rb_len).  This is the form for a pinned dataset prefix.
 *
 * Chain rule (the n-step rule, word for word).  The successor of age g is age g + stride and exists iff g + stride < n.  The link
 * g -> g + stride holds iff the successor exists, the flag float of row g is 0, and the first ob_dim floats of g's s' field equal the
 * first ob_dim floats of the successor's record as 32-bit patterns (-0.0 != +0.0, equal NaN patterns are equal).  A row's chain is the
 * row and every row reached from it over links that hold.
 *
 * Outputs, indexed by ring SLOT (element slot * ld of each array); rows outside the range are not written:
 *   returns       G = sum_j gamma^j r_{t+j} over the chain, float32
 *   undiscounted  the same sum with gamma = 1
 *   length        L >= 1, the rows of the chain
 *   last          the ring slot of the chain's last row
 *   ends          exactly one of SACTD3_RTG_TERMINATED (the last row's flag != 0), SACTD3_RTG_TRUNCATED (flag 0, the successor exists,
 *                 the bits differ), SACTD3_RTG_OPEN (flag 0, no successor in the range), plus SACTD3_RTG_START when no row links into
 *                 this one.
 * A broken link is a flag of the scan, never a multiplication by zero: a NaN or infinite reward makes the returns of the rows at or
 * before it in its own chain non-finite and touches nothing else.  Such rewards are counted (stats).
 *
 * Arithmetic.  Positions are chain-major (chain c = age mod stride owns consecutive positions, t = age div stride ascending) and cut
 * into spans of SACTD3_RTG_SPAN; the sums are one fixed tree of float32 operations per (range, stride), products rounded, then added,
 * nothing contracted: the outputs are a pure function of (ring, range, stride, gamma).  At most L multiplications and L additions lie
 * on the path of any term.  A chain of one row returns its reward bit for bit.
 *
 * Semantics are those of sactd3_ring_knn_device: eager launches on the learner stream behind every update issued before, no copy, no
 * host wait; SACTD3_SRC_ORDERED / SACTD3_DST_ORDERED order the caller's arrays both ways against `caller_stream`.  The call is
 * invisible to training and acting: scratch of its own (sized by the ring's capacity, made at its first use), no batch slot, counter,
 * noise buffer or acting scratch moves, a precomputed opening pair of sactd3_step_period stays valid, and the call is allowed while
 * sactd3_predict_begin is in flight.
 */
#ifndef SACTD3_RETURNS_H
#define SACTD3_RETURNS_H

#include "sactd3.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SACTD3_RTG_TERMINATED = 1, SACTD3_RTG_TRUNCATED = 2, SACTD3_RTG_OPEN = 4, SACTD3_RTG_START = 8 };   /* bits of `ends` */
#define SACTD3_RTG_SPAN 2048   /* positions of one workgroup of the scan */

typedef struct sactd3_returns_io {        /* device pointers, NULL = not wanted; ld: the stride between two slots, in elements (>= 1) */
  float*   returns;      int64_t returns_ld;
  float*   undiscounted; int64_t undiscounted_ld;
  int32_t* length;       int64_t length_ld;
  int32_t* last;         int64_t last_ld;
  int32_t* ends;         int64_t ends_ld;
} sactd3_returns_io;

/* Refusals, all in front of any launch, the engine left usable.  SACTD3_EINVAL: a NULL handle or io; no output set; gamma outside
 * [0, 1] or NaN; stride < 1 or above the ring's capacity; first < 0, count < 0, first != 0 beside count == 0, or a range that leaves
 * [0, rb_len) of a ring that holds rows; an unknown flag (SACTD3_SRC_ORDERED | SACTD3_DST_ORDERED); a stride between slots below 1; a
 * pointer not on the engine's device.  SACTD3_ESTATE: the ring is empty; count == 0 while rows are pinned (two wrap points exist
 * there: ask for the pinned prefix and the live rows by range). */
int sactd3_returns_to_go_device(sactd3_engine* e, float gamma, int stride, int64_t first, int64_t count,
                                const sactd3_returns_io* io, void* caller_stream, int flags);
/* out = {calls, rows scanned, chains that end TERMINATED, TRUNCATED, OPEN, START rows, non-finite rewards, 0}, summed over the calls.
 * Device memory: [sync]. */
int sactd3_returns_to_go_stats(sactd3_engine* e, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* SACTD3_RETURNS_H */
