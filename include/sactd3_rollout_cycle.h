/*
 * sactd3_rollout_cycle.h -- the part of include/sactd3_rollout.h that issues one whole env step of a training loop as ONE graph
 * launch.  It is included by sactd3_rollout.h (behind its types) and declares nothing on its own: include that header.  The ABI
 * version stays 1: three functions are added, nothing that existed changes.
 *
 * One body of a training loop on a GPU-resident env is
 *     sactd3_rollout_advance(r);  sactd3_rollout_choose(r, mode);  sactd3_step(engine, do_actor);
 * -- three calls, a dozen small dependent launches on two streams, four event hand-overs between them.  sactd3_rollout_cycle is the
 * same launches as ONE linear graph on the engine's stream, captured once per (mode, iteration schedule) and replayed while the ring
 * grows and wraps: the ring append takes its cursor from device memory (csrc/rollout_cycle.hip: k_rb_ingest_g), as the acting pair
 * and the iteration already take their counters.
 *
 * Equivalence.  The call is bit for bit the three-call sequence above -- device memory: the ring, the env's state and books, `obs` /
 * `actions` / `records`, every parameter, the Adam state, the counters, the noise buffers, the batch slot; host state: the rollout's
 * stats, the ring's length / cursor / wrapped flag, the update count, the batch generation, what the batch slot and the gradient arenas
 * are known to hold, the order against an acting stream, sactd3_predict_device_stats.  The ONLY host counters that may differ are those of
 * sactd3_boundary_stats: the cycle records one pair of events where the sequence records two (ordered_calls grows by 1, not by 2).
 *
 * Streams.  The graph runs on the engine's stream.  The rollout's stream is ordered around it once per call, with the two events of
 * SACTD3_SRC_ORDERED: the cycle runs behind what the rollout's stream held at the call (a reset, a write of the buffers), and what that
 * stream is given next (sactd3_env_episode_stats, a reset, a read of the buffers) runs behind the cycle.  Nothing waits on the host --
 * except that a cycle of ANOTHER rollout of the same engine, and sactd3_rollout_destroy, first wait for the engine's stream to drop
 * the graphs of the binding that held them.
 *
 * The graph.  One per (mode, k), k = 2 (actor updates run) + (targets are updated): at most 8, captured from the engine's stream at first
 * use, never updated, never re-instantiated.  Its nodes, in order: the env step (k_env_step_rec); the ring append (k_rb_ingest_g, and
 * behind a slab of more than one block the single-thread k_rb_publish_g); the observation pack; the acting pair (with its counter launch
 * behind a multi-block tail); the action unpack; the uniform iteration of sactd3_step.  No parallel branches.  The rollout's three
 * buffers are in the nodes by value: they are fixed for the rollout's life anyway.  The graphs belong to the rollout binding, not to the
 * engine's table: sactd3_instantiate_graphs does not build them (it has no rollout to build them from) and sactd3_graph_kernel_count
 * does not count them.  With sactd3_config::use_graphs == 0 the same launches go out eagerly, in the same order, from the same definition.
 *
 * A rollout that has issued a cycle must be destroyed BEFORE its engine (the rule of sactd3_rollout_create, now with a reason: the
 * engine holds graphs whose nodes point into the rollout's buffers).
 */
#ifndef SACTD3_ROLLOUT_CYCLE_H
#define SACTD3_ROLLOUT_CYCLE_H

#ifndef SACTD3_ROLLOUT_H
#error "include sactd3_rollout.h: it declares the rollout handle and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* sactd3_rollout_advance(r); sactd3_rollout_choose(r, mode); sactd3_step(engine, do_actor) -- as ONE graph launch.
 * Refusals, all in front of any side effect (a refused call has launched, counted and moved nothing):
 *   SACTD3_EINVAL  a NULL handle; `mode` is not SACTD3_ROLLOUT_EXPLORE or SACTD3_ROLLOUT_EXPLOIT (a random or repeated choice runs no
 *                  update: it stays on the call sequence); num_envs above the ring's capacity (one append launch must hold the slab)
 *   SACTD3_ESTATE  rows are pinned (sactd3_rb_pin); priorities are enabled (sactd3_prio_enable: the append would owe their launches);
 *                  an acting call is in flight (sactd3_predict_begin without its end)
 * The iteration inside is the uniform one of sactd3_step; the draws of sactd3_step_sampled are not served. */
int sactd3_rollout_cycle(sactd3_rollout* r, int mode, int do_actor);
/* host counters: out = {cycles issued, graphs captured, nodes of the last graph launched, cycles issued eagerly (use_graphs == 0)} */
int sactd3_rollout_cycle_stats(const sactd3_rollout* r, int64_t out[4]);
/* *out = appends of a cycle that found a ring length outside [0, capacity] or a cursor outside [0, capacity) in device memory: the
 * kernel bounds both before it derives an address and counts the append.  0 in every run whose ring the engine's own calls wrote.
 * Waits for the engine's stream. */
int sactd3_rollout_cycle_clamped(sactd3_rollout* r, int64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* SACTD3_ROLLOUT_CYCLE_H */
