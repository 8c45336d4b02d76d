// Host side of libsactd3_hip.so: memory plan, kernel sequences, hipGraph capture, C ABI (include/sactd3.h).
//
// The kernel sequences restate agents/agent.py:183-331 of the reference in the decomposition that
// oracle/manual_grads.py documents (and checks against autograd).  One engine owns:
//   - parameter / gradient / Adam arenas (flat, padded so that every row is float4 aligned),
//   - the HBM replay ring (one 64-byte-aligned record per transition),
//   - one batch slot and all activations of one iteration,
//   - a HIP stream and the captured graphs of update_qnets / update_actor / whole iterations.
// No torch, no BLAS: the .so depends on libamdhip64 only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <chrono>
#include <vector>

#include "../../include/sactd3.h"
#include "kernels.h"
__global__ void k_set_int1(int* dst, int v) { if (threadIdx.x == 0 && blockIdx.x == 0) *dst = v; }      // (set_flag)
#include "prio_kernels.h"
#include "nstep_kernels.h"
#include "mix_kernels.h"
#include "policy_kernels.h"
// All device code stands above.  The order of the template instances in the code object is pinned by this list, not by where the
// host code below names them: a new instance is appended there.
#include "kernel_instances.inc"
// the hindsight kernels are a translation unit of their own (hindsight.hip): only their argument structs and launchers are known here
#include "hindsight.h"
// ... and so is the graph form of the ring append (rollout_cycle.hip); the same header is how the rollout handle (env.hip) asks for a cycle
#include "rollout_cycle.h"
// ... and the parameter initialiser (param_init.hip; its C ABI is include/sactd3_init.h, defined at the end of the extern "C" block below)
#include "param_init.h"
#include "../../include/sactd3_init.h"
// ... and the evaluation rollout, whose kernel is compiled with the env kernels (env.hip): host code only here, at the end of this file
#include "eval_rollout.h"
// ... and the collected rollout segment, split the same way (collect_rollout.h)
#include "collect_rollout.h"

static thread_local std::string g_create_error;

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
// ceil(2^32 / d) if it divides every n < n_max exactly via mulhi (n_max * d < 2^32), else 0 (= use a real division)
static inline unsigned magic_div(unsigned d, unsigned long long n_max) {
  return (d > 1 && n_max * d < (1ull << 32)) ? (unsigned)(((1ull << 32) + d - 1) / d) : 0u;
}

static NetLayout make_layout(int K, int nh) {
  NetLayout L{};
  L.K = K; L.ld1 = round_up(K, 4); L.nh = nh;
  int off = 0;
  L.W1 = off; off += HID * L.ld1;
  L.b1 = off; off += HID; L.g1 = off; off += HID; L.be1 = off; off += HID;
  L.W2 = off; off += HID * HID;
  L.b2 = off; off += HID; L.g2 = off; off += HID; L.be2 = off; off += HID;
  L.Wh = off; off += nh * HID;
  L.bh = off; off += round_up(nh, 4);
  L.size = off;
  return L;
}

// reference (state_dict order, unpadded) <-> arena (padded) for one net
static int64_t ref_count(const NetLayout& L, int ln) {
  return (int64_t)HID * L.K + HID + (ln ? 2 * HID : 0) + (int64_t)HID * HID + HID + (ln ? 2 * HID : 0) + (int64_t)L.nh * HID + L.nh;
}
static void pack_net(const NetLayout& L, int ln, const float* src, float* dst, bool is_param) {
  std::fill(dst, dst + L.size, 0.f);
  if (is_param && !ln) {  // unused LN affine: identity
    std::fill(dst + L.g1, dst + L.g1 + HID, 1.f);
    std::fill(dst + L.g2, dst + L.g2 + HID, 1.f);
  }
  for (int r = 0; r < HID; ++r) { memcpy(dst + L.W1 + (size_t)r * L.ld1, src, sizeof(float) * L.K); src += L.K; }
  memcpy(dst + L.b1, src, sizeof(float) * HID); src += HID;
  if (ln) { memcpy(dst + L.g1, src, sizeof(float) * HID); src += HID; memcpy(dst + L.be1, src, sizeof(float) * HID); src += HID; }
  memcpy(dst + L.W2, src, sizeof(float) * HID * HID); src += HID * HID;
  memcpy(dst + L.b2, src, sizeof(float) * HID); src += HID;
  if (ln) { memcpy(dst + L.g2, src, sizeof(float) * HID); src += HID; memcpy(dst + L.be2, src, sizeof(float) * HID); src += HID; }
  memcpy(dst + L.Wh, src, sizeof(float) * L.nh * HID); src += (size_t)L.nh * HID;
  memcpy(dst + L.bh, src, sizeof(float) * L.nh);
}
static void unpack_net(const NetLayout& L, int ln, const float* src, float* dst) {
  for (int r = 0; r < HID; ++r) { memcpy(dst, src + L.W1 + (size_t)r * L.ld1, sizeof(float) * L.K); dst += L.K; }
  memcpy(dst, src + L.b1, sizeof(float) * HID); dst += HID;
  if (ln) { memcpy(dst, src + L.g1, sizeof(float) * HID); dst += HID; memcpy(dst, src + L.be1, sizeof(float) * HID); dst += HID; }
  memcpy(dst, src + L.W2, sizeof(float) * HID * HID); dst += HID * HID;
  memcpy(dst, src + L.b2, sizeof(float) * HID); dst += HID;
  if (ln) { memcpy(dst, src + L.g2, sizeof(float) * HID); dst += HID; memcpy(dst, src + L.be2, sizeof(float) * HID); dst += HID; }
  memcpy(dst, src + L.Wh, sizeof(float) * L.nh * HID); dst += (size_t)L.nh * HID;
  memcpy(dst, src + L.bh, sizeof(float) * L.nh);
}

static const int BIG_BATCH = 1024;   // from here on the hidden layers run as 64 x 64-tiled GEMMs + a LayerNorm row kernel
enum { G_Q = 0, G_A = 1, G_STEP00 = 2, G_STEP01 = 3, G_STEP10 = 4, G_STEP11 = 5, G_PERIOD = 6, G_PERIOD_B = 7, G_OPENING = 8,
       G_PREFIX = 9 /* + 2 (m - 1) + variant, m = 1, 2: the first m iterations of a period (sactd3_step_prefix) */,
       G_QW = 13 /* update_qnets in its weighted form: captured at its first use only */,
       G_RUN = 14 /* + start variant (sactd3_step_periods) */, G_SAMPLED = 16 /* + 2 do_actor + target update (sactd3_step_sampled) */,
       G_CYCLE = 20 /* + (explore ? 0 : 4) + IterSchedule::k (sactd3_rollout_cycle) */, G_COUNT = 28 };
static const int NSTAGE = 32;

struct NodeInfo { std::string name; double flops; double bytes; long threads; };
// Ring rows into batch slot 0, described once for a call form (sactd3_rb_sample_*) and for a place in a captured iteration
// (sactd3_step_sampled): what such a draw refuses, allocates, launches and leaves in the host state stands in draw_state_refusal,
// draw_alloc, draw_launches and draw_issued, and nowhere else.  kind: SACTD3_DRAW_*; beta: the importance exponent of a prioritised draw;
// steps == 0: one ring row per batch row (k_batch_from_index), steps >= 1: rows chained into n-step returns over (steps, stride) by
// k_batch_from_index_nstep (sactd3_rb_sample_nstep takes it at steps == 1 too).  rows: the caller chose them and nothing is drawn --
// kind then names the staging kernel alone: SACTD3_DRAW_UNIFORM the two above, SACTD3_DRAW_HINDSIGHT k_hindsight_stage.
struct CallerRows {
  const long long* idx = nullptr; int64_t idx_ld = 1; const float* w = nullptr; int64_t w_ld = 1;      // ring slots [, loss weights]
  const int* choice = nullptr; int64_t choice_ld = 1;      // hindsight: the relabelling choices (NULL: the kernel draws them)
  bool weighted = false;                                   // the slot carries loss weights behind the call
};
struct Draw {
  int kind = SACTD3_DRAW_UNIFORM; float beta = 0.f; int steps = 0, stride = 0; const CallerRows* rows = nullptr;
  bool chain() const { return steps > 0; }
  bool weighted() const { return rows ? rows->weighted : kind == SACTD3_DRAW_PRIORITIZED; }
  bool same_graphs(const Draw& d) const { return kind == d.kind && steps == d.steps && stride == d.stride; }      // (beta is read on the device)
};
struct sactd3_engine {
  sactd3_config cfg{};
  std::string err;
  hipStream_t stream = nullptr;
  std::vector<void*> dev_allocs, host_allocs;
  std::vector<hipEvent_t> events;

  int o = 0, a = 0, B = 0, ldc = 0, ldo = 0, a4 = 0, nh = 0, ldu = 0, rec_f = 0, rec4 = 0, cx = 0, cn = 0;
  int nq_actor = 2;            // critics evaluated in the actor update (SAC 2, TD3 1)
  int nblk = 0, nblk4 = 0;     // row-kernel blocks for B rows: 16 rows each (MFMA-using tails) / 4 rows each (plain row kernels)
  int maxn = 0;                // rows accepted by predict
  int num_cus = 256;
  int stage_rows = 0;
  NetLayout La{}, Lc{};

  DevCtl* ctl = nullptr;
  float *min_ac = nullptr, *max_ac = nullptr, *scale = nullptr, *bias = nullptr;
  float *Pa = nullptr, *Ta = nullptr, *Ga = nullptr, *Ma = nullptr, *Va = nullptr;
  float *Ta2 = nullptr, *Ta3 = nullptr;     // TD3 period graphs: the actor target one / two Polyak steps ahead (TnArgs::T2, T3)
  float *Pc = nullptr, *Tc = nullptr, *Gc = nullptr, *Mc = nullptr, *Vc = nullptr;
  float *la = nullptr, *gscale = nullptr;
  float* ring = nullptr; float* stage_dev = nullptr;
  float *X = nullptr, *Xn = nullptr, *Xp = nullptr, *rew = nullptr, *done = nullptr;
  int* idx = nullptr;
  float *logp_n = nullptr, *logp_pi = nullptr, *logp_al = nullptr, *act_scratch = nullptr;
  float* eps[SACTD3_NUM_SITES] = {};
  float *a_z1 = nullptr, *a_xh1 = nullptr, *a_h1 = nullptr, *a_rs1 = nullptr, *a_z2 = nullptr, *a_xh2 = nullptr, *a_h2 = nullptr, *a_rs2 = nullptr, *a_tg = nullptr;
  float *a_du = nullptr, *a_dz2 = nullptr, *a_dh1 = nullptr, *a_dz1 = nullptr;
  float *qa_ps = nullptr, *qa_S = nullptr;   // dQ/da partials of the fused actor update (QaFold): [nq][B][16][16], [nq][16][8]
  float *a_ps = nullptr, *c_ps = nullptr;     // row-sum partials of the folded layer-1 LayerNorm backward (TnProb::fold): [nets][B][PS_W]
  float* a_z2n = nullptr;        // layer-2 output of the s' pass when the pi(s) pass shares its launch
  float* ah_z1[4] = {}; float* ah_z2[4] = {};   // layer outputs of the passes that run ahead (pipelined period, see BatchSlot)
  // Batch slots.  Slot 0 is THE batch slot (X, Xn, rew, done, idx, logp_n, eps of the critic site above).  A pipelined period graph
  // (sactd3_step_period, SAC) samples and runs the next-action pass of its critic-only iterations AHEAD, inside the last actor
  // update's launches -- the actor does not change in between -- into slots 1 and 2, which those iterations then train on; and it
  // does the same for the opening pair of the NEXT period's first iteration (next-action pass on s' and the first actor update's
  // policy pass on s), whose slot alternates between 0 and 3 from one period to the next (the running period still reads its own).
  struct BatchSlot { float *X, *Xn, *rew, *done, *logp_n, *eps_c; int* idx; float* w; } bs[4] = {};      // w: loss weights [B], slot 0 only, see below
  // What the host knows about the slots.  cur: the slot the most recent update trained on, or 0 behind a refill (what read_batch /
  // read_noise / debug_read / the TD write-back report).  weighted: slot 0 carries loss weights -> sactd3_update_qnets replays the weighted
  // graph (G_QW).  nstep: slot 0 was filled by an n-step staging (ns_k / ns_last describe its rows).  td_valid: e->q / e->y belong to a
  // critic update on the rows now in bs[cur] (sactd3_td_errors_device, sactd3_prio_update_from_td).  Written by the two transitions
  // slot_refilled / slot_trained alone -- and by slot_set_weighted, for sactd3_batch_weights_device, which changes `weighted` only.
  // generation: how often the rows that read_batch reports were replaced (sactd3_batch_generation); it only ever grows.
  // hindsight: slot 0 was filled by a hindsight staging (hs_off / hs_gs describe its rows); every other refill and every fused update clears it.
  struct SlotState { int cur = 0; bool weighted = false, nstep = false, td_valid = false; int64_t generation = 0; bool hindsight = false; } slot;
  // chain_ready = v (0 / 1): the previous sactd3_step_period left the opening pair of the next period precomputed in slot (v ? 3 : 0)
  // and nothing has touched the state it depends on since (parameters, ring length, counters, noise injection, the slots);
  // -1: not so -- the next period starts with the opening graph.  Every state-changing ABI call resets it (CHAIN_BREAK).
  int chain_ready = -1;
  // Stores that only inspection reads (debug_read: the gradient arenas, the folded launches' dz1) are left out of the period and cut-short
  // period sequences when the optimiser step is fused and nothing clips (EnqCtx::lean_stores, set by enqueue_period:
  // launch_tn).  grads_stale[0 critics, 1 actor]: such a sequence ran since that family's arenas were last written in full --
  // sactd3_debug_read refuses the family's names (grad_*, *_dz1) until an API-path update or a sactd3_step rewrites them.
  bool grads_stale[2] = {false, false};
  float *c_z1 = nullptr, *c_xh1 = nullptr, *c_h1 = nullptr, *c_rs1 = nullptr, *c_z2 = nullptr, *c_dz2 = nullptr, *c_dh1 = nullptr, *c_dz1 = nullptr;
  float *t_z1 = nullptr, *t_z2 = nullptr, *q = nullptr, *qt = nullptr, *y = nullptr, *q_pi = nullptr, *dA = nullptr;
  float* s_h1 = nullptr;         // large-batch path: layer-1 activations of nets whose caller keeps no copy ([4][B][256])
  float* Gp = nullptr; int gp_slabs = 0;      // large-batch path: split-M partial slabs of the weight gradients ([slab][nets][arena])
  float *part = nullptr, *part_s = nullptr, *part_sa = nullptr;   // column partials; scalar partials of the critic / actor updates
  float *p_x = nullptr, *p_z1 = nullptr, *p_z2 = nullptr, *p_act = nullptr;
  float *h_obs = nullptr, *h_act = nullptr;      // pinned predict staging
  int* h_done = nullptr; int predict_calls = 0;  // pinned completion word of the acting tail / calls issued (see ActorTail::done_flag)
  float* h_stage[NSTAGE] = {}; int stage_next = 0, stage_used = 0;   // pinned staging slots of rb_extend
  float* h_batch = nullptr;                      // pinned [B][rec_f]

  int64_t rb_len = 0, rb_cursor = 0, qnet_updates = 0;
  hipGraphExec_t graphs[G_COUNT] = {}; int graph_nodes[G_COUNT] = {};      // every learner and cycle graph, by its G_* id (enqueue_graph says what each holds)
  std::vector<hipGraphExec_t> predict_graphs;   // [explore][n]: the two launches of sactd3_predict, captured per row count
  // Acting on a stream of its own (sactd3_predict_begin / _end), created at the first begin.  Order between the two streams is kept
  // by the host, with events, only where the acting kernels and a learner call touch the same memory -- the actor parameters:
  //   actor_dirty   a write of them was issued on the learner stream since the acting stream last waited for it -> the next begin waits
  //                 (also set by sactd3_predict_device, whose queued kernels use the acting scratch, draw buffer and counter);
  //   act_inflight  a call has begun and not ended -> the next learner call that writes them waits for it first (act_ordered: one did).
  hipStream_t act_stream = nullptr;
  hipEvent_t ev_learner = nullptr, ev_acting = nullptr;
  bool actor_dirty = true, act_inflight = false, act_ordered = false, act_spin = false;
  int act_n = 0, act_want = 0;
  int64_t act_stats[4] = {};                    // sactd3_acting_stats
  // The device boundary (sactd3_rb_extend_fields_device / sactd3_load_batch_device): the two events that order the learner stream
  // against the caller's producer stream, created at the first SACTD3_SRC_ORDERED call, and the host counters of sactd3_boundary_stats.
  hipEvent_t ev_src_ready = nullptr, ev_src_read = nullptr;
  int64_t bnd_stats[4] = {};
  // The same boundary outwards (sactd3_read_batch_device / sactd3_rb_read_rows_device): host counters of sactd3_readout_stats
  // {batch read-outs, row read-outs, rows requested}; the fourth, rows refused, is DevCtl::readout_refused.
  int64_t ro_stats[3] = {};
  long long* time_idx = nullptr;                // sactd3_time_kernel("rows_to_fields"): its index array
  // Acting on device observations (sactd3_predict_device): [explore][n] graphs of the acting pair on p_x / p_act -- they hold no
  // caller pointer -- and the host counters of sactd3_predict_device_stats.
  std::vector<hipGraphExec_t> predict_dev_graphs;
  int64_t pdev_stats[4] = {};
  // Scoring caller-supplied rows (sactd3_qvalues_device): scratch for Q_CHUNK rows, made at the first call (the actor's at the first
  // policy-form call) -- packed [s | a | 0] rows at ldc and z1 / z2 of the two critics; the actor's x / z1 / z2 / action rows -- and the
  // host counters of sactd3_qvalues_stats.  Nothing else of the engine is written by a scoring call.
  float *qs_sa = nullptr, *qs_z1 = nullptr, *qs_z2 = nullptr;
  float *qs_x = nullptr, *qs_az1 = nullptr, *qs_az2 = nullptr, *qs_act = nullptr;
  float *qs_hq = nullptr, *qs_hobs = nullptr, *qs_hact = nullptr;      // sactd3_qvalues (host arrays): device staging of one chunk
  int64_t q_stats[4] = {};
  // Querying the policy on caller-supplied rows (sactd3_policy_device; device code: policy_kernels.h).  Everything below is made at the
  // first call -- an engine that never asks holds nothing more and launches nothing more than before.  pi_x / pi_z1 / pi_z2: packed
  // observations and the actor trunk's two outputs for Q_CHUNK rows; pi_ctl[0]: the native draws' counter and the two row counters,
  // pi_ctl[1]: the same words for sactd3_time_kernel("pi_head"), so that a timing run counts nothing; pi_h*: device staging of the host
  // form; pi_time: the outputs of the timing run.  pi_rows: rows of the last chunk (what "pi_z2" holds; 0: no call yet).
  // pi_stats: {calls, rows}.
  float *pi_x = nullptr, *pi_z1 = nullptr, *pi_z2 = nullptr;
  struct PiCtl* pi_ctl = nullptr;
  float *pi_hobs = nullptr, *pi_hio = nullptr, *pi_time = nullptr;
  int pi_rows = 0;
  int64_t pi_stats[2] = {};
  // Training on caller-chosen rows with loss weights (sactd3_rb_sample_indices_device / sactd3_batch_weights_device): bs[0].w is made at
  // the first staging call -- an engine that never stages weights holds nothing more than before.  prio_stats: {index stagings, weight stagings,
  // td read-outs}; the fourth value of sactd3_priority_stats is DevCtl::priority_refused.
  int64_t prio_stats[3] = {};
  // Proportional prioritised replay as engine state (sactd3_prio_enable; device code and table layout: prio_kernels.h).  Everything
  // below is made by sactd3_prio_enable -- an engine that never calls it holds nothing more and launches nothing more than before.
  // pt_leaf [groups x 1024] = p^alpha per ring slot (0: not filled), pt_sums [ceil(groups / 1024) x 1024] the group sums, both
  // zero-padded; pt_ctl the device words (maximum priority, draw counter, refused rows); pt_idx / pt_dleaf / pt_w / pt_total what a
  // draw leaves for the staging launch; pt_u the injected uniforms (pt_inject: in use).  pt_host: {prioritised samples, write-backs,
  // rows that entered at the maximum priority}; the rows refused on the device are PrioCtl::refused.
  bool pt_on = false, pt_inject = false;
  float pt_alpha = 0.f, pt_eps = 0.f;
  int pt_groups = 0;
  float *pt_leaf = nullptr, *pt_sums = nullptr, *pt_dleaf = nullptr, *pt_w = nullptr, *pt_total = nullptr, *pt_u = nullptr, *pt_ones = nullptr;
  long long* pt_idx = nullptr;
  struct PrioCtl* pt_ctl = nullptr;
  int64_t pt_host[3] = {};
  // N-step returns staged from the ring (sactd3_rb_sample_nstep*; device code: nstep_kernels.h).  ns_k / ns_last [B] and the two device
  // counters ns_ctr {rows cut short, rows refused} are made at the first n-step call -- an engine that never makes one holds nothing
  // more than before.  ns_host: {n-step stagings, rows staged}.
  int *ns_k = nullptr, *ns_last = nullptr, *ns_ctr = nullptr;
  int64_t ns_host[2] = {};
  // The replay-aware iteration as one graph launch (sactd3_step_sampled): one executable graph per (do_actor, target update), G_SAMPLED + k,
  // for the current ss_draw (kind, steps, stride) -- a change of those three drops all four.  Their staging and priority launches are the
  // graph forms (prio_kernels.h), which read the ring length, the cursor, beta and the injection switch from device memory: ss_beta_bits /
  // ss_inject are what the host last published into PrioCtl (-1: nothing yet).  ss_stats: {launches, graph captures, 0, 0}.
  Draw ss_draw;
  int64_t ss_beta_bits = -1; int ss_inject = -1;
  int64_t ss_stats[4] = {};
  // Runs of whole periods as one graph launch (sactd3_step_periods): RUN_PERIODS consecutive pipelined periods, one executable graph
  // per start variant, G_RUN + v (the run that starts on variant v leaves chain_ready == v behind: RUN_PERIODS is even).
  // run_stats: {calls, run launches, single-period launches made inside those calls, run graphs captured}.
  int64_t run_stats[4] = {};
  // TD3+BC (sactd3_config::bc_alpha > 0 at create; kernels.h: BcArgs).  bc_on picks the BC forms of the head-backward launch and of the
  // actor's weight-gradient launch, for good; bc_alpha / bc_weight mirror DevCtl::bc, which is what the kernels read (sactd3_set_bc
  // republishes it with one launch: no captured graph holds a value).  bc_part [nblk4]: the head backward's partial sums of (pi - a)^2,
  // made at create only when bc_on -- an engine without BC holds nothing more than before.
  bool bc_on = false;
  float bc_alpha = 0.f, bc_weight = 1.f;
  float* bc_part = nullptr;
  // Prior data under an online run (sactd3_rb_pin / sactd3_rb_set_mix; device code: mix_kernels.h).  rb_pinned = P: appends go round
  // [P, cap) and never write slots [0, P) (ring_append, the one place that moves the cursor).  rb_wrapped: an append has overwritten a
  // row -- pinning is allowed before that only.  Run-time state, not part of a checkpoint.  mix_m: batch rows a mixed draw takes from
  // the pinned rows.  mix_ctl (the device's P and m, read by the graph form of the draw) and mix_idx (the drawn slots, int64
  // [B rounded up to 4]) are made at the first mixed draw -- an engine that never mixes holds nothing more than before; mix_pub: what
  // the host last published into mix_ctl (-1: nothing yet).  mix_stats: sactd3_mix_stats.
  int64_t rb_pinned = 0; bool rb_wrapped = false;
  int mix_m = 0;
  struct MixCtl* mix_ctl = nullptr; long long* mix_idx = nullptr;
  int64_t mix_pub[2] = {-1, -1};
  int64_t mix_stats[4] = {};
  // Hindsight relabelling at staging (sactd3_hindsight_configure, sactd3_rb_sample_hindsight*; device code: hindsight_kernels.h, a
  // translation unit of its own).  hs_on / hs_cfg: host state, set by the configure call.  hs_off / hs_gs [B] (per batch row: the offset j
  // and the goal's ring slot) and the device counters hs_ctr {rows relabelled, rows refused, rows whose relabelled reward is 0} are made at
  // the first staging call -- an engine that never makes one holds nothing more than before.  hs_calls: native draws made so far, the
  // first counter word of the next one.  Run-time state, not part of a checkpoint.
  // The graph form (sactd3_step_sampled, SACTD3_DRAW_HINDSIGHT) counts the draws on the device as well: hs_ctr[HS_WORD_MASTER], which its
  // draw kernel advances.  hs_pub: what the host knows that word to hold (-1: nothing yet); hs_calls is published in front of a graph
  // launch only when the two differ (a call-form native draw in between), as mix_publish does for P and m.
  bool hs_on = false;
  sactd3_hindsight_config hs_cfg{};
  int *hs_off = nullptr, *hs_gs = nullptr, *hs_ctr = nullptr;
  int64_t hs_calls = 0, hs_pub = -1;
  // One env step of a native rollout as one graph launch (sactd3_rollout_cycle; engine_rollout_cycle at the end of this file): env step,
  // ring append in its graph form, acting pair, uniform iteration.  One executable graph per (mode, IterSchedule::k), G_CYCLE + 4 exploit + k,
  // for the rollout handle cyc.owner, whose three buffers and env-step launcher its nodes hold by value -- cyc is the binding they were
  // captured from (enqueue_graph reads it): a cycle of another handle, and that handle's destruction, drop all eight.  cyc_ctr: the
  // device word the append counts a clamped cursor / length in; made at the first cycle -- an engine that never cycles holds nothing
  // more than before.  sactd3_instantiate_graphs has no rollout to build them from and leaves these ids alone.
  CycleBinding cyc{};
  int* cyc_ctr = nullptr;
  // Initialising / resetting the networks on the device (sactd3_init_params; device code: param_init_kernels.h, a translation unit of its
  // own).  init_scratch: the Gaussian matrices of all nine weights, each at a fixed offset (init_mats); init_redrawn: the device word that
  // counts redrawn columns.  Both are made at the first call -- an engine that never calls holds nothing more than before.
  // init_host: {calls accepted, weight matrices of the last call}.
  float* init_scratch = nullptr;
  int* init_redrawn = nullptr;
  int64_t init_host[2] = {};
  // On-policy evaluation in one launch (sactd3_eval_rollout; include/sactd3_eval.h; the kernel: eval_kernels.h, compiled in env.hip).
  // ev_ctr: the device word that numbers the feature's draws (stream 0x800); ev_rew / ev_lp: [T][n] rewards and log-probs of the running
  // call, which wait there for its backward pass -- ev_rows floats each, made at the first call; a call that needs more than any before it
  // makes larger ones (the old pair stays until sactd3_destroy: a queued launch may still use it).  An engine that never evaluates holds
  // nothing more than before.  ev_stats: {calls, env steps rolled, calls that drew}.
  int* ev_ctr = nullptr;
  float *ev_rew = nullptr, *ev_lp = nullptr;
  int64_t ev_rows = 0;
  int64_t ev_stats[3] = {};
  // A training segment in one launch (sactd3_rollout_collect; include/sactd3_rollout_collect.h; the kernel: collect_kernels.h, compiled
  // in env.hip).  cl_ctr: the device word that numbers the feature's draws (stream 0x900), made at the first call.
  int* cl_ctr = nullptr;

  int fail(int code, const char* what, hipError_t he = hipSuccess) {
    err = what;
    if (he != hipSuccess) { err += ": "; err += hipGetErrorString(he); }
    return code;
  }
};

#define HIPCHK(call)                                                   \
  do {                                                                 \
    hipError_t _he = (call);                                           \
    if (_he != hipSuccess) return e->fail(SACTD3_EHIP, #call, _he);    \
  } while (0)
// every entry point runs against the engine's own device, whatever the calling thread's current device is
#define USE_DEVICE(e)                                                                        \
  do {                                                                                       \
    hipError_t _he = hipSetDevice((e)->cfg.device_id);                                       \
    if (_he != hipSuccess) return (e)->fail(SACTD3_EHIP, "hipSetDevice", _he);               \
    (void)hipGetLastError();   /* a stale error of an unrelated earlier call must not be blamed on this one */ \
  } while (0)
// any call that changes what a precomputed opening pair depends on (see sactd3_engine::chain_ready)
#define CHAIN_BREAK(e) do { (e)->chain_ready = -1; } while (0)
// The two transitions of sactd3_engine::slot.  slot_refilled: slot 0 was filled outside an update -- it is the current slot, e->q / e->y
// are no longer its rows, and it carries weights / n-step chains only if this refill staged them.
// The generation counts new rows: a refill is one; so is a fused update, which drew its own sample; an update on the rows a refill left
// (sactd3_update_qnets, the tail of sactd3_step_sampled) is none.  These two are its only writers.
static inline void slot_refilled(sactd3_engine* e, bool weighted, bool nstep) { e->slot = {0, weighted, nstep, false, e->slot.generation + 1}; }
// slot_trained: a critic update ran on `slot`.  fused: it was part of an iteration that drew its own sample (sactd3_step and the period
// graphs: a uniform 1-step draw, never weighted); otherwise (sactd3_update_qnets) the slot keeps what its refill staged.
static inline void slot_trained(sactd3_engine* e, int slot, bool fused) {
  e->slot.cur = slot; e->slot.td_valid = true;
  if (fused) { e->slot.weighted = e->slot.nstep = e->slot.hindsight = false; ++e->slot.generation; }
}
static inline void slot_set_weighted(sactd3_engine* e, bool weighted) { e->slot.weighted = weighted; }
// the batch slot that iteration i of a period (or cut-short period) of variant v trains on (see BatchSlot, enqueue_period)
static inline int period_slot(bool pipelined, int v, int i) { return !pipelined ? 0 : i ? i : (v ? 3 : 0); }
#define RCCHK(call)                    \
  do {                                 \
    int _rc = (call);                  \
    if (_rc != 0) return _rc;          \
  } while (0)

template <class T>
static int dalloc(sactd3_engine* e, T** p, size_t count, bool zero = true) {
  void* v = nullptr;
  HIPCHK(hipMalloc(&v, std::max<size_t>(count, 4) * sizeof(T)));
  e->dev_allocs.push_back(v);
  if (zero) HIPCHK(hipMemset(v, 0, std::max<size_t>(count, 4) * sizeof(T)));
  *p = (T*)v;
  return 0;
}
// THE allocation of state made after sactd3_create, at a feature's first use: nothing if *p exists (a call that failed half way keeps
// what it had made), and a zero fill goes onto the learner stream -- a non-blocking one, which a null-stream fill is not ordered with --
// so it stands in front of that stream's next launch.  Every caller runs in front of run_graph, never between the begin and the end
// of a capture (the fill would become a node of the graph): keep it that way.
template <class T>
static int first_use_alloc(sactd3_engine* e, T** p, size_t count, bool zero = true) {
  if (*p) return 0;
  void* v = nullptr;
  HIPCHK(hipMalloc(&v, std::max<size_t>(count, 4) * sizeof(T)));
  e->dev_allocs.push_back(v);
  if (zero) HIPCHK(hipMemsetAsync(v, 0, std::max<size_t>(count, 4) * sizeof(T), e->stream));
  *p = (T*)v;
  return 0;
}
template <class T>
static int halloc(sactd3_engine* e, T** p, size_t count) {
  void* v = nullptr;
  HIPCHK(hipHostMalloc(&v, std::max<size_t>(count, 4) * sizeof(T), hipHostMallocDefault));
  e->host_allocs.push_back(v);
  memset(v, 0, std::max<size_t>(count, 4) * sizeof(T));
  *p = (T*)v;
  return 0;
}

// ------------------------------------------------------------------------------------------------ launches
// What exists only while ONE sequence of launches is enqueued (one graph capture, or one pass of its eager form): created where the
// sequence starts, handed down to every enqueue_* / launch_* function, gone when it ends -- a failed enqueue leaves nothing behind.
struct EnqCtx {
  sactd3_engine* e; hipStream_t s;
  const char* role = "";          // which part of the iteration is being enqueued (names the nodes)
  bool lean_stores = false;       // leave out the stores that only inspection reads (see sactd3_engine::grads_stale)
  // The sequence is replayed as a graph while the ring grows (set by enqueue_graph for G_SAMPLED, nowhere else): the staging and priority
  // launchers take the kernel instances that read what varies from device memory (prio_kernels.h: the graph forms)
  bool graph_form = false;
  // a temperature step deferred into the next update's trunk launch ...
  AlphaArgs alpha{}; bool alpha_pending = false;
  bool alpha_tick_owed = false;   // ... across an ITERATION boundary (period graphs): its counter tick is owed until the next critic update's last kernel
  // node registry (sactd3_time_nodes, see node_on)
  int node_seq = 0, node_only = -1;
  std::vector<NodeInfo>* node_log = nullptr;
};
// where every sequence ends: nothing deferred may be left over (it would never run)
static int enqueue_end(EnqCtx& x, int rc) {
  return (rc == 0 && (x.alpha_pending || x.alpha_tick_owed)) ? x.e->fail(SACTD3_ESTATE, "enqueue: a deferred temperature step was left over") : rc;
}
// Every kernel launch of the update path is numbered here (EnqCtx::node_seq); with node_only >= 0 only that launch is issued (the
// others are skipped), with node_log set the launch's name and algorithmic FLOPs / bytes are recorded.  flops = 2 x MACs of the GEMMs
// the launch contains (SURVEY.md 8d counts GEMM FLOPs only); bytes = the operands it has to read and the results it has
// to write, each counted once (what a perfect cache hierarchy would move).
// `name` = "<kernel instance as rocprofv3 prints it, without blanks>[.detail]"; logged as "instance:role[/detail]" with
// the launch's total thread count (what rocprofv3 calls Grid_Size), so that a profile row can be matched to a node.
static inline bool node_on(EnqCtx& x, const char* name, double flops, double bytes, dim3 grid, dim3 block) {
  if (x.node_only < 0 && !x.node_log) return true;      // the normal case: not being timed
  const int k = x.node_seq++;
  if (x.node_log) {
    std::string n(name), detail;
    const size_t dot = n.find('.');
    if (dot != std::string::npos) { detail = "/" + n.substr(dot + 1); n.resize(dot); }
    x.node_log->push_back(NodeInfo{n + ":" + x.role + detail, flops, bytes,
                                    (long)grid.x * grid.y * grid.z * block.x * block.y * block.z});
  }
  return x.node_only < 0 || x.node_only == k;
}
// THE launch: on the sequence's stream, with the one error check.  Every launch of the file goes through it (the launch_nt_* / launch_k_*
// helpers aside, which are handed x.s) -- the feature layer plainly: its launches are not nodes of the registry ...
#define LAUNCH_ON(kernel, grid, block, ...)                                 \
  do {                                                                      \
    hipLaunchKernelGGL(kernel, grid, block, 0, x.s, __VA_ARGS__);           \
    const hipError_t _he = hipGetLastError();                               \
    if (_he != hipSuccess) return x.e->fail(SACTD3_EHIP, "hipGetLastError()", _he); \
  } while (0)
// ... and the update path as a numbered node
#define LAUNCH(name, flops, bytes, kernel, grid, block, ...)                 \
  do {                                                                      \
    if (node_on(x, name, flops, bytes, grid, block)) LAUNCH_ON(kernel, grid, block, __VA_ARGS__); \
  } while (0)
// the two single-thread launches that many sequences end or begin with: a counter tick, two adjacent device words set
static int launch_tick(EnqCtx& x, int* ctr) {
  LAUNCH_ON(k_tick, dim3(1), dim3(1), ctr, (int*)nullptr);
  return 0;
}
static int launch_set_int2(EnqCtx& x, int* dst, int v0, int v1) {
  LAUNCH_ON(k_set_int2, dim3(1), dim3(1), dst, v0, v1);
  return 0;
}

static inline dim3 tile_grid(int tiles, int nets) { return dim3((unsigned)((tiles + 3) / 4), 1, (unsigned)nets); }
// blocks of 256 threads at `cpt` chunks per thread
static inline unsigned cpt_blocks(long chunks, int cpt) { return (unsigned)((chunks + 256L * cpt - 1) / (256L * cpt)); }

// one float4 chunk per thread while that still fills the chip; GATHER_CPT chunks (loads in flight) per thread beyond
static unsigned gather_blocks(long chunks) {
  const long one = (chunks + 255) / 256;
  return one <= 4096 ? (unsigned)one : cpt_blocks(chunks, GATHER_CPT);
}
static GatherArgs gather_args(sactd3_engine* e, const float* ring, int identity_len, int slot = 0, int ctr_add = 0) {
  GatherArgs g{};
  const sactd3_engine::BatchSlot& S = e->bs[slot];
  g.ring = (const float4*)ring; g.rec4 = e->rec4; g.cx = e->cx; g.cn = e->cn; g.ctl = e->ctl; g.idx = S.idx;
  g.X = (float4*)S.X; g.Xn = (float4*)S.Xn; g.rew = S.rew; g.done = S.done;
  g.B = e->B; g.len_override = identity_len; g.ctr_add = ctr_add;
  g.rec4_magic = magic_div((unsigned)e->rec4, (unsigned long long)e->B * e->rec4 + 1);
  const long chunks = (long)e->B * e->rec4;
  g.cpb = (int)((chunks + 256L * gather_blocks(chunks) - 1) / (256L * gather_blocks(chunks)));
  return g;
}
template <int PRO, bool F1, int C1>
static void launch_nt_ks(hipStream_t s, int ks, dim3 grid, const NtArgs& g) {      // ks = 2 or 4
  if (ks == 4) launch_k_nt(k_nt<PRO, F1, 4, C1>, grid, s, g);
  else launch_k_nt(k_nt<PRO, F1, 2, C1>, grid, s, g);
}
template <int PRO>
static void launch_nt_f1(hipStream_t s, int ks, int nt, dim3 grid, const NtArgs& g) {
  const int c1 = (g.K1 + 15) / 16;
  if (nt == 2) {   // (KS == 2 only) two column tiles per block
    if (c1 <= 1) launch_k_nt(k_nt<PRO, true, 2, 1, 2>, grid, s, g);
    else if (c1 == 2) launch_k_nt(k_nt<PRO, true, 2, 2, 2>, grid, s, g);
    else launch_k_nt(k_nt<PRO, true, 2, 4, 2>, grid, s, g);
    return;
  }
  if (c1 <= 1) launch_nt_ks<PRO, true, 1>(s, ks, grid, g);
  else if (c1 == 2) launch_nt_ks<PRO, true, 2>(s, ks, grid, g);
  else launch_nt_ks<PRO, true, 4>(s, ks, grid, g);
}
static void launch_nt_c4(hipStream_t s, int nt, dim3 grid, const NtArgs& g) {      // (LayerNorm form, fused first layer, KS = 2 with KS = 4's sums)
  const int c1 = (g.K1 + 15) / 16;
  if (nt == 2) {
    if (c1 <= 1) launch_k_nt(k_nt<1, true, 2, 1, 2, true>, grid, s, g);
    else if (c1 == 2) launch_k_nt(k_nt<1, true, 2, 2, 2, true>, grid, s, g);
    else launch_k_nt(k_nt<1, true, 2, 4, 2, true>, grid, s, g);
  } else {
    if (c1 <= 1) launch_k_nt(k_nt<1, true, 2, 1, 1, true>, grid, s, g);
    else if (c1 == 2) launch_k_nt(k_nt<1, true, 2, 2, 1, true>, grid, s, g);
    else launch_k_nt(k_nt<1, true, 2, 4, 1, true>, grid, s, g);
  }
}
// XCD row groups for xcd_tile (kernels.h) of an R x C tile grid whose row operand is A bytes and column operand W bytes: the
// split xr x xc = 8 with the least total fetch xc A + xr W among those that divide the grid; 0 = keep row-major numbering.
static int pick_xr(int R, int C, double A, double W) {
  int best = 0; double cost = 1e300;
  for (int xr = 1; xr <= 8; xr *= 2) {
    const int xc = 8 / xr;
    if (R % xr || C % xc) continue;
    const double c = xc * A + xr * W;
    if (c < cost) { cost = c; best = xr; }
  }
  return best;
}
// pro == 0: the generic-K form (unfused first layer).  Otherwise K == 256 and the block shape (16 / 32 / 64 rows x 16
// columns) is chosen so that the launch has about one block per CU.
static int launch_nt(EnqCtx& x, const char* name, int pro, bool fuse1, const NtArgs& g, int nets, int force_ks = 0) {
  sactd3_engine* e = x.e;
  const hipStream_t s = x.s;
  const int tiles_m = (g.M + 15) / 16, tiles_n = (g.N + 15) / 16;
  // algorithmic work: the (fused) first layer + this layer; operands: input rows, the weight blocks, the output (+ stored activations)
  const double fl = 2.0 * nets * (double)g.M * g.N * (g.K + (fuse1 ? g.K1 : 0));
  double by = 4.0 * ((double)nets * g.N * (g.K + 3) + (double)nets * g.M * g.N);
  by += fuse1 ? 4.0 * ((double)nets * HID * (g.K1 + 1) + (double)(nets / g.npg) * g.M * g.K1) : 4.0 * (double)nets * g.M * g.K;
  for (int i = 0; i < nets / g.npg; ++i) by += 4.0 * g.npg * (double)g.M * HID * ((g.g[i].xh_out ? 1 : 0) + (g.g[i].h_out ? 1 : 0));
  if (g.gblocks) by += (g.gblocks / std::max(g.gb_each, 1)) * 8.0 * (double)g.ga[0].B * 4 * (g.ga[0].cx + g.ga[0].cn + 1);
  if (pro == 0) {
    const dim3 grid((unsigned)(tiles_m * tiles_n), 1, (unsigned)nets);
    LAUNCH("k_nt_wide.layer1", fl, by, k_nt_wide, grid, dim3(256), g);
  } else {
    const int tiles = tiles_m * tiles_n * nets;
    int ks = tiles >= 2 * e->num_cus ? 2 : 4;   // measured on 256 .. 4096-tile launches (KS = 1 never won)
    if (force_ks) ks = force_ks;
    // a launch that must reproduce the KS = 4 sums (force_ks: the run-ahead passes of a period graph) but holds several groups: 32-row
    // blocks with the KS = 4 summation tree (k_nt's C4 form) -- half as many blocks fetch W1 and their W2 tile
    const bool c4 = force_ks == 4 && fuse1 && pro == 1 && tiles >= 2 * e->num_cus;
    if (c4) ks = 2;
    const int rb = 64 / ks;
    // two column tiles per block when the launch would otherwise put two rounds of blocks on every CU: the fused first
    // layer is then recomputed (or the A rows fetched and normalised) by half as many blocks
    int nt = (ks == 2 && ((g.M + rb - 1) / rb) * tiles_n * nets >= 2 * e->num_cus && tiles_n % 2 == 0) ? 2 : 1;
    if (force_ks && !c4) nt = 1;
    // (C4: two column tiles per block only when that leaves at most one block per CU: 4 groups -> 256 blocks; 5 groups would be 320,
    //  a quarter of the CUs with two -- they take 640 single-tile blocks instead)
    if (c4 && nt == 2 && ((g.M + rb - 1) / rb) * (tiles_n / 2) * nets > e->num_cus) nt = 1;
    NtArgs gg = g;
    gg.nt_blocks = ((g.M + rb - 1) / rb) * (tiles_n / nt);
    if (!gg.ga[0].ctl) gg.ga[0].ctl = e->ctl;      // (the launch header hands it to every block: k_nt reads the ring's control words through it before it knows its group)
    // unfused launches read whole input rows: place the tiles so that an XCD pulls few rows and few weight columns (the fused
    // form's input rows are a few dozen bytes: it keeps one weight column tile per XCD, the row-major numbering)
    gg.xr = fuse1 ? 0 : pick_xr((g.M + rb - 1) / rb, tiles_n / nt, 4.0 * g.M * g.K, 4.0 * g.N * g.K);
    int nzb = 0;
    for (int i = 0; i < gg.nz_n && i < 5; ++i) nzb += gg.nz[i].blocks;
    const int riders = gg.gblocks + gg.alpha_block + nzb;
    // (see NtArgs::flat; with many riders -- the run-ahead launches' gathers and noise blocks -- the 3-D grid's order, net 0's tiles,
    //  the riders, then the other nets' tiles, measured 0.3 us per TD3 iteration better; TD3's 4-net critic trunk, one block per CU by
    //  its LDS, with its 1-3 noise riders: 0.5 us better in the 3-D grid too)
    gg.flat = (nets > 1 && gg.alpha_block && riders <= 8) ? nets : 0;      // (the critic trunk that carries a deferred temperature step)
    gg.flat_r = gg.flat ? (riders + 7) & ~7 : 0; gg.flat_n = riders;
    const dim3 grid = gg.flat ? dim3((unsigned)(gg.nt_blocks * nets + gg.flat_r)) : dim3((unsigned)(gg.nt_blocks + riders), 1, (unsigned)nets);
    char inst[64] = "k_nt";
    if (x.node_log) {
      const int c1 = (g.K1 + 15) / 16;
      snprintf(inst, sizeof(inst), c4 ? "k_nt<%d,%s,%d,%d,%d,true>.%s" : "k_nt<%d,%s,%d,%d,%d>.%s", pro, fuse1 ? "true" : "false", ks, fuse1 ? (c1 <= 1 ? 1 : (c1 == 2 ? 2 : 4)) : 0, nt, name);
    }
    if (!node_on(x, inst, fl, by, grid, dim3(256))) return 0;
    if (c4) launch_nt_c4(s, nt, grid, gg);
    else if (fuse1) { if (pro == 1) launch_nt_f1<1>(s, ks, nt, grid, gg); else launch_nt_f1<2>(s, ks, nt, grid, gg); }
    else if (nt == 2) {   // (KS == 2) the A rows are fetched and normalised by half as many blocks
      if (pro == 1) launch_k_nt(k_nt<1, false, 2, 0, 2>, grid, s, gg);
      else launch_k_nt(k_nt<2, false, 2, 0, 2>, grid, s, gg);
    } else { if (pro == 1) launch_nt_ks<1, false, 0>(s, ks, grid, gg); else launch_nt_ks<2, false, 0>(s, ks, grid, gg); }
  }
  HIPCHK(hipGetLastError());
  return 0;
}
static int launch_nn(EnqCtx& x, const char* name, const NnArgs& g, int nets) {
  if (g.M >= BIG_BATCH && g.Kout == HID && g.k_off == 0) {   // large batch: LDS-tiled form, ~1 block per CU
    const double fl = 2.0 * nets * (double)g.M * HID * HID, by = 4.0 * nets * (2.0 * g.M * HID + (double)HID * HID);
    if (nets >= 2) {
      const dim3 grid((unsigned)(((g.M + 31) / 32) * (HID / 64) * nets));
      LAUNCH("k_nn64<2,2,2>.dh1", fl, by, (k_nn64<2, 2, 2>), grid, dim3(256), g);
    } else {
      const dim3 grid((unsigned)(((g.M + 31) / 32) * (HID / 32) * nets));
      LAUNCH("k_nn64<2,2,1>.dh1", fl, by, (k_nn64<2, 2, 1>), grid, dim3(256), g);
    }
    (void)name;
    return 0;
  }
  const dim3 grid((unsigned)(((g.M + 15) / 16) * ((g.Kout + 15) / 16)), 1, (unsigned)nets);
  NnArgs gg = g;
  gg.xr = pick_xr((g.M + 15) / 16, (g.Kout + 15) / 16, 4.0 * g.M * HID, 4.0 * HID * g.Kout);
  LAUNCH(name, 2.0 * nets * (double)g.M * HID * g.Kout, 4.0 * nets * ((double)g.M * HID + (double)HID * g.Kout + (double)g.M * g.Kout),
         k_nn, grid, dim3(256), gg);
  return 0;
}
// block tile / chunk rows of the large-batch weight-gradient GEMM (must agree with the k_tn64 instance launched)
#ifndef TN64_CFG
#define TN64_CFG 2, 2, 2, 1, 64      /* 64 (n) x 32 (k) tile, 64-row chunks: the fastest of tools/kprobe_tn64.hip's shapes */
#define TN64_N 64
#define TN64_K 32
#define TN64_M 64
#endif
#define TN64_KERNEL (k_tn64<TN64_CFG>)
// What is not a GEMM tile of a weight-gradient launch: the vector finalisations of its problems, the optimiser step (+ Polyak), the
// loss and the counter tick -- k_adam_red's arguments in the split-M form, the riding blocks' in k_tn (see TnArgs::fin)
static AdamRedArgs adam_red_args(const TnArgs& g, int nets, long g_ns, int tick_extra) {
  AdamRedArgs r{};
  r.s_off = -1;
  for (int i = 0; i < g.nprob; ++i) {
    const TnProb& q = g.pr[i];
    for (int f = 0; f < q.nfin; ++f) { r.vec[r.nvec].off = q.fin_off[f]; r.vec[r.nvec].slot = q.fin_slot[f]; r.vec[r.nvec].nblk = q.fin_nblk[f]; ++r.nvec; }
    if (q.fin_s_off >= 0) { r.s_off = q.fin_s_off; r.s_nblk = q.fin_s_nblk; }
  }
  r.nets = nets; r.g_ns = g_ns; r.G = g.G; r.keep_g = g.keep_g;
  r.apply = g.apply; r.P = g.P; r.Mo = g.Mo; r.Vo = g.Vo; r.T = g.T; r.tau = g.tau; r.adam = g.adam; r.b1 = g.b1; r.b2 = g.b2; r.eps = g.eps;
  r.T2 = g.T2; r.T3 = g.T3;      // (never set on the split-M route: actor_dw_is_tiled64)
  r.part = g.part; r.pstride = g.pstride; r.part_s = g.part_s;
  r.loss_part = g.loss_part; r.loss_n = g.loss_n; r.loss_stride = g.loss_stride; r.loss_off = g.loss_off; r.loss_scale = g.loss_scale;
  r.loss_dst = g.loss_dst; r.tick = g.tick; r.tick_extra = tick_extra;
  return r;
}
// Large batches: split-M GEMM into partial slabs (k_tn64) + slab sum / vector gradients / Adam / Polyak (k_adam_red).
// (called by launch_tn, which has set g.keep_g)
static int launch_tn64(EnqCtx& x, const char* name, const TnArgs& g, int nets, int tick_extra = 0, const BcFin* bf = nullptr) {
  sactd3_engine* e = x.e;
  Tn64Args a{};
  a.nprob = g.nprob; a.M = g.M; a.nets = nets; a.Gp = e->Gp; a.g_ns = nets > 1 ? g.g_ns : (long)e->La.size;
  int tiles = 0;
  double fl = 0.0, by = 0.0;
  for (int i = 0; i < g.nprob; ++i) {
    const TnProb& q = g.pr[i];
    Tn64Prob& t = a.pr[i];
    t.dY = q.dY; t.ldy = q.ldy; t.dy_ns = q.dy_ns; t.N = q.N; t.X = q.X; t.ldx = q.ldx; t.x_ns = q.x_ns; t.K = q.K;
    t.w_off = q.w_off; t.ldw = q.ldw; t.b_off = q.b_off;
    t.tiles_n = (q.N + TN64_N - 1) / TN64_N; t.tiles_k = (q.ldw + TN64_K - 1) / TN64_K; t.tile0 = tiles;
    tiles += t.tiles_n * t.tiles_k;
    fl += 2.0 * nets * (double)g.M * q.N * q.K;
    by += 4.0 * nets * (double)g.M * (q.N + q.K);
  }
  a.tiles_per_net = tiles;
  const int nch = (g.M + TN64_M - 1) / TN64_M;
  // slices: about two blocks per CU, all of (nearly) the same length
  int S = (2 * e->num_cus + tiles * nets / 2) / (tiles * nets);
  S = std::max(1, std::min(S, std::min(e->gp_slabs, nch)));
  a.S = S;
  const long size = a.g_ns;
  {
    const dim3 grid((unsigned)(tiles * nets * S));
    char inst[96];
    snprintf(inst, sizeof(inst), "k_tn64<2,2,2,1,64>.dW(split-M x%d)", S);   // (instance = TN64_CFG: the name rocprofv3 reports)
    LAUNCH(inst, fl, by + 4.0 * S * nets * (double)size, TN64_KERNEL, grid, dim3(256), a);
  }
  AdamRedArgs r = adam_red_args(g, nets, size, tick_extra);
  r.Gp = e->Gp; r.S = S;
  const dim3 grid((unsigned)((size / 4 + 255) / 256 + 4 * r.nvec + 1), (unsigned)nets);
  const char* rname = g.apply ? (g.T ? "k_adam_red.sum+adam+polyak" : "k_adam_red.sum+adam") : "k_adam_red.sum";
  const double rbytes = nets * (double)size * (4.0 * S + 4.0 + (g.apply ? 24.0 : 0.0) + (g.apply && g.T ? 8.0 : 0.0));
  if (bf) {      // TD3+BC: the instance whose last tail block finalises the BC loss
    const char* bname = g.apply ? (g.T ? "k_adam_red_bc.sum+adam+polyak" : "k_adam_red_bc.sum+adam") : "k_adam_red_bc.sum";
    if (r.keep_g) LAUNCH(bname, 0.0, rbytes, k_adam_red_bc<true>, grid, dim3(256), r, *bf);
    else LAUNCH(bname, 0.0, rbytes, k_adam_red_bc<false>, grid, dim3(256), r, *bf);
  } else if (r.keep_g) LAUNCH(rname, 0.0, rbytes, k_adam_red<true>, grid, dim3(256), r);
  else LAUNCH(rname, 0.0, rbytes, k_adam_red<false>, grid, dim3(256), r);
  (void)name;
  return 0;
}

static inline int tn_width(const TnProb& q) { return q.kw > 0 ? q.kw : q.ldw; }
// The split-M form pays an extra node (k_adam_red): taken at large batch when the launch has enough 64 x 32 tiles (over all of its
// nets) to fill the chip with long slices (the critics' 168 at Humanoid: 25.6 -> 18.6 us); the actor's 88 tiles gain nothing (14.3
// vs 14.4 us)
static bool tn_is_tiled64(const sactd3_engine* e, int M, int tiles64) { return M >= BIG_BATCH && e->Gp && tiles64 >= e->num_cus / 2; }
static inline int tn64_tiles(int N, int ldw) { return ((N + TN64_N - 1) / TN64_N) * ((ldw + TN64_K - 1) / TN64_K); }
// bf != nullptr (TD3+BC actor launch): the k_tn_bc / k_adam_red_bc instances; g.loss_dst is NULL then, BcFin names the slots
static int launch_tn(EnqCtx& x, const char* name, TnArgs& g, int nets, int tick_extra = 0, const BcFin* bf = nullptr) {
  sactd3_engine* e = x.e;
  const hipStream_t s = x.s;
  g.keep_g = !(x.lean_stores && g.apply);      // (see sactd3_engine::grads_stale)
  if (!g.keep_g) for (int i = 0; i < g.nprob; ++i) g.pr[i].f_dz = nullptr;
  {
    int tiles = 0;
    for (int i = 0; i < g.nprob; ++i) tiles += tn64_tiles(g.pr[i].N, g.pr[i].ldw);
    if (tn_is_tiled64(e, g.M, tiles * nets)) return launch_tn64(x, name, g, nets, tick_extra, bf);
  }
  auto count = [&](int kt) {
    int tiles = 0;
    for (int i = 0; i < g.nprob; ++i) {
      g.pr[i].tile0 = tiles;
      tiles += ((g.pr[i].N + 15) / 16) * (((tn_width(g.pr[i]) + 15) / 16 + kt - 1) / kt);
    }
    return tiles;
  };
  // two k tiles per block (one dY slice fetched and transposed for both) once single tiles would be more than two blocks per CU
  // (the critics' launch at B = 256: 544 blocks -> 288, -0.6 us per iteration)
  int kt = (count(1) * nets > 2 * e->num_cus && g.M < BIG_BATCH) ? 2 : 1;   // (measured: no gain with a thousand rows per tile)
  const int tiles = count(kt);
  for (int i = 0; i < g.nprob; ++i)      // n tiles need dY columns, k tiles X columns (both M rows long)
    g.pr[i].xr = g.pr[i].xr_force ? g.pr[i].xr_force
                                  : pick_xr((g.pr[i].N + 15) / 16, ((tn_width(g.pr[i]) + 15) / 16 + kt - 1) / kt, 4.0 * g.M * g.pr[i].N, 4.0 * g.M * tn_width(g.pr[i]));
  // dW = dY^T X of every problem; operands dY, X once each; the weight block's gradient written, and with the fused
  // optimiser step p, m, v read and written (+ the Polyak target): 4 (g) + 24 (Adam) + 8 (Polyak) bytes per parameter
  double fl = 0.0, by = 0.0;
  for (int i = 0; i < g.nprob; ++i) {
    fl += 2.0 * nets * (double)g.M * g.pr[i].N * g.pr[i].K;
    by += 4.0 * nets * (double)g.M * ((g.pr[i].x_dup == 2 ? 0 : g.pr[i].N) + (g.pr[i].x_dup == 1 ? 0 : g.pr[i].K)) + (4.0 + (g.apply ? 24.0 : 0.0) + (g.apply && g.T ? 8.0 : 0.0)) * nets * (double)g.pr[i].N * (g.pr[i].K + 1);
  }
  bool fold = false;
  for (int i = 0; i < g.nprob; ++i) fold = fold || g.pr[i].fold;
  char inst[96];
  if (bf) snprintf(inst, sizeof(inst), fold ? "k_tn_bc<%d,true>.%s" : "k_tn_bc<%d>.%s", kt, name);
  else snprintf(inst, sizeof(inst), fold ? "k_tn<%d,true>.%s" : "k_tn<%d>.%s", kt, name);
  g.tiles = tiles;
  if (g.pk_blocks) by += 12.0 * (g.pk.n0 + g.pk.n1);
  g.fin = adam_red_args(g, nets, g.g_ns, tick_extra);      // what is not a GEMM tile goes to riding blocks (see TnArgs::fin)
  g.fin_blocks = 4 * g.fin.nvec + 1;
  const dim3 grid((unsigned)((tiles + g.pk_blocks + g.fin_blocks + (nets > 1 ? 7 : 0)) & (nets > 1 ? ~7 : ~0)), 1, (unsigned)nets);
  if (!node_on(x, inst, fl, by, grid, dim3(256))) return 0;
  if (bf) {
    if (g.keep_g) {
      if (fold) {
        if (kt == 2) launch_k_tn_bc<2, true, true>(grid, s, g, *bf);
        else launch_k_tn_bc<1, true, true>(grid, s, g, *bf);
      } else if (kt == 2) launch_k_tn_bc<2, false, true>(grid, s, g, *bf);
      else launch_k_tn_bc<1, false, true>(grid, s, g, *bf);
    } else if (fold) {
      if (kt == 2) launch_k_tn_bc<2, true, false>(grid, s, g, *bf);
      else launch_k_tn_bc<1, true, false>(grid, s, g, *bf);
    } else if (kt == 2) launch_k_tn_bc<2, false, false>(grid, s, g, *bf);
    else launch_k_tn_bc<1, false, false>(grid, s, g, *bf);
  } else if (g.keep_g) {
    if (fold) {
      if (kt == 2) launch_k_tn<2, true, true>(grid, s, g);
      else launch_k_tn<1, true, true>(grid, s, g);
    } else if (kt == 2) launch_k_tn<2, false, true>(grid, s, g);
    else launch_k_tn<1, false, true>(grid, s, g);
  } else if (fold) {      // the instances without the gradient-arena stores (TnArgs::keep_g)
    if (kt == 2) launch_k_tn<2, true, false>(grid, s, g);
    else launch_k_tn<1, true, false>(grid, s, g);
  } else if (kt == 2) launch_k_tn<2, false, false>(grid, s, g);
  else launch_k_tn<1, false, false>(grid, s, g);
  HIPCHK(hipGetLastError());
  return 0;
}
static TnProb tn_prob(const float* dY, int ldy, long dy_ns, int N, const float* X, int ldx, long x_ns, int K,
                      int w_off, int ldw, int b_off) {
  TnProb q{};
  q.dY = dY; q.ldy = ldy; q.dy_ns = dy_ns; q.N = N; q.X = X; q.ldx = ldx; q.x_ns = x_ns; q.K = K;
  q.w_off = w_off; q.ldw = ldw; q.b_off = b_off; q.nfin = 0; q.fin_s_off = -1;
  return q;
}
// Rows [n_lo, n_lo + n) of a weight-gradient problem as a problem of its own (the same GEMM, cut along dW's rows).  A launch with a
// folded layer-1 problem puts it BETWEEN two such pieces of the W2 problem: a launch of 300 blocks gives the first ~50 CUs a second
// block (ids 256 ..), and the folded blocks -- 80 KB of operands, the launch's long pole -- must not be among the first ~50 ids (the
// critics' net-0 ones were: 6.8 us against net 1's 6.1, tools/blocks_probe.py).  Vector finalisations stay with the first piece.
static TnProb tn_rows(const TnProb& q, int n_lo, int n) {
  TnProb r = q;
  r.dY = q.dY + n_lo; r.N = n; r.w_off = q.w_off + n_lo * q.ldw; r.b_off = q.b_off >= 0 ? q.b_off + n_lo : -1;
  if (n_lo) { r.nfin = 0; r.fin_s_off = -1; r.x_dup = 1; }
  return r;
}
// Columns [k_lo, k_lo + k) of a weight-gradient problem as a problem of its own (cut along dW's COLUMNS: every piece has all of the
// rows).  With xr_force = 8 the 8 XCDs each own two 16-row tiles of a piece -- the rows of W2 (and of its Polyak target) that the
// next trunk launch reads on that very XCD (its column tile t = rows 32 t .. 32 t + 31 sits on XCD t mod 8): the optimiser epilogue
// leaves them in the L2 that will want them.
static TnProb tn_cols(const TnProb& q, int k_lo, int k) {
  TnProb r = q;
  r.X = q.X + k_lo; r.K = k; r.kw = k; r.w_off = q.w_off + k_lo;
  if (k_lo) { r.b_off = -1; r.nfin = 0; r.fin_s_off = -1; r.x_dup = 2; }
  return r;
}
static void tn_fin(TnProb& q, int slot, int off, int nblk) { q.fin_slot[q.nfin] = slot; q.fin_off[q.nfin] = off; q.fin_nblk[q.nfin++] = nblk; }
// The layer-1 problem with the layer's LayerNorm backward folded in (TnProb::fold): L = the net's layout, ps = the row-sum partials
// that the launch in front left, with its gamma1 snapshot g behind them (fold_args); dz: where dz1 goes for inspection
static void tn_fold(TnProb& q, int ln, const NetLayout& L, const float* xh, const float* rstd, const float* ps, float* dz, const float* g) {
  q.fold = 1; q.f_ln = ln; q.f_g_off = L.g1; q.f_be_off = L.be1; q.f_xh = xh; q.f_rstd = rstd; q.f_ps = ps; q.f_dz = dz; q.f_g = g;
}
// ... and what the fused tail + dh1 launch in front of it is told (NnFold): the partials and the snapshot it leaves for tn_fold
static NnFold fold_args(bool fold, int ln, const NetLayout& L, const float* h1, const float* xh1, float* ps, float* gsnap) {
  NnFold f{};
  f.fold = fold; f.ln = ln; f.h1 = h1; f.xh1 = xh1; f.g1_off = L.g1; f.ps = ps; f.gsnap = gsnap;
  return f;
}
// dh1 = dz2 W2 of nets that lie ns floats apart in dz2 / dh1 and p_ns floats apart in the parameter arena holding W2
static NnArgs dh1_args(const float* dz2, const float* W2, float* dh1, int M, long ns, long p_ns) {
  NnArgs g{};
  g.dY = dz2; g.dy_ns = ns; g.Wt = W2; g.ldw = HID; g.p_ns = p_ns; g.k_off = 0;
  g.dX = dh1; g.ldx = HID; g.dx_ns = ns; g.M = M; g.Kout = HID;
  return g;
}
// layer 1's LayerNorm backward as a launch of its own: dz1 from dh1 and the forward pass's stores (gamma: the first net's gamma1)
static LnBwd ln_bwd_args(const sactd3_engine* e, const float* dh, const float* xh, const float* h, const float* rstd,
                         const float* gamma, long p_ns, int want_part, float* dz) {
  LnBwd l{};
  l.dh = dh; l.xh = xh; l.h = h; l.rstd = rstd; l.gamma = gamma; l.p_ns = p_ns;
  l.B = e->B; l.ln = e->cfg.layer_norm; l.want_part = want_part; l.dz = dz; l.part = e->part; l.pstride = e->nblk4;
  return l;
}
// what the two launches around a folded dQ/da agree on (QaFold of k_qtail_nn, QaIn of k_headbwd_nn): the partials' shape and place
template <class Qa>
static void qa_fold_args(Qa& q, const sactd3_engine* e) {
  q.on = 1; q.ln = e->cfg.layer_norm; q.a = e->a; q.pqw = e->a <= 3 ? 8 : 16; q.ntile = HID / (e->nq_actor == 2 ? 32 : 16);
  q.ps = e->qa_ps; q.S = e->qa_S;
}

// The two hidden layers of MLP trunks: z2 = relu(LN(x W1^T + b1)) W2^T + b2 for up to two groups of nets
// (a group = nets sharing an input and a parameter arena) in ONE launch.  One kernel when the input is narrow
// (first layer recomputed per output tile), two otherwise.  Optional stores of layer 1's xhat / h / rstd.
// ring: the group's rows are read from the replay ring (field offset ring_off) -- the sample drawn with sample_ctr + sctr_add
struct TrunkGrp { const float* x; const float* P; float* z1; float* z2; float* xh; float* h; float* rstd; int ring_off = 0;
                  bool ring = false; int sctr_add = 0; const int* ring_idx = nullptr; };
struct TrunkTicks { int* tick0; int* tick1; float* adam_out; double* adam_pw; float lr;
                    int ngather = 0; GatherArgs gather[3] = {};   // replay gathers into batch slots riding as extra blocks (launches with ring groups)
                    const AlphaArgs* alpha = nullptr;      // alpha: a pending temperature step to carry as one extra block
                    int nnoise = 0; NoiseJob noise[5] = {}; bool* noise_taken = nullptr;      // the following tails' draws (see NoiseJob)
                    int force_ks = 0;                      // keep the single-net launch's K split (bit-equal results across launch shapes)
                    bool no_tiled64 = false;               // keep the 32 x 32-tile launches (the ones that can read ring rows / carry gathers)
                    bool pin_shape = false;                // scoring (sactd3_qvalues_device): a row's bits must not depend on M -- the KS = 4 sums in both
                                                           // k_nt launches (fused, and the unfused layer 2), no large-batch form even when M == B
                    int* tick0b = nullptr; float* adam_out_b = nullptr; double* adam_pw_b = nullptr; float lr_b = 0.f; };   // a second step counter
static int enqueue_trunk(EnqCtx& x, int ldx, int K, int M, const NetLayout& L, long p_ns,
                         int ngrp, int npg, const TrunkGrp* grp, TrunkTicks tk) {
  sactd3_engine* e = x.e;
  const int pro = e->cfg.layer_norm ? 1 : 2;
  NtArgs h{};
  h.npg = npg; h.oW = L.W2; h.ldw = HID; h.oBias = L.b2; h.oG = L.g1; h.oBe = L.be1; h.p_ns = p_ns;
  h.ldy = HID; h.y_ns = (long)M * HID; h.M = M; h.N = HID; h.K = HID; h.act_ns = (long)M * HID;
  for (int i = 0; i < ngrp; ++i) {
    h.g[i].P = grp[i].P; h.g[i].Y = grp[i].z2; h.g[i].xh_out = grp[i].xh; h.g[i].h_out = grp[i].h; h.g[i].rstd_out = grp[i].rstd;
  }
  const int nets = ngrp * npg;
  const bool big_m = M >= BIG_BATCH && M == e->B && !tk.pin_shape;
  const bool big_path = big_m && ((M + 63) / 64) * (HID / 64) * nets >= (3 * e->num_cus) / 4 && !tk.no_tiled64;
  auto set_ring = [&](NtArgs& a) {   // which groups read their rows from the replay ring, and the gathers that ride along
    for (int i = 0; i < ngrp; ++i) { a.g[i].ring = grp[i].ring ? 1 : 0; a.g[i].ring_off = grp[i].ring_off; a.g[i].sctr_add = grp[i].sctr_add; a.g[i].ring_idx = grp[i].ring_idx; }
    a.ga[0] = gather_args(e, e->ring, -1);                                     // (ring groups take the ring / control block from ga[0])
    for (int i = 0; i < tk.ngather && i < 3; ++i) a.ga[i] = tk.gather[i];
    a.gb_each = tk.ngather > 0 ? (int)gather_blocks((long)e->B * e->rec4) : 0;
    a.gblocks = tk.ngather * a.gb_each;
  };
  auto set_noise = [&](NtArgs& a) {  // the draws of the tail(s) that follow ride in this launch as a few extra blocks
    if (tk.nnoise <= 0) return;
    a.nz_n = tk.nnoise; a.nz_ctl = e->ctl;
    for (int i = 0; i < tk.nnoise; ++i) { a.nz[i] = tk.noise[i]; a.nz[i].blocks = (tk.noise[i].n + 1023) / 1024; }
    if (tk.noise_taken) *tk.noise_taken = true;
  };
  // the first layer as a launch of its own (every form but the fused one of narrow inputs); it makes the ticks
  NtArgs g{};
  g.npg = npg; g.oW = L.W1; g.ldw = L.ld1; g.oBias = L.b1; g.p_ns = p_ns; g.ld_in = ldx; g.in_ns = 0;
  g.ldy = HID; g.y_ns = (long)M * HID; g.M = M; g.N = HID; g.K = K;
  for (int i = 0; i < ngrp; ++i) { g.g[i].in = grp[i].x; g.g[i].P = grp[i].P; g.g[i].Y = grp[i].z1; }
  g.tick0 = tk.tick0; g.tick1 = tk.tick1; g.adam_out = tk.adam_out; g.adam_pw = tk.adam_pw; g.lr = tk.lr; g.b1 = e->cfg.adam_beta1; g.b2 = e->cfg.adam_beta2;
  g.tick0b = tk.tick0b; g.adam_out_b = tk.adam_out_b; g.adam_pw_b = tk.adam_pw_b; g.lr_b = tk.lr_b;
  double st = 0.0;   // rows the large-batch layer-2 launches write besides the output: h and xhat where the caller keeps them
  for (int i = 0; i < ngrp; ++i) st += ((grp[i].xh ? 1.0 : 0.0) + (grp[i].h ? 1.0 : 0.0)) / ngrp;
  // MFMA-bound sizes with enough 64 x 64 tiles to fill the chip: tiled GEMM -> tiled GEMM with the LayerNorm + ReLU prologue
  if (big_path) {
    const dim3 grid((unsigned)(((M + 63) / 64) * (HID / 64) * nets));
    const double by_w = 4.0 * nets * (double)HID, by_rows = 4.0 * nets * (double)M * HID;
    {   // a pending temperature step rides as one extra block of the first-layer launch (nothing in the trunk reads log_alpha)
      dim3 grid1 = grid;
      if (tk.alpha) { g.alpha_block = 1; g.al = *tk.alpha; g.nt_blocks = (int)grid.x; grid1.x += 1; }
      LAUNCH("k_nt64<4,2,2>.layer1", 2.0 * nets * (double)M * HID * K, by_w * (K + 1) + 4.0 * ngrp * (double)M * K + by_rows,
             (k_nt64<4, 2, 2>), grid1, dim3(512), g);
    }
    // second layer with the LayerNorm + ReLU of the first as its prologue (k_nt64_ln): no row kernel in between
    for (int i = 0; i < ngrp; ++i) h.g[i].in = grp[i].z1;
    h.ld_in = HID; h.in_ns = (long)M * HID; h.ln_pro = e->cfg.layer_norm ? 1 : 0;
    LAUNCH("k_nt64_ln<4,2,2>.layer2", 2.0 * nets * (double)M * HID * HID, by_w * (HID + 3) + by_rows * (2.0 + st), (k_nt64_ln<4, 2, 2>), grid, dim3(512), h);
    return 0;
  }
  // the k_nt forms and the 32 x 32-tiled one: the launch that holds layer 2 carries a pending temperature step as one extra block
  // (never together with noise blocks: those read the counter it ticks) and the following tail's draws as a few more
  if (tk.alpha) { h.alpha_block = 1; h.al = *tk.alpha; }
  set_noise(h);
  if (K <= 64) {
    for (int i = 0; i < ngrp; ++i) h.g[i].in = grp[i].x;
    h.ld_in = ldx; h.in_ns = 0; h.K1 = K; h.oW1 = L.W1; h.ldw1 = L.ld1; h.oB1 = L.b1;
    h.tick0 = tk.tick0; h.tick1 = tk.tick1; h.adam_out = tk.adam_out; h.adam_pw = tk.adam_pw; h.lr = tk.lr; h.b1 = e->cfg.adam_beta1; h.b2 = e->cfg.adam_beta2;
    h.w1_magic = magic_div((unsigned)L.ld1, 4u * HID * (unsigned)L.ld1);
    set_ring(h);            // x = a field of the sampled records; extra blocks fill the batch slot(s) (see NtArgs)
    h.tick0b = tk.tick0b; h.adam_out_b = tk.adam_out_b; h.adam_pw_b = tk.adam_pw_b; h.lr_b = tk.lr_b;
    return launch_nt(x, "layers1+2", pro, true, h, nets, tk.pin_shape ? 4 : tk.force_ks);
  }
  if (big_m) {   // large batch, too few nets for 64 x 64 tiles to fill the chip: 32 x 32 LDS-tiled form
    unsigned nblk = (unsigned)(((M + 31) / 32) * (HID / 32) * nets);
    set_ring(g);            // x = the field of the sampled records itself; extra blocks fill the batch slot(s) (as in the fused k_nt form)
    g.nt_blocks = (int)nblk;
    nblk += (unsigned)g.gblocks;
    const dim3 grid(nblk);
    LAUNCH("k_nt64<2,2,1>.layer1", 2.0 * nets * (double)M * HID * K, 4.0 * (nets * (double)HID * (K + 1) + ngrp * (double)M * K + nets * (double)M * HID),
           (k_nt64<2, 2, 1>), grid, dim3(256), g);
  } else RCCHK(launch_nt(x, "layer1", 0, false, g, nets));
  for (int i = 0; i < ngrp; ++i) h.g[i].in = grp[i].z1;
  h.ld_in = HID; h.in_ns = (long)M * HID;
  if (big_m) {   // large batch: the 32 x 32 LDS-tiled form with the LayerNorm prologue
    h.ln_pro = e->cfg.layer_norm ? 1 : 0;
    h.nt_blocks = ((M + 31) / 32) * (HID / 32) * nets;
    int nzb = 0;
    for (int i = 0; i < h.nz_n && i < 5; ++i) nzb += h.nz[i].blocks;
    LAUNCH("k_nt64_ln<2,2,1>.layer2", 2.0 * nets * (double)M * HID * HID, 4.0 * nets * ((double)HID * (HID + 3) + (double)M * HID * (2.0 + st)),
           (k_nt64_ln<2, 2, 1>), dim3((unsigned)(h.nt_blocks + h.alpha_block + nzb)), dim3(256), h);
    return 0;
  }
  return launch_nt(x, "layer2", pro, false, h, nets, tk.pin_shape ? 4 : 0);
}

static ActorTail tail_args(sactd3_engine* e, const float* z2, const float* P, int M, int mode, int train,
                           int site_buf, unsigned site_code, float* dst, int ldd, int dst_off, float* logp) {
  ActorTail t{};
  t.z2 = z2; t.P = P; t.L = e->La; t.B = M; t.o = e->o; t.a = e->a; t.ln = e->cfg.layer_norm;
  t.sac = !e->cfg.prefer_td3_over_sac; t.mode = mode; t.train = train;
  t.ctl = e->ctl; t.ctr = site_buf == SACTD3_SITE_PREDICT ? &e->ctl->predict_ctr : &e->ctl->noise_ctr;
  t.site_buf = site_buf; t.site_code = site_code; t.eps = e->eps[site_buf];
  t.scale = e->scale; t.bias = e->bias; t.min_ac = e->min_ac; t.max_ac = e->max_ac;
  t.dst = dst; t.ldd = ldd; t.dst_off = dst_off; t.logp = logp;
  t.h2 = e->a_h2; t.xh2 = e->a_xh2; t.rstd2 = e->a_rs2; t.tg = e->a_tg; t.a4 = e->a4;
  t.td3_std = e->cfg.td3_std; t.td3_c = e->cfg.td3_c; t.noise_std = e->cfg.actor_noise_std;
  return t;
}
static NoiseJob noise_job(sactd3_engine* e, int site_buf, unsigned site_code, int ctr_add, int rows) {
  NoiseJob z{};
  z.eps = e->eps[site_buf]; z.ctr = site_buf == SACTD3_SITE_PREDICT ? &e->ctl->predict_ctr : &e->ctl->noise_ctr;
  z.ctr_add = ctr_add; z.site_code = site_code; z.site_buf = site_buf; z.n = rows * e->a;
  return z;
}
// rows of the batch one block of the actor-tail kernel handles (narrow heads: one wave per 4 rows, see k_actor_tail_s)
static int tail_rows_per_block(const ActorTail& t) { return (t.L.nh <= 8 && t.a <= 8) ? 4 : 16; }
// The tails t[0 .. n) (all of B rows through the same head shape) as ONE launch of the kernel that holds `width` of them: 1; 2 (the
// opening pair's target-action and policy tails); 5 (the run-ahead: n <= 5, blocks exist for n tails only).  4-row or 16-row form.
static int launch_tails(EnqCtx& x, int width, const ActorTail* t, int n) {
  const int B = t[0].B, nh = t[0].L.nh, a = t[0].a, o = t[0].o;
  const bool rows4 = tail_rows_per_block(t[0]) == 4;
  const int nb = rows4 ? (B + 3) / 4 : (B + 15) / 16;
  const dim3 grid((unsigned)(n * nb)), block(rows4 ? 64 : 256);
  const double fl = 2.0 * n * B * (double)HID * nh;
  if (width == 1) {
    const double by = 4.0 * ((double)B * HID * (t->train ? 3 : 1) + (double)nh * (HID + 1) + 2.0 * HID + (double)B * (3 * a + 2) + (t->obs_src ? 2.0 * B * o : 0.0));
    if (rows4) LAUNCH("k_actor_tail_s<4>", fl, by, k_actor_tail_s<4>, grid, block, t[0]);
    else LAUNCH("k_actor_tail", fl, by, k_actor_tail, grid, block, t[0]);
  } else if (width == 2) {
    const double by = 4.0 * ((double)B * HID * 4 + 2.0 * nh * (HID + 1) + 4.0 * HID + (double)B * (6 * a + 4 + 2 * o));
    if (rows4) LAUNCH("k_actor_tail_s2<4>", fl, by, k_actor_tail_s2<4>, grid, block, t[0], t[1], nb);
    else LAUNCH("k_actor_tail2", fl, by, k_actor_tail2, grid, block, t[0], t[1], nb);      // (wide heads: the two tails as one launch of the general kernel)
  } else {
    ActorTail5 T{};
    for (int i = 0; i < 5; ++i) T.t[i] = t[i < n ? i : 0];                               // (the copies never run: blocks exist for n tails only)
    T.nb = nb; T.n = n;
    // (a policy pass at the end -- the next period's -- also writes its backward stores and [s | pi(s)])
    const double by = 4.0 * n * ((double)B * HID + (double)nh * (HID + 1) + 2.0 * HID + (double)B * (3 * a + 2)) + (t[n - 1].train ? 8.0 * (double)B * (HID + o) : 0.0);
    if (rows4) LAUNCH("k_actor_tail_s5<4>", fl, by, k_actor_tail_s5<4>, grid, block, T);
    else LAUNCH("k_actor_tail5", fl, by, k_actor_tail5, grid, block, T);
  }
  return 0;
}
static int launch_tail(EnqCtx& x, const ActorTail& t) { return launch_tails(x, 1, &t, 1); }

static int enqueue_gather(EnqCtx& x, const float* ring, int identity_len) {
  sactd3_engine* e = x.e;
  const GatherArgs g = gather_args(e, ring, identity_len);
  // 2 B T + 4 B, T = 4 (2o + a + 1) + 1
  LAUNCH("k_gather", 0.0, 2.0 * e->B * (4.0 * (2 * e->o + e->a + 1) + 1.0) + 4.0 * e->B, k_gather, dim3(gather_blocks((long)e->B * e->rec4)), dim3(256), g);
  return 0;
}

static AdamArgs adam_args(sactd3_engine* e, float* p, const float* g, float* m, float* v, long n, const float* adam) {
  AdamArgs a{};
  a.p = p; a.g = g; a.m = m; a.v = v; a.n = n; a.adam = adam;
  a.b1 = e->cfg.adam_beta1; a.b2 = e->cfg.adam_beta2; a.eps = e->cfg.adam_eps;
  return a;
}
static int launch_adam(EnqCtx& x, const AdamArgs& a) {
  const int blocks = (int)std::min<long>(512, (a.n / 4 + 255) / 256);
  LAUNCH("k_adam", 0.0, 28.0 * a.n, k_adam, dim3(std::max(blocks, 1)), dim3(256), a);
  return 0;
}

// Can the actor trunk that opens an iteration (1 net, or 2 groups when the policy pass is merged in) carry a temperature step as an
// extra block?  The k_nt launches can (fused first layer, or the layer-2 launch of the layer-by-layer form); the tiled k_nt64 pair
// of launches with >= 3/4 of the chip in 64 x 64 tiles cannot (see enqueue_trunk).
static bool opening_trunk_carries_alpha(const sactd3_engine* e) {
  const int B = e->B;
  const bool tiled = B >= BIG_BATCH && ((B + 63) / 64) * (HID / 64) * 2 >= (3 * e->num_cus) / 4;
  return !tiled;
}
// Does the actor trunk that opens a fused iteration read its rows from the ring itself, with the gather into the batch slot riding in
// the same launch?  Narrow observations below the large-batch threshold (fused k_nt), and wide ones at large batch (k_nt64<2,2,1>).
static bool opening_trunk_gathers(const sactd3_engine* e) {
  return (e->o <= 64 && e->B < BIG_BATCH) || (e->o > 64 && e->B >= BIG_BATCH && opening_trunk_carries_alpha(e));
}

// Does the opening pair of a fused iteration with actor updates hold the FIRST actor update's pi(s) pass too (see enqueue_opening_pair)?
// In the fused-first-layer launches of narrow observations, and as a second group of the layer-by-layer launches of wide ones at
// large batch (Humanoid: two nodes fewer per actor iteration).
static bool opening_merges_policy(const sactd3_engine* e) {
  return (opening_trunk_gathers(e) && e->o <= 64) || (e->o > 64 && e->B >= BIG_BATCH);
}
// (TD3, fused iteration without actor updates) can the critics' weight-gradient launch carry the actor target's Polyak update as
// extra blocks?  (the split-M route has no riding blocks)
static bool actor_target_rides(const sactd3_engine* e) { return !(e->B >= BIG_BATCH && e->Gp); }

// An iteration's place in the sequence being enqueued (orchestrator.py:337-352 decides the first two).
// slot / pre_sampled / ahead: the pipelined form of a period graph (period_is_pipelined): iteration i of the period trains on batch
// slot i; the first one (with the actor updates) also runs the sampling + next-action passes of the `ahead` iterations behind it,
// which are then `pre_sampled`: their sample, gather and next-action pass (a', log pi(a'|s')) are there, the update starts at the
// twin-critic trunk.  The first iteration is itself pre_sampled: its opening pair (with the first actor update's policy pass) was
// left by the previous period or by the opening graph.
// chain_slot >= 0: (chained periods) ... and the opening pair of the NEXT period's first iteration into that batch slot.
struct IterPlace {
  bool actor = false, targets = false;      // the iteration has actor updates / a target update
  bool more = false;                        // another iteration follows in the same graph
  bool weighted = false;                    // (the API path only) the critic loss is weighted by the slot's w
  int slot = 0; bool pre_sampled = false; int ahead = 0, chain_slot = -1;
};
static IterPlace single_iteration(bool actor, bool targets) {      // (sactd3_step)
  IterPlace it;
  it.actor = actor; it.targets = targets;
  return it;
}

// The opening pair of a critic update (agents/agent.py:194-205): the actor trunk on s' and its tail, the target action.
// fused_sample: the update opens a fused iteration and owns the replay sampling (orchestrator.py:338); with a narrow
// observation the gather rides in the trunk kernel, otherwise enqueue_step has launched k_gather just before.
// it.actor: also run the first actor update's policy pass pi(s) in the same two launches where they can (opening_merges_policy).
// it.pre_sampled: the pair runs ahead of its iteration (the opening graph): the counter ticks -- critics' and actor's step counters,
// sample counter -- are left to that iteration's twin-critic trunk (enqueue_update_qnets).
static int enqueue_opening_pair(EnqCtx& x, const IterPlace& it, bool fused_sample) {
  sactd3_engine* e = x.e;
  const bool ticks = !it.pre_sampled;
  const sactd3_config& c = e->cfg;
  const int B = e->B, td3 = c.prefer_td3_over_sac;
  const sactd3_engine::BatchSlot& S = e->bs[it.slot];
  // target action: SAC a' ~ pi(s') with the ONLINE actor (agent.py:205); TD3 pi_targ(s') + clipped noise (agent.py:194-200)
  const float* Pact = td3 ? e->Ta : e->Pa;
  const bool in_kernel_gather = fused_sample && opening_trunk_gathers(e);
  const bool merge_policy = it.actor && fused_sample && opening_merges_policy(e);
  const bool wide_merge = merge_policy && e->o > 64;
  x.role = fused_sample ? (merge_policy ? "critic/next-action+sample & actor0/policy" : "critic/next-action+sample") : "critic/next-action";
  // (layer-by-layer launches materialise z1: the target-action group borrows the target critics' z1 slab, idle until the next launch)
  TrunkGrp g[2] = {{S.Xn, Pact, wide_merge ? e->t_z1 : e->a_z1, merge_policy ? e->a_z2n : e->a_z2, nullptr, nullptr, nullptr, e->ldc},
                   {S.X, e->Pa, e->a_z1, e->a_z2, e->a_xh1, e->a_h1, e->a_rs1, 0}};
  TrunkTicks tk{&e->ctl->t_q, (fused_sample && !in_kernel_gather) ? &e->ctl->sample_ctr : nullptr, e->ctl->adam_q, e->ctl->pw_q, c.qnets_lr};
  if (!ticks) { tk.tick0 = nullptr; tk.tick1 = nullptr; tk.adam_out = nullptr; tk.adam_pw = nullptr; }
  if (in_kernel_gather) {   // the trunk reads its rows from the ring itself; the gather into the batch slot rides along
    tk.ngather = 1; tk.gather[0] = gather_args(e, e->ring, -1, it.slot);
    for (auto& gg : g) { gg.ring = true; gg.ring_idx = S.idx; }
  }
  const int mode = td3 ? (c.targ_actor_smoothing ? 1 : 0) : 0;
  bool eps_ready = false;
  if (!td3 || mode == 1) { tk.noise[tk.nnoise++] = noise_job(e, SACTD3_SITE_CRITIC, 0u, 0, B); tk.noise[tk.nnoise - 1].eps = S.eps_c; tk.noise_taken = &eps_ready; }
  // a temperature step deferred from the previous iteration of the same graph (sactd3_step_period) rides in this launch; its
  // tick of the noise counter stays owed: this iteration's draws count one ahead and the critics' last kernel ticks by two
  int owed = 0;
  if (x.alpha_pending && x.alpha_tick_owed && fused_sample && opening_trunk_carries_alpha(e)) {
    tk.alpha = &x.alpha; x.alpha_pending = false;
    owed = 1;
    for (int i = 0; i < tk.nnoise; ++i) tk.noise[i].ctr_add += 1;
  }
  if (merge_policy) {
    // the policy sample of the first actor update: same actor parameters (the critic update does not touch them), the stream
    // counter one ahead (the critic update's last kernel bumps it before the actor update would have read it)
    if (!td3) { tk.noise[tk.nnoise++] = noise_job(e, SACTD3_SITE_ACTOR0, 16u, 1 + owed, B); tk.noise_taken = &eps_ready; }
    if (!wide_merge) tk.force_ks = 4;
    if (ticks) { tk.tick0b = &e->ctl->t_a; tk.adam_out_b = e->ctl->adam_a; tk.adam_pw_b = e->ctl->pw_a; tk.lr_b = c.actor_lr; }
  }
  RCCHK(enqueue_trunk(x, e->ldc, e->o, B, e->La, 0, merge_policy ? 2 : 1, 1, g, tk));
  ActorTail t[2];
  t[0] = tail_args(e, merge_policy ? e->a_z2n : e->a_z2, Pact, B, mode, 0, SACTD3_SITE_CRITIC, 0u, S.Xn, e->ldc, e->o, S.logp_n);
  t[0].eps = S.eps_c;
  t[0].eps_ready = eps_ready; t[0].ctr_add = owed;
  if (in_kernel_gather && ticks) t[0].tick = &e->ctl->sample_ctr;   // every reader of the index stream (the trunk kernel) is done
  if (!merge_policy) return launch_tail(x, t[0]);
  t[1] = tail_args(e, e->a_z2, e->Pa, B, 0, 1, SACTD3_SITE_ACTOR0, 16u, e->Xp, e->ldc, e->o, e->logp_pi);
  t[1].obs_src = S.X; t[1].lds = e->ldc; t[1].ctr_add = 1 + owed; t[1].eps_ready = eps_ready;     // Xp = [s | pi(s)]
  return launch_tails(x, 2, t, 2);
}

// agents/agent.py:183-242
// fused_sample: see enqueue_opening_pair (false: the API path -- the batch slot was filled by the caller, no policy pass, no target update).
// it.targets: with the target updates in the optimiser epilogue (see enqueue_step, actor_target_rides).
// it.pre_sampled: the opening pair is already there: the update starts at the twin-critic trunk, which then makes its ticks.
static int enqueue_update_qnets(EnqCtx& x, const IterPlace& it, bool fused_sample) {
  sactd3_engine* e = x.e;
  const sactd3_config& c = e->cfg;
  const int B = e->B, ln = c.layer_norm, td3 = c.prefer_td3_over_sac;
  const long BH = (long)B * HID;
  const sactd3_engine::BatchSlot& S = e->bs[it.slot];
  float* const fused_polyak_targ = it.targets ? e->Tc : nullptr;
  if (!it.pre_sampled) RCCHK(enqueue_opening_pair(x, it, fused_sample));
  {  // twin target critics on (s', a') and twin online critics on (s, a) in one launch (agent.py:208-210, 230-232).
     // (Measured: running the online pair on a fork/join side branch of the graph instead costs +30 us per replay on
     //  ROCm 7.2 -- cross-stream edges are far dearer than the 1.7 us of a linear edge -- so graphs stay linear.)
    const TrunkGrp g[2] = {{S.Xn, e->Tc, e->t_z1, e->t_z2, nullptr, nullptr, nullptr},
                           {S.X, e->Pc, e->c_z1, e->c_z2, e->c_xh1, e->c_h1, e->c_rs1}};
    x.role = "critic/twin-q(2 target + 2 online)";
    TrunkTicks tk{nullptr, nullptr, nullptr, nullptr, 0.f};
    if (it.pre_sampled) {   // this launch opens the update: the critics' step counter + Adam scalars, and a temperature step deferred from the
                            // period's first iteration (its tick of the noise counter is made up by this update's last kernel)
      tk.tick0 = &e->ctl->t_q; tk.adam_out = e->ctl->adam_q; tk.adam_pw = e->ctl->pw_q; tk.lr = c.qnets_lr;
      if (it.actor) {   // ... the ticks the precomputed opening pair left undone: the sample counter and the actor's step counter
        tk.tick1 = &e->ctl->sample_ctr;
        tk.tick0b = &e->ctl->t_a; tk.adam_out_b = e->ctl->adam_a; tk.adam_pw_b = e->ctl->pw_a; tk.lr_b = c.actor_lr;
      }
      if (x.alpha_pending && x.alpha_tick_owed) { tk.alpha = &x.alpha; x.alpha_pending = false; }
    }
    RCCHK(enqueue_trunk(x, e->ldc, e->o + e->a, B, e->Lc, e->Lc.size, 2, 2, g, tk));
  }
  // the tick a deferred temperature step owes, once one of the two trunk launches above has carried the step
  const int ctr_owed = (x.alpha_tick_owed && !x.alpha_pending) ? 1 : 0;
  if (ctr_owed) x.alpha_tick_owed = false;
  x.role = "critic/loss+backward";
  const bool fused_tail_nn = B < BIG_BATCH;   // the tail AND dh1 = dz2 W2 in one launch (k_ctail_nn)
  const bool fold_ln1 = fused_tail_nn;       // ... then with layer 1's LayerNorm backward inside the weight-gradient launch (TnProb::fold)
  {
    CriticTail t{};
    t.z2t = e->t_z2; t.z2 = e->c_z2; t.PT = e->Tc; t.P = e->Pc; t.p_ns = e->Lc.size; t.L = e->Lc;
    t.rew = S.rew; t.done = S.done; t.logp_next = S.logp_n; t.log_alpha = e->la;
    t.B = B; t.ln = ln; t.sac = !td3; t.bcq = c.bcq_style_targ_mix; t.gamma = c.gamma;
    t.qt = e->qt; t.y = e->y; t.q = e->q; t.dz2 = e->c_dz2; t.part = e->part; t.part_s = e->part_s; t.pstride = e->nblk4;
    if (fused_tail_nn) {   // 16-row blocks x 32-column tiles
      CtailNn f{};
      f.c = t; f.c.pstride = e->nblk4; f.Wt = e->Pc + e->Lc.W2; f.ldw = HID; f.dX = e->c_dh1;
      f.f = fold_args(fold_ln1, ln, e->Lc, e->c_h1, e->c_xh1, e->c_ps, e->c_ps + 2L * B * PS_W);
      f.xr = pick_xr(e->nblk, HID / 32, 4.0 * 3 * B * HID, 4.0 * HID * HID);
      const double fl = 2.0 * 4 * B * (double)HID + 2.0 * 2 * (double)B * HID * HID, by = 4.0 * (6.0 * BH + 4.0 * 4 * HID + 8.0 * B) + 4.0 * 2 * ((double)HID * HID + (double)B * HID);
      const dim3 grid((unsigned)(e->nblk * (HID / 32)), 1, 2);
      if (it.weighted) LAUNCH("k_ctail_nn_w<2>", fl, by + 4.0 * B, k_ctail_nn_w<2>, grid, dim3(256), (CtailNnW{f, S.w}));
      else LAUNCH("k_ctail_nn<2>", fl, by, k_ctail_nn<2>, grid, dim3(256), f);
    } else {
      const double fl = 2.0 * 4 * B * (double)HID, by = 4.0 * (6.0 * BH + 4.0 * 4 * HID + 8.0 * B);
      if (it.weighted) LAUNCH("k_critic_tail_w<16>", fl, by + 4.0 * B, k_critic_tail_w<16>, dim3(e->nblk, 2), dim3(256), (CriticTailW{t, S.w}));
      else LAUNCH("k_critic_tail<16>", fl, by, k_critic_tail<16>, dim3(e->nblk, 2), dim3(256), t);
    }
  }
  if (!fused_tail_nn)  // dh1 = dz2 W2
    RCCHK(launch_nn(x, "k_nn.dh1", dh1_args(e->c_dz2, e->Pc + e->Lc.W2, e->c_dh1, B, BH, e->Lc.size), 2));
  if (!fold_ln1) {
    const LnBwd l = ln_bwd_args(e, e->c_dh1, e->c_xh1, e->c_h1, e->c_rs1, e->Pc + e->Lc.g1, e->Lc.size, ln, e->c_dz1);
    LAUNCH("k_ln_bwd<16>", 0.0, 4.0 * 2 * (4.0 * BH + B + HID), k_ln_bwd<16>, dim3(e->nblk, 2), dim3(256), l);
  }
  {  // every critic gradient + the Adam step (+ Polyak) in one launch:
     //   dW2 = dz2^T h1, db2, dgamma2, dbeta2, dWhead, dbhead ; dW1 = dz1^T [s|a], db1, dgamma1, dbeta1
    TnArgs g{};
    g.nprob = 2; g.M = B; g.G = e->Gc; g.g_ns = e->Lc.size;
    const int i2 = 0, i1 = fold_ln1 ? 2 : 1;           // folded: [W2 columns 0 .. 127][layer 1][W2 columns 128 .. 255] (tn_cols)
    g.pr[i2] = tn_prob(e->c_dz2, HID, BH, HID, e->c_h1, HID, BH, HID, e->Lc.W2, HID, e->Lc.b2);
    if (ln) { tn_fin(g.pr[i2], 0, e->Lc.g2, e->nblk); tn_fin(g.pr[i2], 1, e->Lc.be2, e->nblk); }
    tn_fin(g.pr[i2], 2, e->Lc.Wh, e->nblk); g.pr[i2].fin_s_off = e->Lc.bh; g.pr[i2].fin_s_nblk = e->nblk;
    g.pr[i1] = tn_prob(fold_ln1 ? e->c_dh1 : e->c_dz1, HID, BH, HID, S.X, e->ldc, 0, e->o + e->a, e->Lc.W1, e->Lc.ld1, e->Lc.b1);
    if (!fold_ln1 && ln) { tn_fin(g.pr[i1], 3, e->Lc.g1, e->nblk); tn_fin(g.pr[i1], 4, e->Lc.be1, e->nblk); }
    if (fold_ln1) {
      tn_fold(g.pr[i1], ln, e->Lc, e->c_xh1, e->c_rs1, e->c_ps, e->c_dz1, e->c_ps + 2L * B * PS_W);
      g.nprob = 3;
      g.pr[1] = tn_cols(g.pr[0], HID / 2, HID / 2); g.pr[0] = tn_cols(g.pr[0], 0, HID / 2); g.pr[0].xr_force = g.pr[1].xr_force = 8;
      std::swap(g.pr[1], g.pr[2]);
    }
    g.part = e->part; g.pstride = e->nblk4; g.part_s = e->part_s;
    g.apply = 1; g.P = e->Pc; g.Mo = e->Mc; g.Vo = e->Vc; g.T = fused_polyak_targ; g.tau = c.polyak; g.adam = e->ctl->adam_q;
    g.b1 = c.adam_beta1; g.b2 = c.adam_beta2; g.eps = c.adam_eps;
    g.loss_part = e->part_s; g.loss_n = 2 * e->nblk4; g.loss_stride = 2; g.loss_off = 1; g.loss_scale = 1.0f / (float)B;   // unused tail entries stay 0
    g.loss_dst = &e->ctl->metrics[SACTD3_M_QF_LOSS]; g.tick = &e->ctl->noise_ctr;
    const bool rides = it.targets && td3 && !it.actor && actor_target_rides(e);
    if (rides) {
      g.pk.t0 = e->Ta; g.pk.p0 = e->Pa; g.pk.n0 = e->La.size; g.pk.tau = c.polyak;
      // (few of them: the launch already has more blocks than the chip has CUs, and every extra one lands beside a tile block --
      //  64 riding blocks instead of 8: +0.8 us per TD3 iteration)
      g.pk_blocks = (int)std::min<long>(8, (e->La.size / 4 + 255) / 256);
    }
    RCCHK(launch_tn(x, fused_polyak_targ ? (rides ? "dW+adam+polyak & actor-target polyak" : "dW+adam+polyak") : "dW+adam", g, 2, ctr_owed));
  }
  return 0;
}

// The run-ahead of a pipelined period (see BatchSlot): passes through the actor that later iterations would open with, as extra groups
// of ONE trunk + tail pair inside the last actor update of the period's first iteration -- the actor does not change any more before
// those iterations run.  Every pass reads its rows from the ring itself (the sample drawn with sample_ctr + sample_add), the gathers
// into the batch slots and the tails' draws ride in the trunk launch.  buf: which of ah_z1 / ah_z2 holds the pass's layer outputs.
struct RunAhead {
  sactd3_engine* e;
  TrunkGrp g[5] = {};
  TrunkTicks tk{nullptr, nullptr, nullptr, nullptr, 0.f};
  ActorTail t[5] = {};
  int n = 0;
  // the next-action pass a'(s') of the iteration that trains on batch slot k, through the actor parameters P (SAC: the online actor,
  // TD3: the target actor as it will be then); its draws are those of noise counter + noise_add
  void add_next(int k, const float* P, int buf, int sample_add, int noise_add) {
    const sactd3_engine::BatchSlot& S = e->bs[k];
    const bool td3 = e->cfg.prefer_td3_over_sac;
    const int mode = (td3 && e->cfg.targ_actor_smoothing) ? 1 : 0;
    g[n] = TrunkGrp{S.Xn, P, e->ah_z1[buf], e->ah_z2[buf], nullptr, nullptr, nullptr, e->ldc};
    g[n].ring = true; g[n].sctr_add = sample_add; g[n].ring_idx = S.idx;
    tk.gather[tk.ngather++] = gather_args(e, e->ring, -1, k, sample_add);
    if (!td3 || mode == 1) { tk.noise[tk.nnoise] = noise_job(e, SACTD3_SITE_CRITIC, 0u, noise_add, e->B); tk.noise[tk.nnoise++].eps = S.eps_c; }
    t[n] = tail_args(e, e->ah_z2[buf], P, e->B, mode, 0, SACTD3_SITE_CRITIC, 0u, S.Xn, e->ldc, e->o, S.logp_n);
    t[n].eps = S.eps_c; t[n].ctr_add = noise_add;
    ++n;
  }
  // the first actor update's policy pass pi(s) of the iteration that trains on batch slot k (behind add_next(k, ...): the same sample,
  // that gather fills S.X); it keeps its stores for the backward pass
  void add_policy(int k, int buf, int sample_add, int noise_add) {
    const sactd3_engine::BatchSlot& S = e->bs[k];
    g[n] = TrunkGrp{S.X, e->Pa, e->ah_z1[buf], e->ah_z2[buf], e->a_xh1, e->a_h1, e->a_rs1, 0};
    g[n].ring = true; g[n].sctr_add = sample_add; g[n].ring_idx = S.idx;
    if (!e->cfg.prefer_td3_over_sac) tk.noise[tk.nnoise++] = noise_job(e, SACTD3_SITE_ACTOR0, 16u, noise_add, e->B);
    t[n] = tail_args(e, e->ah_z2[buf], e->Pa, e->B, 0, 1, SACTD3_SITE_ACTOR0, 16u, e->Xp, e->ldc, e->o, e->logp_pi);
    t[n].obs_src = S.X; t[n].lds = e->ldc; t[n].ctr_add = noise_add;      // Xp = [s | pi(s)]
    ++n;
  }
  // the trunk + tail pair; tail 0 moves the sample counter past the `ahead` samples drawn here
  int launch(EnqCtx& x, int ahead) {
    bool eps_ready = false;
    if (tk.nnoise) tk.noise_taken = &eps_ready;
    if (tk.ngather) { tk.force_ks = 4; tk.no_tiled64 = true; }      // (the launch shapes of the single-net passes: ring rows, riding gathers, bit-equal results)
    RCCHK(enqueue_trunk(x, e->ldc, e->o, e->B, e->La, 0, n, 1, g, tk));
    if (ahead) { t[0].tick = &e->ctl->sample_ctr; t[0].tick_add = ahead - 1; }      // every reader of the index streams (the trunk launch above) is done
    for (int i = 0; i < n; ++i) t[i].eps_ready = eps_ready;
    return launch_tails(x, tk.ngather ? 5 : 1, t, n);
  }
};

// agents/agent.py:244-318.  j = index of this actor update inside the iteration (selects the noise buffers).
// fused == false: the API path -- one update on its own (a default place: batch slot 0, nothing ahead, nothing deferred).
static int enqueue_update_actor(EnqCtx& x, const IterPlace& it, int j, bool fused) {
  sactd3_engine* e = x.e;
  const sactd3_config& c = e->cfg;
  const int B = e->B, ln = c.layer_norm, td3 = c.prefer_td3_over_sac, nq = e->nq_actor;
  const long BH = (long)B * HID;
  const bool last = j + 1 == c.actor_update_delay, can_merge = fused && !td3 && c.autotune;
  // head_done: this update's policy sample was already produced -- by the opening pair (first update), or by the previous update's dual tail
  const bool head_done = j == 0 ? fused && (it.pre_sampled || opening_merges_policy(e)) : can_merge;
  const bool merge_next = can_merge && !last;      // produce the NEXT update's policy sample together with this update's temperature draw
  // (TD3, last actor update of a fused iteration) lerp the actor target towards the freshly stepped actor in the same kernel that applies
  // the step (agents/agent.py:331 after :286)
  float* const polyak_targ = (it.targets && td3 && last) ? e->Ta : nullptr;
  // (last actor update of an iteration that is followed by another one in the same graph) leave the temperature step to the next
  // iteration's opening launch, when that launch can carry it
  const bool defer_alpha = last && it.more && !td3 && (it.ahead > 0 || opening_trunk_carries_alpha(e));
  // (last actor update) the run-ahead of a pipelined period, see RunAhead and IterPlace -- SAC: in this update's last trunk / tail
  // launches (the temperature draw's), TD3: as a pair of its own
  const int ahead = last ? it.ahead : 0, chain_slot = last ? it.chain_slot : -1;
  const int sb_a = SACTD3_SITE_ACTOR0 + (j & 1), sb_l = SACTD3_SITE_ALPHA0 + (j & 1);
  const bool clip = c.clip_norm > 0.f;
  const float* SX = e->bs[it.slot].X;       // the observations of the batch this iteration trains on
  const bool small_head = e->nh <= 8 && e->a <= 8;      // single-wave 4-row head backward (k_actor_head_bwd_s)
  x.role = (j & 1) ? "actor1/policy" : "actor0/policy";
  if (!head_done) {  // a_pi, logp = pi(s) with stores for the backward pass
    const TrunkGrp g{SX, e->Pa, e->a_z1, e->a_z2, e->a_xh1, e->a_h1, e->a_rs1};
    TrunkTicks tk{&e->ctl->t_a, nullptr, e->ctl->adam_a, e->ctl->pw_a, c.actor_lr};
    bool eps_ready = false;
    if (!td3) { tk.nnoise = 1; tk.noise[0] = noise_job(e, sb_a, 16u, 0, B); tk.noise_taken = &eps_ready; }
    RCCHK(enqueue_trunk(x, e->ldc, e->o, B, e->La, 0, 1, 1, &g, tk));
    ActorTail t = tail_args(e, e->a_z2, e->Pa, B, 0, 1, sb_a, 16u, e->Xp, e->ldc, e->o, e->logp_pi);
    t.obs_src = SX; t.lds = e->ldc;   // Xp = [s | pi(s)]
    t.eps_ready = eps_ready;
    RCCHK(launch_tail(x, t));
  }
  x.role = (j & 1) ? "actor1/q(s,pi)" : "actor0/q(s,pi)";
  {  // Q_i(s, a_pi) through the online critics as constants (agent.py:272-278)
    const TrunkGrp g{e->Xp, e->Pc, e->c_z1, e->c_z2, e->c_xh1, e->c_h1, e->c_rs1};
    TrunkTicks tk{nullptr, nullptr, nullptr, nullptr, 0.f};
    if (x.alpha_pending) { tk.alpha = &x.alpha; x.alpha_pending = false; }   // the previous update's temperature step
    RCCHK(enqueue_trunk(x, e->ldc, e->o + e->a, B, e->Lc, e->Lc.size, 1, nq, &g, tk));
  }
  x.role = (j & 1) ? "actor1/loss+backward" : "actor0/loss+backward";
  const bool fused_qtail_nn = B < BIG_BATCH;
  // dQ/da finished inside the two fused launches around it (QaFold): narrow heads, ac_dim <= 7
  const bool qa_fold = fused_qtail_nn && small_head && e->a <= 7;    // (small_head: k_headbwd_nn is the consumer)
  {
    ActorQTail t{};
    t.z2c = e->c_z2; t.P = e->Pc; t.p_ns = e->Lc.size; t.L = e->Lc; t.logp = e->logp_pi; t.log_alpha = e->la;
    t.B = B; t.ln = ln; t.sac = !td3; t.q = e->q_pi; t.dz2 = e->c_dz2; t.part_s = e->part_sa;
    if (fused_qtail_nn) {   // the tail AND dh1_i = dz2_i W2_i in one launch (k_qtail_nn): loss partials per 16-row block
      QtailNn f{};
      f.c = t; f.Wt = e->Pc + e->Lc.W2; f.ldw = HID; f.dX = e->c_dh1;
      if (qa_fold) {
        qa_fold_args(f.qa, e);
        f.qa.h1 = e->c_h1; f.qa.xh1 = e->c_xh1; f.qa.g1_off = e->Lc.g1; f.qa.w1_off = e->Lc.W1; f.qa.ld1 = e->Lc.ld1; f.qa.k_off = e->o;
      }
      const double fl = 2.0 * nq * B * (double)HID + 2.0 * nq * (double)B * HID * HID, by = 4.0 * nq * (2.0 * BH + 4.0 * HID + 2.0 * B) + 4.0 * nq * ((double)HID * HID + (double)B * HID);
      if (nq == 2) {
        f.xr = pick_xr(e->nblk, HID / 32, 4.0 * 2 * B * HID, 4.0 * HID * HID);
        LAUNCH("k_qtail_nn<2>", fl, by, k_qtail_nn<2>, dim3((unsigned)(e->nblk * (HID / 32)), 1, 2), dim3(256), f);
      } else {
        f.xr = pick_xr(e->nblk, HID / 16, 4.0 * B * HID, 4.0 * HID * HID);
        LAUNCH("k_qtail_nn<1>", fl, by, k_qtail_nn<1>, dim3((unsigned)(e->nblk * (HID / 16)), 1, 1), dim3(256), f);
      }
    } else LAUNCH("k_actorq_tail<4>", 2.0 * nq * B * (double)HID, 4.0 * nq * (2.0 * BH + 4.0 * HID + 2.0 * B), k_actorq_tail<4>, dim3(e->nblk4), dim3(64), t);
  }
  if (!fused_qtail_nn) RCCHK(launch_nn(x, "k_nn.dh1", dh1_args(e->c_dz2, e->Pc + e->Lc.W2, e->c_dh1, B, BH, e->Lc.size), nq));
  if (!qa_fold) {
    LnBwd l = ln_bwd_args(e, e->c_dh1, e->c_xh1, e->c_h1, e->c_rs1, e->Pc + e->Lc.g1, e->Lc.size, 0, e->c_dz1);
    // fused: dA_i = dz1_i W1_i[:, o:o+a]  (gradient of Q_i with respect to the action)
    l.W1 = e->Pc + e->Lc.W1; l.ldw1 = e->Lc.ld1; l.k_off = e->o; l.na = e->a; l.dA = e->dA; l.ldA = e->a4;
    LAUNCH("k_ln_bwd<16>.dQ/da", 2.0 * nq * B * (double)HID * e->a, 4.0 * nq * (4.0 * BH + B + HID + (double)HID * e->a + (double)B * e->a),
           k_ln_bwd<16>, dim3(e->nblk, nq), dim3(256), l);
  }
  const bool fused_head_nn = small_head && B < BIG_BATCH;   // the head backward AND dh1 = dz2 W2 in one launch (k_headbwd_nn)
  const bool fold_ln1 = fused_head_nn;                     // as the critics' (enqueue_update_qnets)
  {
    ActorHeadBwd h{};
    h.dA = e->dA; h.dA_ns = (long)B * e->a4; h.ldA = e->a4; h.nq = nq; h.tg = e->a_tg; h.a4 = e->a4; h.eps = e->eps[sb_a];
    h.log_alpha = e->la; h.scale = e->scale; h.P = e->Pa; h.L = e->La; h.xh2 = e->a_xh2; h.rstd2 = e->a_rs2; h.h2 = e->a_h2;
    h.B = B; h.a = e->a; h.ln = ln; h.sac = !td3; h.du = e->a_du; h.ldu = e->ldu; h.dz2 = e->a_dz2;
    h.part = e->part;
    // TD3+BC: the same launch in its BC form (kernels.h, BcArgs) -- the dataset action from the batch slot this iteration trains on
    BcArgs bk{};
    if (e->bc_on) {
      bk.ctl = e->ctl->bc; bk.q = e->q_pi; bk.pi = e->Xp; bk.act = SX; bk.ld = e->ldc; bk.off = e->o;
      bk.inv_ba = 1.0f / ((float)B * (float)e->a); bk.part = e->bc_part; bk.lam = &e->ctl->metrics[SACTD3_M_BC_LAMBDA];
    }
    if (fused_head_nn) {   // column partials per 16-row block
      HeadBwdNn f{};
      f.c = h; f.Wt = e->Pa + e->La.W2; f.ldw = HID; f.dX = e->a_dh1;
      if (qa_fold) { qa_fold_args(f.qa, e); f.qa.rstd = e->c_rs1; f.qa.dA = e->dA; }
      f.f = fold_args(fold_ln1, ln, e->La, e->a_h1, e->a_xh1, e->a_ps, e->a_ps + (long)B * PS_W);
      f.xr = pick_xr(e->nblk, HID / 16, 4.0 * 2 * B * HID, 4.0 * HID * HID);
      const double fl = 2.0 * B * (double)HID * e->nh + 2.0 * (double)B * HID * HID;
      const double by = 4.0 * (3.0 * BH + (double)e->nh * HID + (double)B * (nq * e->a + 4 * e->a + e->nh)) + 4.0 * ((double)HID * HID + (double)B * HID);
      if (e->bc_on) LAUNCH("k_headbwd_nn_bc", fl, by + 4.0 * B * (2.0 * e->a + 1), k_headbwd_nn_bc, dim3((unsigned)(e->nblk * (HID / 16))), dim3(256), f, bk);
      else LAUNCH("k_headbwd_nn", fl, by, k_headbwd_nn, dim3((unsigned)(e->nblk * (HID / 16))), dim3(256), f);
    } else {
      const double fl = 2.0 * B * (double)HID * e->nh, by = 4.0 * (3.0 * BH + (double)e->nh * HID + (double)B * (nq * e->a + 4 * e->a + e->nh));
      if (small_head) {
        if (e->bc_on) LAUNCH("k_actor_head_bwd_s_bc<4>", fl, by + 4.0 * B * (2.0 * e->a + 1), k_actor_head_bwd_s_bc<4>, dim3(e->nblk4), dim3(64), h, bk);
        else LAUNCH("k_actor_head_bwd_s<4>", fl, by, k_actor_head_bwd_s<4>, dim3(e->nblk4), dim3(64), h);
      } else if (e->bc_on) LAUNCH("k_actor_head_bwd_bc", fl, by + 4.0 * B * (2.0 * e->a + 1), k_actor_head_bwd_bc, dim3(e->nblk), dim3(256), h, bk);
      else LAUNCH("k_actor_head_bwd", fl, by, k_actor_head_bwd, dim3(e->nblk), dim3(256), h);
    }
  }
  if (!fused_head_nn) RCCHK(launch_nn(x, "k_nn.dh1", dh1_args(e->a_dz2, e->Pa + e->La.W2, e->a_dh1, B, 0, 0), 1));
  if (!fold_ln1) {
    const LnBwd l = ln_bwd_args(e, e->a_dh1, e->a_xh1, e->a_h1, e->a_rs1, e->Pa + e->La.g1, 0, ln, e->a_dz1);
    LAUNCH("k_ln_bwd<16>", 0.0, 4.0 * (4.0 * BH + B + HID), k_ln_bwd<16>, dim3(e->nblk, 1), dim3(256), l);
  }
  {  // every actor gradient (+ Adam unless clip_grad_norm_ needs the global norm first) in one launch:
     //   dWhead = du^T h2, dbhead ; dW2 = dz2^T h1, db2, dgamma2, dbeta2 ; dW1 = dz1^T s, db1, dgamma1, dbeta1
    TnArgs g{};
    g.nprob = 3; g.M = B; g.G = e->Ga; g.g_ns = 0;
    const int ih = 0, i2 = 1, i1 = fold_ln1 ? 3 : 2;      // folded: [head][W2 rows 0 .. 47][layer 1][W2 rows 48 .. 255] (tn_rows)
    g.pr[ih] = tn_prob(e->a_du, e->ldu, 0, e->nh, e->a_h2, HID, 0, HID, e->La.Wh, HID, e->La.bh);
    g.pr[i2] = tn_prob(e->a_dz2, HID, 0, HID, e->a_h1, HID, 0, HID, e->La.W2, HID, e->La.b2);
    const int nb_head = (small_head && !fused_head_nn) ? e->nblk4 : e->nblk;      // row blocks that wrote the head backward's column partials
    if (ln) { tn_fin(g.pr[i2], 0, e->La.g2, nb_head); tn_fin(g.pr[i2], 1, e->La.be2, nb_head); }
    g.pr[i1] = tn_prob(fold_ln1 ? e->a_dh1 : e->a_dz1, HID, 0, HID, SX, e->ldc, 0, e->o, e->La.W1, e->La.ld1, e->La.b1);
    if (!fold_ln1 && ln) { tn_fin(g.pr[i1], 3, e->La.g1, e->nblk); tn_fin(g.pr[i1], 4, e->La.be1, e->nblk); }
    if (fold_ln1) {
      tn_fold(g.pr[i1], ln, e->La, e->a_xh1, e->a_rs1, e->a_ps, e->a_dz1, e->a_ps + (long)B * PS_W);
      g.nprob = 4; g.pr[2] = tn_rows(g.pr[1], 48, HID - 48); g.pr[1] = tn_rows(g.pr[1], 0, 48); std::swap(g.pr[2], g.pr[3]);
    }
    g.part = e->part; g.pstride = e->nblk4; g.part_s = e->part_s;
    g.apply = clip ? 0 : 1; g.P = e->Pa; g.Mo = e->Ma; g.Vo = e->Va; g.T = clip ? nullptr : polyak_targ; g.tau = c.polyak; g.adam = e->ctl->adam_a;
    if (td3 && g.T && (ahead > 0 || chain_slot >= 0)) { g.T2 = e->Ta2; g.T3 = e->Ta3; }   // the actor target of the next two Polyak updates, now
    g.b1 = c.adam_beta1; g.b2 = c.adam_beta2; g.eps = c.adam_eps;
    g.loss_part = e->part_sa; g.loss_n = e->nblk4; g.loss_stride = 2; g.loss_off = 1; g.loss_scale = 1.0f / (float)B;
    g.loss_dst = &e->ctl->metrics[SACTD3_M_ACTOR_LOSS]; g.tick = (td3 && !clip) ? &e->ctl->noise_ctr : nullptr;
    BcFin bf{};
    if (e->bc_on) {      // the loss is finalised from the two kinds of partials and lambda (kernels.h, bc_loss_finish)
      bf.q_part = e->part_sa; bf.q_n = e->nblk4; bf.bc_part = e->bc_part; bf.bc_n = e->nblk4;
      bf.inv_b = 1.0f / (float)B; bf.inv_ba = 1.0f / ((float)B * (float)e->a);
      bf.ctl = e->ctl->bc; bf.lam = &e->ctl->metrics[SACTD3_M_BC_LAMBDA];
      bf.loss_dst = &e->ctl->metrics[SACTD3_M_ACTOR_LOSS]; bf.bc_dst = &e->ctl->metrics[SACTD3_M_BC_LOSS];
      g.loss_dst = nullptr;
    }
    RCCHK(launch_tn(x, clip ? "dW" : (polyak_targ ? "dW+adam+polyak" : "dW+adam"), g, 1, 0, e->bc_on ? &bf : nullptr));
  }
  if (clip) {
    NormArgs n{e->Ga, (long)e->La.size, c.clip_norm, e->gscale};
    LAUNCH("k_gradnorm", 0.0, 4.0 * e->La.size, k_gradnorm, dim3(1), dim3(1024), n);
    AdamArgs a = adam_args(e, e->Pa, e->Ga, e->Ma, e->Va, e->La.size, e->ctl->adam_a);
    a.gscale = e->gscale;
    a.targ = polyak_targ; a.tau = c.polyak;
    a.tick = td3 ? &e->ctl->noise_ctr : nullptr;
    RCCHK(launch_adam(x, a));
  }
  if (td3 && (ahead > 0 || chain_slot >= 0)) {
    // TD3, pipelined period (see BatchSlot): the online actor is final until the next period's actor updates, and the TARGET actor
    // of the following iterations is a fixed sequence of lerps towards it -- Ta (after this update's Polyak step), Ta2, Ta3 (written by
    // the Adam epilogue above).  So the sampling, gather and next-action pass of the period's critic-only iterations, and the opening
    // pair of the next period's first iteration (its next-action pass through Ta3 / Ta2, its first policy pass through Pa), run here
    // as ONE trunk + tail pair.  Streams: iteration k samples with sample_ctr + (k - 1) and draws its smoothing noise with noise
    // counter + (k - 1) (the counter already counts this update's tick; one tick per critic update in between); the next period's
    // first iteration with + ahead -- the values their own opening launches would use.
    x.role = chain_slot >= 0 ? "next-action passes ahead & next period's opening" : "next-action passes ahead";
    const float* Tk[3] = {e->Ta, e->Ta2, e->Ta3};
    RunAhead ra{e};
    for (int k = 1; k <= ahead; ++k) ra.add_next(k, Tk[k - 1], k - 1, k - 1, k - 1);
    if (chain_slot >= 0) {
      ra.add_next(chain_slot, Tk[ahead], ahead, ahead, ahead);
      ra.add_policy(chain_slot, ahead + 1, ahead, 0);                       // (TD3's policy pass draws nothing)
    }
    RCCHK(ra.launch(x, ahead));
  }
  x.role = (j & 1) ? "actor1/alpha" : "actor0/alpha";
  if (!td3) {
    if (c.autotune && merge_next) {
      // The temperature draw (agent.py:297-299) and the next actor update's policy sample (agent.py:254) both go through
      // the SAME freshly updated actor on the SAME observations: one trunk launch (with the next update's backward
      // stores and Adam tick) and one tail launch with two draws.  Streams: temperature (ctr, 32), policy (ctr + 1, 16),
      // exactly what the two separate launches would consume.
      const TrunkGrp g{SX, e->Pa, e->a_z1, e->a_z2, e->a_xh1, e->a_h1, e->a_rs1};
      const int sb_a_next = SACTD3_SITE_ACTOR0 + ((j + 1) & 1);
      TrunkTicks tk{&e->ctl->t_a, nullptr, e->ctl->adam_a, e->ctl->pw_a, c.actor_lr};
      bool eps_ready = false;
      tk.nnoise = 2; tk.noise[0] = noise_job(e, sb_a_next, 16u, 1, B); tk.noise[1] = noise_job(e, sb_l, 32u, 0, B); tk.noise_taken = &eps_ready;
      RCCHK(enqueue_trunk(x, e->ldc, e->o, B, e->La, 0, 1, 1, &g, tk));
      ActorTail t = tail_args(e, e->a_z2, e->Pa, B, 0, 1, sb_a_next, 16u, e->Xp, e->ldc, e->o, e->logp_pi);
      t.obs_src = SX; t.lds = e->ldc; t.ctr_add = 1;
      t.dual = 1; t.site_buf2 = sb_l; t.site_code2 = 32u; t.eps2 = e->eps[sb_l]; t.logp2 = e->logp_al;
      t.eps_ready = eps_ready;
      RCCHK(launch_tail(x, t));
    } else if (c.autotune) {  // fresh draw through the already-updated actor (agent.py:297-299): group 0 / tail 0 of the pair ...
      RunAhead ra{e};
      ra.g[0] = TrunkGrp{SX, e->Pa, e->a_z1, e->a_z2, nullptr, nullptr, nullptr};
      ra.tk.noise[ra.tk.nnoise++] = noise_job(e, sb_l, 32u, 0, B);
      ra.t[0] = tail_args(e, e->a_z2, e->Pa, B, 0, 0, sb_l, 32u, e->act_scratch, e->a4, 0, e->logp_al);
      ra.n = 1;
      // ... that also holds the run-ahead (SAC, pipelined period).  The noise counter stands at N + (this update's index + 1) here
      // (one tick by the critic update, one per finished temperature step), the sample counter already counts this iteration.
      // Iteration k of the period (k = 1 .. ahead): its sample is the one drawn with sample_ctr + (k - 1), its critic-site draws those
      // of noise counter + k (the tick owed by this update's deferred temperature step, one per critic update in between) -- exactly
      // what its own opening launches would have used.
      for (int k = 1; k <= ahead; ++k) ra.add_next(k, e->Pa, k - 1, k - 1, k);
      // ... and the opening pair of the NEXT period's first iteration, into batch slot `chain_slot`: sample sample_ctr + ahead,
      // critic-site draws of noise counter + ahead + 1 (where that period starts), policy draws (site 16) one further -- the values
      // its own opening launches use (enqueue_opening_pair: merge_policy)
      if (chain_slot >= 0) {
        ra.add_next(chain_slot, e->Pa, 2, ahead, ahead + 1);
        ra.add_policy(chain_slot, 3, ahead, ahead + 2);
      }
      if (ra.n > 1) x.role = chain_slot >= 0 ? "alpha & next-action passes ahead & next period's opening" : "alpha & next-action passes ahead";
      RCCHK(ra.launch(x, ahead));
    }
    AlphaArgs al{};
    al.logp = e->logp_al; al.B = B; al.targ_ent = -(float)e->a; al.autotune = c.autotune; al.la = e->la; al.ctl = e->ctl;
    al.lr = c.log_alpha_lr; al.b1 = c.adam_beta1; al.b2 = c.adam_beta2; al.eps = c.adam_eps; al.tick = &e->ctl->noise_ctr;
    if (merge_next) { x.alpha = al; x.alpha_pending = true; }   // rides in the next update's critic-trunk launch
    else if (defer_alpha) { al.tick = nullptr; x.alpha = al; x.alpha_pending = true; x.alpha_tick_owed = true; }
    else {
      LAUNCH("k_alpha_step", 0.0, 4.0 * B, k_alpha_step, dim3(1), dim3(256), al);
    }
  }
  return 0;
}

// agents/agent.py:328-331
enum { POLYAK_CRITICS = 1, POLYAK_ACTOR = 2 };
static int enqueue_polyak(EnqCtx& x, int which) {
  sactd3_engine* e = x.e;
  x.role = "targets";
  PolyakArgs p{};
  p.tau = e->cfg.polyak;
  if (which & POLYAK_CRITICS) { p.t0 = e->Tc; p.p0 = e->Pc; p.n0 = 2L * e->Lc.size; }
  if (which & POLYAK_ACTOR) { p.t1 = e->Ta; p.p1 = e->Pa; p.n1 = e->La.size; }
  const long n = p.n0 + p.n1;
  if (n == 0) return 0;
  LAUNCH("k_polyak", 0.0, 12.0 * n, k_polyak, dim3((unsigned)std::min<long>(512, (n / 4 + 255) / 256)), dim3(256), p);
  return 0;
}

// orchestrator.py:337-352 as one sequence (see IterPlace)
static int enqueue_step(EnqCtx& x, const IterPlace& it) {
  sactd3_engine* e = x.e;
  const bool td3 = e->cfg.prefer_td3_over_sac;
  x.role = "sample";
  if (!it.pre_sampled && !opening_trunk_gathers(e)) RCCHK(enqueue_gather(x, e->ring, -1));   // otherwise the gather is inside the first trunk kernel
  // Target updates (agents/agent.py:320-331) are folded into the kernels that apply the optimiser steps: the critic targets are
  // lerped towards the freshly stepped critics inside the critics' Adam epilogue (same element, same order as :328 after :236;
  // nothing between there and the end of the iteration reads the targets).  TD3 also moves the actor target every iteration:
  // in the last actor update's Adam epilogue when the iteration has actor updates, otherwise -- the actor did not change -- as a
  // few extra blocks of the critics' weight-gradient launch.
  RCCHK(enqueue_update_qnets(x, it, true));
  if (it.actor)
    for (int j = 0; j < e->cfg.actor_update_delay; ++j) RCCHK(enqueue_update_actor(x, it, j, true));
  else if (it.targets && td3 && !actor_target_rides(e)) RCCHK(enqueue_polyak(x, POLYAK_ACTOR));
  return 0;
}

// launch == false: capture + instantiate only (sactd3_instantiate_graphs); on: the stream to capture and launch on (default: the learner's)
template <class F>
static int run_graph_slot(sactd3_engine* e, hipGraphExec_t* slot, int* nodes, F&& enqueue, bool launch = true, hipStream_t on = nullptr) {
  const hipStream_t st = on ? on : e->stream;
  auto sequence = [&]() { EnqCtx x{e, st}; return enqueue_end(x, enqueue(x)); };      // a context per sequence: begins and ends here
  if (!e->cfg.use_graphs) return launch ? sequence() : 0;
  if (!*slot) {
    hipGraph_t g = nullptr;
    HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    const int rc = sequence();
    hipError_t he = hipStreamEndCapture(st, &g);
    if (rc != 0) { if (g) hipGraphDestroy(g); return rc; }
    if (he != hipSuccess) return e->fail(SACTD3_EHIP, "hipStreamEndCapture", he);
    size_t n = 0;
    HIPCHK(hipGraphGetNodes(g, nullptr, &n));
    if (nodes) *nodes = (int)n;
    he = hipGraphInstantiate(slot, g, nullptr, nullptr, 0);
    hipGraphDestroy(g);
    if (he != hipSuccess) return e->fail(SACTD3_EHIP, "hipGraphInstantiate", he);
    // move the executable graph's launch resources to the device now, not inside its first launch (a loop that instantiates ahead --
    // sactd3_instantiate_graphs -- then pays nothing extra the first time each graph runs); not every runtime implements it: best effort
    if (hipGraphUpload(*slot, st) != hipSuccess) (void)hipGetLastError();
  }
  if (launch) HIPCHK(hipGraphLaunch(*slot, st));
  return 0;
}
// The learner graphs and the rollout cycle's live in one table, sactd3_engine::graphs, keyed by the G_* ids; enqueue_graph (below the sequences it names) is
// the one place that says which sequence an id holds, so an id cannot be captured with one sequence here and another there.
static int enqueue_graph(EnqCtx& x, int which);
static int run_graph(sactd3_engine* e, int which, bool launch = true) {
  const bool had = e->graphs[which] != nullptr;
  RCCHK(run_graph_slot(e, &e->graphs[which], &e->graph_nodes[which], [which](EnqCtx& x) { return enqueue_graph(x, which); }, launch));
  // whoever needs a graph first captures it (its entry point, sactd3_instantiate_graphs): the capture counters are kept here
  if (!had && e->graphs[which] && which >= G_RUN) ++*(which >= G_CYCLE ? &e->cyc.stats[1] : which >= G_SAMPLED ? &e->ss_stats[1] : &e->run_stats[3]);
  return 0;
}
// drop the graphs [first, first + count) of the table (an executable graph is not destroyed under its own replay: the stream drains first)
static int drop_graphs(sactd3_engine* e, int first, int count) {
  hipGraphExec_t* g = &e->graphs[first];
  if (std::count(g, g + count, nullptr) < count) HIPCHK(hipStreamSynchronize(e->stream));
  for (int i = 0; i < count; ++i) {
    if (g[i]) hipGraphExecDestroy(g[i]);
    g[i] = nullptr; e->graph_nodes[first + i] = 0;
  }
  return 0;
}

// A learner-stream call that writes the actor parameters (what the acting kernels read through that stream) is about to be issued:
// if an acting call is in flight on the acting stream, the learner stream first waits for an event recorded behind its launches, so
// the parameters are not overwritten under a running predict; and the next sactd3_predict_begin has to wait for this call.
static int actor_write_begin(sactd3_engine* e) {
  e->actor_dirty = true;
  if (!e->act_inflight || e->act_ordered) return 0;      // (once predict_end has returned the host knows the kernels are done)
  HIPCHK(hipEventRecord(e->ev_acting, e->act_stream));
  HIPCHK(hipStreamWaitEvent(e->stream, e->ev_acting, 0));
  e->act_ordered = true;
  ++e->act_stats[2];
  return 0;
}

static int set_flag(EnqCtx& x, int* dst, int v) {
  LAUNCH_ON(k_set_int1, dim3(1), dim3(1), dst, v);
  return 0;
}
// ctl->rb_len and ctl->rb_cursor are adjacent ints
static int publish_rb_state(EnqCtx& x) { return launch_set_int2(x, &x.e->ctl->rb_len, (int)x.e->rb_len, (int)x.e->rb_cursor); }
// THE cursor arithmetic of every append path (sactd3_rb_extend, _extend_device, _extend_fields_device).  With P = rb_pinned the
// appends go round-robin over [P, cap): the ingest kernels take (ring, cursor, cap) as launch arguments and are told the ring advanced
// by P records, the cursor relative to P and the region's size cap - P -- with P == 0 exactly what they were told before.
// ring_region: the most rows one launch may append.  ring_append: moves the host's cursor and length over `chunk` <= ring_region rows
// and returns what the launch is told; new_len / new_cursor (what the kernel publishes into DevCtl) keep their absolute meaning.
struct RingSpan { float4* ring; int cursor, cap; int first /* absolute slot of the first row written */, new_len, new_cursor; };
static inline int64_t ring_region(const sactd3_engine* e) { return (int64_t)e->cfg.rb_capacity - e->rb_pinned; }
static RingSpan ring_append(sactd3_engine* e, int chunk) {
  const int64_t cap = e->cfg.rb_capacity, P = e->rb_pinned, region = cap - P, rel = e->rb_cursor - P;
  RingSpan s{};
  s.ring = (float4*)e->ring + (size_t)P * e->rec4; s.cursor = (int)rel; s.cap = (int)region; s.first = (int)e->rb_cursor;
  if (e->rb_len + chunk > cap) e->rb_wrapped = true;             // a row is being overwritten
  if (P > 0 && rel + chunk >= region) ++e->mix_stats[3];         // the cursor comes back to P, not to 0
  e->rb_cursor = P + (rel + chunk) % region;
  e->rb_len = std::min<int64_t>(cap, e->rb_len + chunk);
  s.new_len = (int)e->rb_len; s.new_cursor = (int)e->rb_cursor;
  return s;
}

// ------------------------------------------------------------------------------------------------ ring rows into batch slot 0: launches
// Launches of the staging calls (stage_ring_rows, in the replay-buffer part of the C ABI below) and of the engine-owned priorities
// (device code: prio_kernels.h, nstep_kernels.h).  They stand in front of the extern "C" block, where a helper may be a template.
static int slot_weights_alloc(sactd3_engine* e) {      // (never zeroed: every staging kernel writes all B entries before anything reads them)
  return first_use_alloc(e, &e->bs[0].w, (size_t)e->B, false);
}
static int nstep_alloc(sactd3_engine* e) {
  RCCHK(first_use_alloc(e, &e->ns_k, (size_t)e->B));
  RCCHK(first_use_alloc(e, &e->ns_last, (size_t)e->B));
  return first_use_alloc(e, &e->ns_ctr, 32);
}
// What k_batch_from_index and k_batch_from_index_nstep are both told (IndexBatchArgs and NstepArgs name these fields alike): the ring's
// geometry, the index and weight sources, slot 0's arrays, the magic divisor.  Returns the gather's span: chunks per thread over
// gather_blocks(B * rec4) blocks.
template <class Args>
static long ring_rows_args(sactd3_engine* e, Args& g, const long long* idx, int64_t idx_ld, const float* w, int64_t w_ld, float* wdst) {
  const sactd3_engine::BatchSlot& S = e->bs[0];
  g.ring = (const float4*)e->ring; g.rec4 = e->rec4; g.cx = e->cx; g.cn = e->cn; g.B = e->B; g.len = (int)e->rb_len;
  g.idx = idx; g.idx_ld = (long)idx_ld; g.w = w; g.w_ld = (long)w_ld;
  g.X = (float4*)S.X; g.Xn = (float4*)S.Xn; g.rew = S.rew; g.done = S.done; g.slot_idx = S.idx; g.wdst = wdst;
  const long chunks = (long)e->B * e->rec4;      // (< 2^31: create_impl)
  g.rec4_magic = magic_div((unsigned)e->rec4, (unsigned long long)chunks + 1);
  const unsigned blocks = gather_blocks(chunks);
  return (chunks + 256L * blocks - 1) / (256L * blocks);
}
// the 1-step kernel: it always writes the slot's weights (w == NULL: 1).  (Here and in the launchers below: EnqCtx::graph_form picks
// the kernel instance.)
static int launch_batch_index(EnqCtx& x, const long long* idx, int64_t idx_ld, const float* w, int64_t w_ld) {
  sactd3_engine* e = x.e;
  IndexBatchArgs g{};
  g.cpb = (int)ring_rows_args(e, g, idx, idx_ld, w, w_ld, e->bs[0].w);
  g.refused = &e->ctl->priority_refused;
  const dim3 grid(gather_blocks((long)e->B * e->rec4));
  if (x.graph_form) LAUNCH_ON(k_batch_from_index_g, grid, dim3(256), IndexBatchArgsG{g, e->ctl, (int)e->cfg.rb_capacity});
  else LAUNCH_ON(k_batch_from_index, grid, dim3(256), g);
  return 0;
}
// idx == NULL: the uniform draw at the current sample counter; wdst: the slot's weight array, or NULL for a slot without weights
static int launch_batch_nstep(EnqCtx& x, const long long* idx, int64_t idx_ld, const float* w, int64_t w_ld, float* wdst, int steps, int stride) {
  sactd3_engine* e = x.e;
  NstepArgs g{};
  const long cpb_g = ring_rows_args(e, g, idx, idx_ld, w, w_ld, wdst);
  g.o = e->o; g.cursor = (int)e->rb_cursor; g.cap = (int)e->cfg.rb_capacity;
  g.steps = steps; g.stride = stride; g.gamma = e->cfg.gamma; g.ctl = e->ctl;
  g.nk = e->ns_k; g.nlast = e->ns_last;
  // the gather's grid, with the span cut so that a block's rows fit its LDS tables: (cpb * 256) / rec4 + 2 <= NS_ROWS
  const long chunks = (long)e->B * e->rec4, cpb_l = std::max(1L, (long)(NS_ROWS - 2) * e->rec4 / 256);
  g.cpb = (int)std::min(cpb_g, cpb_l);
  if ((256L * g.cpb) / e->rec4 + 2 > NS_ROWS) return e->fail(SACTD3_EINVAL, "n-step staging: the record is too short for the kernel's row tables");
  const unsigned blocks = (unsigned)((chunks + 256L * g.cpb - 1) / (256L * g.cpb));
  g.counters = e->ns_ctr;
  if (x.graph_form) LAUNCH_ON(k_batch_from_index_nstep_g, dim3(blocks), dim3(256), g);
  else LAUNCH_ON(k_batch_from_index_nstep, dim3(blocks), dim3(256), g);
  return 0;
}
static int launch_batch_weights(EnqCtx& x, const float* w, int64_t w_ld) {
  sactd3_engine* e = x.e;
  const WeightArgs g{w, (long)w_ld, e->bs[0].idx, e->bs[0].w, e->B, &e->ctl->priority_refused};
  LAUNCH_ON(k_batch_weights, dim3((unsigned)((e->B + 255) / 256)), dim3(256), g);
  return 0;
}
static int launch_td_out(EnqCtx& x, float* td, int64_t td_ld, int64_t td_ns) {
  sactd3_engine* e = x.e;
  const TdArgs g{e->q, e->y, e->B, td, (long)td_ld, (long)td_ns};
  LAUNCH_ON(k_td_to_field, dim3((unsigned)((e->B + 255) / 256)), dim3(256), g);
  return 0;
}
// rows [first, first + n) of the ring, wrapping at the capacity, have just been written: they enter at the maximum priority
static int prio_refresh(EnqCtx& x, int64_t first, int64_t n) {
  sactd3_engine* e = x.e;
  const int64_t cap = e->cfg.rb_capacity;
  PrioRefreshArgs g{};
  g.leaf = e->pt_leaf; g.sums = e->pt_sums; g.pc = e->pt_ctl; g.alpha = e->pt_alpha;
  if (n >= cap) { first = 0; n = cap; }
  g.lo0 = (int)first; g.hi0 = (int)std::min(first + n, cap);
  g.lo1 = 0; g.hi1 = (int)std::max<int64_t>(first + n - cap, 0);
  g.g0 = g.lo0 / PRIO_G; g.n0 = (g.hi0 - 1) / PRIO_G - g.g0 + 1;
  g.g1 = 0;
  const int n1 = g.hi1 > 0 ? (g.hi1 - 1) / PRIO_G + 1 : 0;
  LAUNCH_ON(k_prio_refresh, dim3((unsigned)(g.n0 + n1)), dim3(256), g);
  e->pt_host[2] += n;
  return 0;
}
// (nothing is launched while priorities are off)
static int prio_after_append(EnqCtx& x, int64_t first, int64_t n) {
  return (x.e->pt_on && n > 0) ? prio_refresh(x, first, n) : 0;
}
// the two launches of a prioritised draw: slots and leaves, then weights (+ counter tick); the staging kernel follows (draw_launches)
static int prio_draw_launches(EnqCtx& x, float beta) {
  sactd3_engine* e = x.e;
  if (x.graph_form) beta = 0.f;      // (read from PrioCtl on the device: a captured node holds no value of it)
  PrioDrawArgs d{};
  d.leaf4 = (const float4*)e->pt_leaf; d.sums4 = (const float4*)e->pt_sums;
  d.ngroups = e->pt_groups; d.nch = (e->pt_groups + PRIO_G - 1) / PRIO_G; d.len = (int)e->rb_len;
  d.u_inj = (x.graph_form || e->pt_inject) ? e->pt_u : nullptr; d.ctl = e->ctl; d.pc = e->pt_ctl;
  d.idx_out = e->pt_idx; d.leaf_out = e->pt_dleaf; d.total_out = e->pt_total;
  const int cap = (int)e->cfg.rb_capacity;
  if (x.graph_form) LAUNCH_ON(k_prio_draw_g, dim3((unsigned)e->B), dim3(256), PrioDrawArgsG{d, cap});
  else LAUNCH_ON(k_prio_draw, dim3((unsigned)e->B), dim3(256), d);
  const PrioWeightArgs w{e->pt_idx, e->pt_dleaf, e->pt_total, e->pt_w, e->B, (float)e->rb_len, beta, e->pt_inject ? nullptr : &e->pt_ctl->draw_ctr};
  if (x.graph_form) LAUNCH_ON(k_prio_weights_g, dim3(1), dim3(256), PrioWeightArgsG{w, e->ctl, e->pt_ctl, cap});
  else LAUNCH_ON(k_prio_weights, dim3(1), dim3(256), w);
  return 0;
}
static int launch_prio_update(EnqCtx& x, PrioUpdateArgs g) {
  sactd3_engine* e = x.e;
  g.leaf = e->pt_leaf; g.sums = e->pt_sums; g.len = (int)e->rb_len; g.alpha = e->pt_alpha; g.eps = e->pt_eps; g.pc = e->pt_ctl;
  if (x.graph_form) LAUNCH_ON(k_prio_update_g, dim3((unsigned)g.n), dim3(256), PrioUpdateArgsG{g, e->ctl, (int)e->cfg.rb_capacity});
  else LAUNCH_ON(k_prio_update, dim3((unsigned)g.n), dim3(256), g);
  return 0;
}
// the TD form of the write-back: the rows of batch slot `slot` and the TD errors of the critic update that ran on them
static PrioUpdateArgs prio_td_args(sactd3_engine* e, int slot) {
  PrioUpdateArgs g{};
  g.n = e->B; g.slot_idx = e->bs[slot].idx; g.q = e->q; g.y = e->y; g.B = e->B;
  return g;
}

// ---- the mixed draw (device code: mix_kernels.h)
static int mix_alloc(sactd3_engine* e) {
  RCCHK(first_use_alloc(e, &e->mix_idx, (size_t)round_up(e->B, 4)));
  return first_use_alloc(e, &e->mix_ctl, 1);
}
// what a mixed draw needs of the ring, checked on the host, which knows len, P and m (NULL: nothing to refuse)
static const char* mix_refusal(const sactd3_engine* e) {
  if (e->rb_len <= 0) return "buffer is empty";
  if (e->mix_m > 0 && e->rb_pinned == 0) return "prior rows were asked for (sactd3_rb_set_mix) but no row is pinned (sactd3_rb_pin)";
  if (e->mix_m < e->B && e->rb_len == e->rb_pinned) return "live rows were asked for but every row of the ring is pinned";
  return nullptr;
}
// the device's copy of P and m, for the graph form: one single-thread launch, and only when a value changed
static int mix_publish(EnqCtx& x) {
  sactd3_engine* e = x.e;
  if (e->mix_pub[0] == e->rb_pinned && e->mix_pub[1] == e->mix_m) return 0;
  RCCHK(launch_set_int2(x, &e->mix_ctl->pinned, (int)e->rb_pinned, e->mix_m));
  e->mix_pub[0] = e->rb_pinned; e->mix_pub[1] = e->mix_m;
  return 0;
}
// the draw of B slots into mix_idx, m of them from the P pinned rows (it advances the sample counter itself); P = m = 0: the uniform
// draw of sactd3_rb_sample.  The graph form reads P and m from mix_ctl.
static int launch_mix_draw(EnqCtx& x, int64_t P, int m) {
  sactd3_engine* e = x.e;
  const MixDrawArgs d{e->ctl, e->mix_idx, e->B, (int)e->rb_len, (int)P, m};
  if (x.graph_form) LAUNCH_ON(k_mix_draw<true>, dim3(1), dim3(256), d, (const MixCtl*)e->mix_ctl, (int)e->cfg.rb_capacity);
  else LAUNCH_ON(k_mix_draw<false>, dim3(1), dim3(256), d, (const MixCtl*)nullptr, 0);
  return 0;
}

// ---- hindsight relabelling (device code: hindsight_kernels.h, through the launcher of hindsight.h)
static int hindsight_alloc(sactd3_engine* e) {
  RCCHK(first_use_alloc(e, &e->hs_off, (size_t)e->B));
  RCCHK(first_use_alloc(e, &e->hs_gs, (size_t)e->B));
  return first_use_alloc(e, &e->hs_ctr, HS_WORDS);
}
// what both forms of the staging kernel are told: the ring's geometry as ring_rows_args states it, everything else by value.  Returns
// the grid.
static unsigned hindsight_args(sactd3_engine* e, HindsightArgs& g, const long long* idx, int64_t idx_ld, const int* choice, int64_t choice_ld,
                               unsigned hctr) {
  const sactd3_engine::BatchSlot& S = e->bs[0];
  const sactd3_hindsight_config& c = e->hs_cfg;
  g.ring = (const float4*)e->ring; g.rec4 = e->rec4; g.cx = e->cx; g.cn = e->cn; g.o = e->o;
  g.B = e->B; g.len = (int)e->rb_len; g.cursor = (int)e->rb_cursor; g.cap = (int)e->cfg.rb_capacity;
  g.ag_off = c.ag_off; g.dg_off = c.dg_off; g.G = c.goal_dim; g.thr = c.threshold; g.ratio = c.ratio; g.window = c.window; g.stride = c.stride;
  g.seed = e->cfg.seed; g.hctr = hctr;
  g.idx = idx; g.idx_ld = (long)idx_ld; g.choice = choice; g.choice_ld = (long)choice_ld;
  g.X = (float4*)S.X; g.Xn = (float4*)S.Xn; g.rew = S.rew; g.done = S.done; g.slot_idx = S.idx;
  g.offset = e->hs_off; g.goal_slot = e->hs_gs; g.counters = e->hs_ctr;
  const long chunks = (long)e->B * e->rec4;      // (< 2^31: create_impl)
  g.rec4_magic = magic_div((unsigned)e->rec4, (unsigned long long)chunks + 1);
  // the gather's grid, with the span cut so that a block's rows fit the kernel's LDS tables: (cpb * 256) / rec4 + 2 <= HS_ROWS
  const unsigned blocks_g = gather_blocks(chunks);
  const long cpb_g = (chunks + 256L * blocks_g - 1) / (256L * blocks_g), cpb_l = std::max(1L, (long)(HS_ROWS - 2) * e->rec4 / 256);
  g.cpb = (int)std::min(std::min(cpb_g, cpb_l), (long)HS_CPT);
  return (unsigned)((chunks + 256L * g.cpb - 1) / (256L * g.cpb));
}
// the one launch of k_hindsight_stage into batch slot 0
static int launch_hindsight(EnqCtx& x, const long long* idx, int64_t idx_ld, const int* choice, int64_t choice_ld, unsigned hctr) {
  sactd3_engine* e = x.e;
  HindsightArgs g{};
  const unsigned blocks = hindsight_args(e, g, idx, idx_ld, choice, choice_ld, hctr);
  const hipError_t he = hindsight_stage_launch(g, blocks, x.s);
  if (he != hipSuccess) return e->fail(SACTD3_EHIP, "hindsight_stage_launch", he);
  return 0;
}
// The graph forms (hindsight_kernels.h): the draw into mix_idx, which ticks the sample counter and the device's draw counter itself,
// then the staging of the drawn slots.  Ring length, cursor and draw counter are read on the device through the pointers given here;
// the config travels by value (sactd3_hindsight_configure drops the graphs that hold an earlier one).
static int hindsight_draw_launches_g(EnqCtx& x) {
  sactd3_engine* e = x.e;
  const HindsightDrawArgs d{&e->ctl->seed, &e->ctl->sample_ctr, &e->ctl->rb_len, e->hs_ctr, e->mix_idx, e->B, (int)e->cfg.rb_capacity};
  hipError_t he = hindsight_draw_g_launch(d, x.s);
  if (he != hipSuccess) return e->fail(SACTD3_EHIP, "hindsight_draw_g_launch", he);
  HindsightArgsG g{};
  const unsigned blocks = hindsight_args(e, g.a, e->mix_idx, 1, nullptr, 0, 0u);
  g.a.len = g.a.cursor = 0;      // (the device's, read by the kernel)
  g.ring_words = &e->ctl->rb_len; g.hs_words = e->hs_ctr;
  he = hindsight_stage_g_launch(g, blocks, x.s);
  if (he != hipSuccess) return e->fail(SACTD3_EHIP, "hindsight_stage_g_launch", he);
  return 0;
}
// the device's draw counter, for the graph form: one single-thread launch, and only when the host's count is not what the word holds
static int hindsight_publish(EnqCtx& x) {
  sactd3_engine* e = x.e;
  if (e->hs_pub == e->hs_calls) return 0;
  static_assert(HS_WORD_SNAPSHOT == HS_WORD_MASTER + 1, "the two words are set by one k_set_int2");
  RCCHK(launch_set_int2(x, e->hs_ctr + HS_WORD_MASTER, (int)e->hs_calls, (int)e->hs_calls));
  e->hs_pub = e->hs_calls;
  return 0;
}

// ---- struct Draw, each part said once: the call forms (stage_ring_rows, sactd3_rb_sample_mixed) and the captured iteration
// (sactd3_step_sampled, enqueue_step_sampled) are these four routines, in the protocol order of stage_ring_rows.
// What a draw needs of the ring and of the engine's features, checked on the host (NULL: nothing to refuse); the caller puts its own
// name in front (state_refusal).
static const char* const PRIO_OFF = "priorities are not enabled (sactd3_prio_enable)";
static const char* draw_state_refusal(const sactd3_engine* e, const Draw& d) {
  const bool hind = d.kind == SACTD3_DRAW_HINDSIGHT;
  if (d.kind == SACTD3_DRAW_PRIORITIZED && !e->pt_on) return PRIO_OFF;
  if (d.chain() && e->rb_pinned > 0) return "rows are pinned (sactd3_rb_pin): the n-step age formula assumes one wrap point, at slot 0";
  if (hind && !e->hs_on) return "hindsight is not configured (sactd3_hindsight_configure)";
  if (hind && e->rb_pinned > 0) return "rows are pinned (sactd3_rb_pin): the chain's age formula assumes one wrap point, at slot 0";
  if (e->rb_len <= 0) return "buffer is empty";
  return d.kind == SACTD3_DRAW_MIXED ? mix_refusal(e) : nullptr;
}
static int state_refusal(sactd3_engine* e, const char* who, const char* why) { e->err = std::string(who) + ": " + why; return SACTD3_ESTATE; }
// first-use allocations: an engine that never uses a feature holds nothing for it
static int draw_alloc(sactd3_engine* e, const Draw& d) {
  const bool hind = d.kind == SACTD3_DRAW_HINDSIGHT;
  if (!hind && (d.weighted() || !d.chain())) RCCHK(slot_weights_alloc(e));      // (the 1-step kernel always writes the slot's weights, the hindsight kernel none)
  if (d.chain()) RCCHK(nstep_alloc(e));
  if (!d.rows && (hind || d.kind == SACTD3_DRAW_MIXED)) RCCHK(mix_alloc(e));      // (where the draw kernel leaves the slots)
  return hind ? hindsight_alloc(e) : 0;
}
// the staging kernel on the rows `idx` [with the weights `w`]: one row each, or chained
static int launch_staging(EnqCtx& x, const Draw& d, const long long* idx, int64_t idx_ld, const float* w, int64_t w_ld) {
  if (d.chain()) return launch_batch_nstep(x, idx, idx_ld, w, w_ld, d.weighted() ? x.e->bs[0].w : nullptr, d.steps, d.stride);
  return launch_batch_index(x, idx, idx_ld, w, w_ld);
}
// The launches, in the call form or, with x.graph_form, the form a captured graph holds: the draw's own, then the staging of the drawn
// slots.  The mixed and hindsight draw kernels advance the sample counter themselves (the hindsight graph form its draw counter too); a
// uniform draw is made by the staging kernel at the sample counter, which a tick then advances.
static int draw_launches(EnqCtx& x, const Draw& d) {
  sactd3_engine* e = x.e;
  const bool hind = d.kind == SACTD3_DRAW_HINDSIGHT;
  if (const CallerRows* r = d.rows)
    return hind ? launch_hindsight(x, r->idx, r->idx_ld, r->choice, r->choice_ld, (unsigned)e->hs_calls) : launch_staging(x, d, r->idx, r->idx_ld, r->w, r->w_ld);
  if (d.kind == SACTD3_DRAW_PRIORITIZED) {      // the draw leaves slots and weights in pt_idx / pt_w
    RCCHK(prio_draw_launches(x, d.beta));
    return launch_staging(x, d, e->pt_idx, 1, e->pt_w, 1);
  }
  if (hind && x.graph_form) return hindsight_draw_launches_g(x);
  if (hind || d.kind == SACTD3_DRAW_MIXED) {      // hindsight: the uniform draw -- no pinned row, no prior share -- relabelled at the draw counter
    RCCHK(launch_mix_draw(x, hind ? 0 : e->rb_pinned, hind ? 0 : e->mix_m));
    return hind ? launch_hindsight(x, e->mix_idx, 1, nullptr, 1, (unsigned)e->hs_calls) : launch_batch_index(x, e->mix_idx, 1, nullptr, 1);
  }
  RCCHK(launch_staging(x, d, nullptr, 1, nullptr, 1));
  return launch_tick(x, &e->ctl->sample_ctr);
}
// The host state behind the launches: the slot, then each feature's counters (ns_host: {n-step stagings, rows staged}; hs_calls: where
// the kernel drew its own choices -- only the graph form's draw kernel has advanced the device's word as well, hs_pub; prio_stats[0]:
// index stagings of the caller's rows).
static void draw_issued(sactd3_engine* e, const Draw& d, bool graph_form) {
  const bool hind = d.kind == SACTD3_DRAW_HINDSIGHT;
  slot_refilled(e, d.weighted(), d.chain());
  e->slot.hindsight = hind;
  if (hind && !(d.rows && d.rows->choice)) { ++e->hs_calls; if (graph_form) ++e->hs_pub; }
  if (d.chain()) { ++e->ns_host[0]; e->ns_host[1] += e->B; }
  if (d.kind == SACTD3_DRAW_PRIORITIZED) ++e->pt_host[0];
  if (d.kind == SACTD3_DRAW_MIXED) { ++e->mix_stats[0]; e->mix_stats[1] += e->mix_m; e->mix_stats[2] += e->B - e->mix_m; }
  if (d.rows && !hind && !d.chain()) ++e->prio_stats[0];
}

// The replay-aware iteration (sactd3_step_sampled) as one linear sequence: what the calls
//   sactd3_rb_sample_prioritized[_nstep] | sactd3_rb_sample_nstep | sactd3_rb_sample_mixed | sactd3_rb_sample_hindsight -> sactd3_update_qnets ->
//   [sactd3_prio_update_from_td] -> [sactd3_update_actor x actor_update_delay] -> sactd3_update_targ_nets
// launch, launch for launch, with the staging and priority kernels in their graph forms.  (The 1-step uniform iteration is sactd3_step.)
static int enqueue_step_sampled(EnqCtx& x, bool actor, bool targets) {
  sactd3_engine* e = x.e;
  const bool prio = e->ss_draw.kind == SACTD3_DRAW_PRIORITIZED;
  RCCHK(draw_launches(x, e->ss_draw));
  IterPlace it;
  it.weighted = prio;
  RCCHK(enqueue_update_qnets(x, it, false));
  if (prio) RCCHK(launch_prio_update(x, prio_td_args(e, 0)));
  if (actor)
    for (int j = 0; j < e->cfg.actor_update_delay; ++j) RCCHK(enqueue_update_actor(x, IterPlace{}, 0, false));
  if (targets) RCCHK(enqueue_polyak(x, POLYAK_CRITICS | (e->cfg.prefer_td3_over_sac ? POLYAK_ACTOR : 0)));
  return 0;
}

// ------------------------------------------------------------------------------------------------ C ABI
#pragma GCC visibility push(default)
extern "C" {

int sactd3_abi_version(void) { return SACTD3_ABI_VERSION; }

int sactd3_get_config(const sactd3_engine* e, sactd3_config* out) {
  if (!e || !out) return SACTD3_EINVAL;
  *out = e->cfg;
  return 0;
}

void sactd3_default_config(sactd3_config* c, int td3) {
  memset(c, 0, sizeof(*c));
  c->abi_version = SACTD3_ABI_VERSION;
  c->batch_size = 256; c->rb_capacity = 1000000; c->max_envs = 4;
  c->prefer_td3_over_sac = td3 ? 1 : 0; c->layer_norm = 1; c->autotune = 1;
  c->bcq_style_targ_mix = td3 ? 1 : 0; c->targ_actor_smoothing = 1;
  c->actor_update_delay = 2; c->crit_targ_update_freq = 1; c->use_graphs = 1;
  c->actor_lr = 3e-4f; c->qnets_lr = td3 ? 3e-4f : 1e-3f; c->log_alpha_lr = 1e-3f;
  c->gamma = 0.99f; c->polyak = 0.005f; c->alpha_init = 0.2f; c->clip_norm = 0.f;
  c->td3_std = 0.2f; c->td3_c = 0.5f; c->actor_noise_std = 0.1f;
  c->adam_beta1 = 0.9f; c->adam_beta2 = 0.999f; c->adam_eps = 1e-8f;
}

const char* sactd3_last_error(const sactd3_engine* e) { return e ? e->err.c_str() : g_create_error.c_str(); }

void sactd3_destroy(sactd3_engine* e) {
  if (!e) return;
  if (e->stream) (void)hipSetDevice(e->cfg.device_id);   // (a failed create may carry a device_id that was never valid)
  if (e->stream) hipStreamSynchronize(e->stream);
  if (e->act_stream) hipStreamSynchronize(e->act_stream);
  (void)drop_graphs(e, 0, G_COUNT);
  for (auto& g : e->predict_graphs) if (g) hipGraphExecDestroy(g);
  for (auto& g : e->predict_dev_graphs) if (g) hipGraphExecDestroy(g);
  for (auto ev : e->events) hipEventDestroy(ev);
  for (void* p : e->dev_allocs) hipFree(p);
  for (void* p : e->host_allocs) hipHostFree(p);
  if (e->ev_learner) hipEventDestroy(e->ev_learner);
  if (e->ev_acting) hipEventDestroy(e->ev_acting);
  if (e->ev_src_ready) hipEventDestroy(e->ev_src_ready);
  if (e->ev_src_read) hipEventDestroy(e->ev_src_read);
  if (e->act_stream) hipStreamDestroy(e->act_stream);
  if (e->stream) hipStreamDestroy(e->stream);
  delete e;
}

static int create_impl(sactd3_engine* e, const float* min_ac, const float* max_ac) {
  const sactd3_config& c = e->cfg;
  if (c.abi_version != SACTD3_ABI_VERSION) return e->fail(SACTD3_EINVAL, "abi_version mismatch");
  if (c.ob_dim < 1 || c.ac_dim < 1 || c.ac_dim > 32) return e->fail(SACTD3_EINVAL, "ob_dim >= 1 and 1 <= ac_dim <= 32 required");
  if (c.batch_size < 1 || c.rb_capacity < 1 || c.max_envs < 1) return e->fail(SACTD3_EINVAL, "batch_size, rb_capacity, max_envs must be positive");
  if (c.actor_update_delay < 0 || c.crit_targ_update_freq < 1) return e->fail(SACTD3_EINVAL, "actor_update_delay >= 0 and crit_targ_update_freq >= 1 required");
  if (!min_ac || !max_ac) return e->fail(SACTD3_EINVAL, "min_ac / max_ac required");
  if (!(c.bc_alpha >= 0.f) || !std::isfinite(c.bc_alpha)) return e->fail(SACTD3_EINVAL, "bc_alpha must be finite and >= 0");
  if (c.bc_alpha > 0.f && !c.prefer_td3_over_sac) return e->fail(SACTD3_EINVAL, "bc_alpha > 0 needs a TD3 engine (prefer_td3_over_sac): SAC has no behaviour-cloning form");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return e->fail(SACTD3_ENODEV, "no HIP device visible");
  if (c.device_id < 0 || c.device_id >= ndev) return e->fail(SACTD3_EINVAL, "device_id out of range");
  HIPCHK(hipSetDevice(c.device_id));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, c.device_id));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return e->fail(SACTD3_ENODEV, "device is not gfx950 (this library carries gfx950 code objects only)");
  e->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  HIPCHK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));

  e->o = c.ob_dim; e->a = c.ac_dim; e->B = c.batch_size;
  const int td3 = c.prefer_td3_over_sac;
  e->nh = td3 ? e->a : 2 * e->a; e->ldu = round_up(e->nh, 4); e->a4 = round_up(e->a, 4);
  e->ldc = round_up(e->o + e->a, 4); e->ldo = round_up(e->o, 4);
  e->cx = e->ldc / 4; e->cn = e->ldo / 4;
  e->rec_f = round_up(e->ldc + e->ldo + 2, 16); e->rec4 = e->rec_f / 4;
  if ((long long)e->B * e->rec4 >= (1ll << 31)) return e->fail(SACTD3_EINVAL, "batch_size x record size too large");
  e->La = make_layout(e->o, e->nh); e->Lc = make_layout(e->o + e->a, 1);
  e->nq_actor = td3 ? 1 : 2;
  e->nblk = (e->B + 15) / 16; e->nblk4 = (e->B + 3) / 4;
  e->maxn = c.max_envs;
  e->stage_rows = std::max(c.max_envs, 256);
  const size_t B = e->B, BH = B * HID;

  RCCHK(dalloc(e, &e->ctl, 1));
  RCCHK(dalloc(e, &e->min_ac, e->a4)); RCCHK(dalloc(e, &e->max_ac, e->a4));
  RCCHK(dalloc(e, &e->scale, e->a4)); RCCHK(dalloc(e, &e->bias, e->a4));
  RCCHK(dalloc(e, &e->Pa, e->La.size)); RCCHK(dalloc(e, &e->Ta, e->La.size)); RCCHK(dalloc(e, &e->Ga, e->La.size));
  RCCHK(dalloc(e, &e->Ma, e->La.size)); RCCHK(dalloc(e, &e->Va, e->La.size));
  RCCHK(dalloc(e, &e->Ta2, e->La.size)); RCCHK(dalloc(e, &e->Ta3, e->La.size));
  RCCHK(dalloc(e, &e->Pc, 2 * e->Lc.size)); RCCHK(dalloc(e, &e->Tc, 2 * e->Lc.size)); RCCHK(dalloc(e, &e->Gc, 2 * e->Lc.size));
  RCCHK(dalloc(e, &e->Mc, 2 * e->Lc.size)); RCCHK(dalloc(e, &e->Vc, 2 * e->Lc.size));
  RCCHK(dalloc(e, &e->la, 4)); RCCHK(dalloc(e, &e->gscale, 4));
  RCCHK(dalloc(e, &e->ring, (size_t)c.rb_capacity * e->rec_f, false));
  RCCHK(dalloc(e, &e->stage_dev, B * e->rec_f));
  RCCHK(dalloc(e, &e->X, B * e->ldc)); RCCHK(dalloc(e, &e->Xn, B * e->ldc)); RCCHK(dalloc(e, &e->Xp, B * e->ldc));
  RCCHK(dalloc(e, &e->rew, B)); RCCHK(dalloc(e, &e->done, B)); RCCHK(dalloc(e, &e->idx, B));
  RCCHK(dalloc(e, &e->logp_n, B)); RCCHK(dalloc(e, &e->logp_pi, B)); RCCHK(dalloc(e, &e->logp_al, B));
  RCCHK(dalloc(e, &e->act_scratch, B * e->a4));
  for (int s = 0; s < SACTD3_NUM_SITES; ++s)
    RCCHK(dalloc(e, &e->eps[s], std::max<size_t>(B, e->maxn) * e->a));
  RCCHK(dalloc(e, &e->a_z1, BH)); RCCHK(dalloc(e, &e->a_xh1, BH)); RCCHK(dalloc(e, &e->a_h1, BH)); RCCHK(dalloc(e, &e->a_rs1, B));
  RCCHK(dalloc(e, &e->a_z2, BH)); RCCHK(dalloc(e, &e->a_xh2, BH)); RCCHK(dalloc(e, &e->a_h2, BH)); RCCHK(dalloc(e, &e->a_rs2, B));
  RCCHK(dalloc(e, &e->a_tg, B * 4 * e->a4)); RCCHK(dalloc(e, &e->a_du, B * e->ldu)); RCCHK(dalloc(e, &e->a_z2n, BH));
  e->bs[0] = {e->X, e->Xn, e->rew, e->done, e->logp_n, e->eps[SACTD3_SITE_CRITIC], e->idx};
  for (int k = 0; k < 4; ++k) { RCCHK(dalloc(e, &e->ah_z1[k], BH)); RCCHK(dalloc(e, &e->ah_z2[k], BH)); }
  for (int k = 1; k < 4; ++k) {
    sactd3_engine::BatchSlot& S = e->bs[k];
    RCCHK(dalloc(e, &S.X, B * e->ldc)); RCCHK(dalloc(e, &S.Xn, B * e->ldc)); RCCHK(dalloc(e, &S.rew, B)); RCCHK(dalloc(e, &S.done, B));
    RCCHK(dalloc(e, &S.logp_n, B)); RCCHK(dalloc(e, &S.eps_c, std::max<size_t>(B, e->maxn) * e->a)); RCCHK(dalloc(e, &S.idx, B));
  }
  RCCHK(dalloc(e, &e->a_dz2, BH)); RCCHK(dalloc(e, &e->a_dh1, BH)); RCCHK(dalloc(e, &e->a_dz1, BH));
  RCCHK(dalloc(e, &e->qa_ps, 2L * B * 256)); RCCHK(dalloc(e, &e->qa_S, 2L * 16 * 8));
  RCCHK(dalloc(e, &e->a_ps, (long)B * PS_W + HID)); RCCHK(dalloc(e, &e->c_ps, 2L * B * PS_W + 2 * HID));   // (+ the gamma1 snapshot behind them)
  RCCHK(dalloc(e, &e->c_z1, 2 * BH)); RCCHK(dalloc(e, &e->c_xh1, 2 * BH)); RCCHK(dalloc(e, &e->c_h1, 2 * BH)); RCCHK(dalloc(e, &e->c_rs1, 2 * B));
  RCCHK(dalloc(e, &e->c_z2, 2 * BH)); RCCHK(dalloc(e, &e->c_dz2, 2 * BH)); RCCHK(dalloc(e, &e->c_dh1, 2 * BH)); RCCHK(dalloc(e, &e->c_dz1, 2 * BH));
  RCCHK(dalloc(e, &e->t_z1, 2 * BH)); RCCHK(dalloc(e, &e->t_z2, 2 * BH));
  RCCHK(dalloc(e, &e->q, 2 * B)); RCCHK(dalloc(e, &e->qt, 2 * B)); RCCHK(dalloc(e, &e->y, B)); RCCHK(dalloc(e, &e->q_pi, 2 * B));
  RCCHK(dalloc(e, &e->dA, 2 * B * e->a4));
  if (e->B >= BIG_BATCH) RCCHK(dalloc(e, &e->s_h1, 4 * BH));
  if (e->B >= BIG_BATCH) {
    e->gp_slabs = 8;
    RCCHK(dalloc(e, &e->Gp, (size_t)e->gp_slabs * std::max<size_t>(2 * (size_t)e->Lc.size, e->La.size)));
  }
  RCCHK(dalloc(e, &e->part, 2 * (size_t)e->nblk4 * NSLOT * HID)); RCCHK(dalloc(e, &e->part_s, 2 * (size_t)e->nblk4 * 2)); RCCHK(dalloc(e, &e->part_sa, (size_t)e->nblk4 * 2));
  e->bc_on = c.bc_alpha > 0.f; e->bc_alpha = c.bc_alpha; e->bc_weight = 1.f;
  if (e->bc_on) RCCHK(dalloc(e, &e->bc_part, (size_t)e->nblk4));
  RCCHK(dalloc(e, &e->p_x, (size_t)e->maxn * e->ldo)); RCCHK(dalloc(e, &e->p_z1, (size_t)e->maxn * HID));
  RCCHK(dalloc(e, &e->p_z2, (size_t)e->maxn * HID)); RCCHK(dalloc(e, &e->p_act, (size_t)e->maxn * e->a4));
  RCCHK(halloc(e, &e->h_obs, (size_t)e->maxn * e->ldo)); RCCHK(halloc(e, &e->h_act, (size_t)e->maxn * e->a4));
  RCCHK(halloc(e, &e->h_done, 4));
  RCCHK(halloc(e, &e->h_batch, B * e->rec_f));
  for (int i = 0; i < NSTAGE; ++i) {
    RCCHK(halloc(e, &e->h_stage[i], (size_t)e->stage_rows * e->rec_f));
  }

  std::vector<float> hb(4 * e->a4, 0.f);
  for (int j = 0; j < e->a; ++j) {
    hb[j] = min_ac[j]; hb[e->a4 + j] = max_ac[j];
    hb[2 * e->a4 + j] = (max_ac[j] - min_ac[j]) / 2.0f;   // agents/nets.py:133-136
    hb[3 * e->a4 + j] = (max_ac[j] + min_ac[j]) / 2.0f;
  }
  HIPCHK(hipMemcpy(e->min_ac, hb.data(), sizeof(float) * e->a4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->max_ac, hb.data() + e->a4, sizeof(float) * e->a4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->scale, hb.data() + 2 * e->a4, sizeof(float) * e->a4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->bias, hb.data() + 3 * e->a4, sizeof(float) * e->a4, hipMemcpyHostToDevice));
  DevCtl hc{};
  hc.seed = c.seed;
  hc.pw_q[0] = hc.pw_q[1] = hc.pw_a[0] = hc.pw_a[1] = hc.pw_l[0] = hc.pw_l[1] = 1.0;
  hc.bc[0] = e->bc_alpha; hc.bc[1] = e->bc_weight;
  HIPCHK(hipMemcpy(e->ctl, &hc, sizeof(hc), hipMemcpyHostToDevice));
  const float la0[4] = {logf(c.alpha_init), 0.f, 0.f, 0.f};   // agents/agent.py:128
  HIPCHK(hipMemcpy(e->la, la0, sizeof(la0), hipMemcpyHostToDevice));
  // LN gamma = 1 (agents/nets.py:44-47); weights stay 0 until sactd3_set_params
  {
    std::vector<float> ha(e->La.size, 0.f), hq(2 * (size_t)e->Lc.size, 0.f);
    std::fill(ha.begin() + e->La.g1, ha.begin() + e->La.g1 + HID, 1.f);
    std::fill(ha.begin() + e->La.g2, ha.begin() + e->La.g2 + HID, 1.f);
    for (int i = 0; i < 2; ++i) {
      std::fill(hq.begin() + i * e->Lc.size + e->Lc.g1, hq.begin() + i * e->Lc.size + e->Lc.g1 + HID, 1.f);
      std::fill(hq.begin() + i * e->Lc.size + e->Lc.g2, hq.begin() + i * e->Lc.size + e->Lc.g2 + HID, 1.f);
    }
    HIPCHK(hipMemcpy(e->Pa, ha.data(), sizeof(float) * ha.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->Ta, ha.data(), sizeof(float) * ha.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->Pc, hq.data(), sizeof(float) * hq.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->Tc, hq.data(), sizeof(float) * hq.size(), hipMemcpyHostToDevice));
  }
  HIPCHK(hipDeviceSynchronize());
  return 0;
}

int sactd3_create(const sactd3_config* cfg, const float* min_ac, const float* max_ac, sactd3_engine** out) {
  if (!cfg || !out) { g_create_error = "null argument"; return SACTD3_EINVAL; }
  *out = nullptr;
  sactd3_engine* e = new sactd3_engine();
  e->cfg = *cfg;
  const int rc = create_impl(e, min_ac, max_ac);
  if (rc != 0) { g_create_error = e->err; sactd3_destroy(e); return rc; }
  *out = e;
  return 0;
}

// ---- parameters
static bool which_arena(sactd3_engine* e, int which, float** P, float** M, float** V, const NetLayout** L, int* nets, int** t) {
  switch (which) {
    case SACTD3_ACTOR: *P = e->Pa; *M = e->Ma; *V = e->Va; *L = &e->La; *nets = 1; *t = &e->ctl->t_a; return true;
    case SACTD3_CRITICS: *P = e->Pc; *M = e->Mc; *V = e->Vc; *L = &e->Lc; *nets = 2; *t = &e->ctl->t_q; return true;
    case SACTD3_ACTOR_TARGET: *P = e->Ta; *M = *V = nullptr; *L = &e->La; *nets = 1; *t = nullptr; return true;
    case SACTD3_CRITICS_TARGET: *P = e->Tc; *M = *V = nullptr; *L = &e->Lc; *nets = 2; *t = nullptr; return true;
    default: return false;
  }
}

int64_t sactd3_param_count(const sactd3_engine* e, int which) {
  if (!e) return SACTD3_EINVAL;
  switch (which) {
    case SACTD3_ACTOR: case SACTD3_ACTOR_TARGET: return ref_count(e->La, e->cfg.layer_norm);
    case SACTD3_CRITICS: case SACTD3_CRITICS_TARGET: return 2 * ref_count(e->Lc, e->cfg.layer_norm);
    case SACTD3_LOG_ALPHA: return 1;
    default: return SACTD3_EINVAL;
  }
}

static int read_arena(sactd3_engine* e, const float* dev, const NetLayout& L, int nets, float* dst) {
  std::vector<float> h((size_t)nets * L.size);
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(h.data(), dev, sizeof(float) * h.size(), hipMemcpyDeviceToHost));
  const int64_t rc = ref_count(L, e->cfg.layer_norm);
  for (int i = 0; i < nets; ++i) unpack_net(L, e->cfg.layer_norm, h.data() + (size_t)i * L.size, dst + i * rc);
  return 0;
}
static int write_arena(sactd3_engine* e, float* dev, const NetLayout& L, int nets, const float* src, bool is_param) {
  std::vector<float> h((size_t)nets * L.size);
  const int64_t rc = ref_count(L, e->cfg.layer_norm);
  for (int i = 0; i < nets; ++i) pack_net(L, e->cfg.layer_norm, src + i * rc, h.data() + (size_t)i * L.size, is_param);
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(dev, h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice));
  return 0;
}

int sactd3_get_params(sactd3_engine* e, int which, float* dst) {
  if (!e || !dst) return SACTD3_EINVAL;
  USE_DEVICE(e);
  if (which == SACTD3_LOG_ALPHA) {
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(dst, e->la, sizeof(float), hipMemcpyDeviceToHost));
    return 0;
  }
  float *P, *M, *V; const NetLayout* L; int nets; int* t;
  if (!which_arena(e, which, &P, &M, &V, &L, &nets, &t)) return e->fail(SACTD3_EINVAL, "bad `which`");
  return read_arena(e, P, *L, nets, dst);
}

int sactd3_set_params(sactd3_engine* e, int which, const float* src) {
  if (!e || !src) return SACTD3_EINVAL;
  USE_DEVICE(e);
  CHAIN_BREAK(e);
  if (which == SACTD3_LOG_ALPHA) {
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(e->la, src, sizeof(float), hipMemcpyHostToDevice));
    return 0;
  }
  float *P, *M, *V; const NetLayout* L; int nets; int* t;
  if (!which_arena(e, which, &P, &M, &V, &L, &nets, &t)) return e->fail(SACTD3_EINVAL, "bad `which`");
  if (which == SACTD3_ACTOR) RCCHK(actor_write_begin(e));   // (write_arena synchronises the learner stream, hence the acting call too)
  return write_arena(e, P, *L, nets, src, true);
}

int sactd3_get_adam_state(sactd3_engine* e, int which, float* m, float* v, int64_t* step) {
  if (!e) return SACTD3_EINVAL;
  USE_DEVICE(e);
  DevCtl hc;
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(&hc, e->ctl, sizeof(hc), hipMemcpyDeviceToHost));
  if (which == SACTD3_LOG_ALPHA) {
    float h[4];
    HIPCHK(hipMemcpy(h, e->la, sizeof(h), hipMemcpyDeviceToHost));
    if (m) *m = h[1];
    if (v) *v = h[2];
    if (step) *step = hc.t_l;
    return 0;
  }
  if (which != SACTD3_ACTOR && which != SACTD3_CRITICS) return e->fail(SACTD3_EINVAL, "no optimiser owns this parameter set");
  float *P, *M, *V; const NetLayout* L; int nets; int* t;
  which_arena(e, which, &P, &M, &V, &L, &nets, &t);
  if (m) RCCHK(read_arena(e, M, *L, nets, m));
  if (v) RCCHK(read_arena(e, V, *L, nets, v));
  if (step) *step = which == SACTD3_ACTOR ? hc.t_a : hc.t_q;
  return 0;
}

int sactd3_set_adam_state(sactd3_engine* e, int which, const float* m, const float* v, int64_t step) {
  if (!e) return SACTD3_EINVAL;
  USE_DEVICE(e);
  CHAIN_BREAK(e);
  HIPCHK(hipStreamSynchronize(e->stream));
  const int st = (int)step;
  if (which == SACTD3_LOG_ALPHA) {
    if (m) HIPCHK(hipMemcpy(e->la + 1, m, sizeof(float), hipMemcpyHostToDevice));
    if (v) HIPCHK(hipMemcpy(e->la + 2, v, sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(&e->ctl->t_l, &st, sizeof(int), hipMemcpyHostToDevice));
    const double pw[2] = {pow((double)e->cfg.adam_beta1, (double)st), pow((double)e->cfg.adam_beta2, (double)st)};
    HIPCHK(hipMemcpy(e->ctl->pw_l, pw, sizeof(pw), hipMemcpyHostToDevice));
    return 0;
  }
  if (which != SACTD3_ACTOR && which != SACTD3_CRITICS) return e->fail(SACTD3_EINVAL, "no optimiser owns this parameter set");
  float *P, *M, *V; const NetLayout* L; int nets; int* t;
  which_arena(e, which, &P, &M, &V, &L, &nets, &t);
  if (m) RCCHK(write_arena(e, M, *L, nets, m, false));
  if (v) RCCHK(write_arena(e, V, *L, nets, v, false));
  HIPCHK(hipMemcpy(t, &st, sizeof(int), hipMemcpyHostToDevice));
  const double pw[2] = {pow((double)e->cfg.adam_beta1, (double)st), pow((double)e->cfg.adam_beta2, (double)st)};
  HIPCHK(hipMemcpy(which == SACTD3_ACTOR ? e->ctl->pw_a : e->ctl->pw_q, pw, sizeof(pw), hipMemcpyHostToDevice));
  return 0;
}

// ---- replay buffer
static void pack_record(const sactd3_engine* e, float* rec, const float* ob, const float* ac, float rw, const float* nob, uint8_t dn) {
  memset(rec, 0, sizeof(float) * e->rec_f);
  memcpy(rec, ob, sizeof(float) * e->o);
  memcpy(rec + e->o, ac, sizeof(float) * e->a);
  memcpy(rec + e->ldc, nob, sizeof(float) * e->o);
  rec[e->ldc + e->ldo] = rw;
  rec[e->ldc + e->ldo + 1] = dn ? 1.f : 0.f;
}
// `chunk` packed records at `src` (pinned host memory or device memory) into the ring: one k_rb_ingest launch of at most max_blocks
// blocks, which writes them round-robin (wrapping at capacity) and publishes the new length / cursor
static int launch_ingest(EnqCtx& x, const float* src, int chunk, long max_blocks) {
  sactd3_engine* e = x.e;
  IngestArgs g{};
  const RingSpan sp = ring_append(e, chunk);
  g.src = (const float4*)src; g.ring = sp.ring; g.rec4 = e->rec4; g.n = chunk; g.cursor = sp.cursor; g.cap = sp.cap;
  g.len_cursor = &e->ctl->rb_len; g.new_len = sp.new_len; g.new_cursor = sp.new_cursor;
  const int blocks = (int)std::min<long>(max_blocks, ((long)chunk * e->rec4 + 255) / 256);
  LAUNCH_ON(k_rb_ingest, dim3(std::max(blocks, 1)), dim3(256), g);
  return prio_after_append(x, sp.first, chunk);
}

int sactd3_rb_extend(sactd3_engine* e, const float* obs, const float* act, const float* rew, const float* nobs, const uint8_t* dones, int n) {
  if (!e || !obs || !act || !rew || !nobs || !dones || n < 0) return e ? e->fail(SACTD3_EINVAL, "rb_extend: bad argument") : SACTD3_EINVAL;
  USE_DEVICE(e);
  CHAIN_BREAK(e);
  EnqCtx x{e, e->stream};
  int done_rows = 0;
  while (done_rows < n) {
    const int chunk = (int)std::min<int64_t>(std::min(n - done_rows, e->stage_rows), ring_region(e));
    // staging slots are reused round-robin; one stream sync per lap of the ring of slots guarantees that the copy
    // that last read a slot has completed (events / device-written flags cost more per call than this amortised sync)
    if (++e->stage_used == NSTAGE) { HIPCHK(hipStreamSynchronize(e->stream)); e->stage_used = 1; }
    const int slot = e->stage_next; e->stage_next = (e->stage_next + 1) % NSTAGE;
    float* st = e->h_stage[slot];
    for (int i = 0; i < chunk; ++i) {
      const int r = done_rows + i;
      pack_record(e, st + (size_t)i * e->rec_f, obs + (size_t)r * e->o, act + (size_t)r * e->a, rew[r], nobs + (size_t)r * e->o, dones[r]);
    }
    RCCHK(launch_ingest(x, st, chunk, 256));      // (the kernel reads the staged rows from pinned host memory)
    done_rows += chunk;
  }
  return 0;
}

int sactd3_rb_layout(const sactd3_engine* e, int32_t out[4]) {
  if (!e || !out) return SACTD3_EINVAL;
  out[0] = e->rec_f; out[1] = e->ldc; out[2] = e->ldo; out[3] = e->cfg.rb_capacity;
  return 0;
}

// rb.extend with packed records that are already in device memory (shared-replay variant: every rank's rows, all-gathered
// over RCCL into one device slab): the same k_rb_ingest launch as the host path, reading the slab instead of a pinned slot.
int sactd3_rb_extend_device(sactd3_engine* e, const float* records, int n) {
  if (!e || !records || n < 0) return e ? e->fail(SACTD3_EINVAL, "rb_extend_device: bad argument") : SACTD3_EINVAL;
  USE_DEVICE(e);
  CHAIN_BREAK(e);
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, records) != hipSuccess || at.type != hipMemoryTypeDevice) {
    (void)hipGetLastError();
    return e->fail(SACTD3_EINVAL, "rb_extend_device: `records` is not a device pointer");
  }
  EnqCtx x{e, e->stream};
  int done_rows = 0;
  while (done_rows < n) {
    const int chunk = (int)std::min<int64_t>(n - done_rows, ring_region(e));
    RCCHK(launch_ingest(x, records + (size_t)done_rows * e->rec_f, chunk, 1024));
    done_rows += chunk;
  }
  return 0;
}

int64_t sactd3_rb_len(const sactd3_engine* e) { return e ? e->rb_len : SACTD3_EINVAL; }
int64_t sactd3_batch_generation(const sactd3_engine* e) { return e ? e->slot.generation : SACTD3_EINVAL; }

int sactd3_rb_sample(sactd3_engine* e) {
  if (!e) return SACTD3_EINVAL;
  USE_DEVICE(e);
  CHAIN_BREAK(e);
  if (e->rb_len <= 0) return e->fail(SACTD3_ESTATE, "rb_sample: buffer is empty");
  slot_refilled(e, false, false);
  EnqCtx x{e, e->stream};
  RCCHK(enqueue_gather(x, e->ring, -1));
  return launch_tick(x, &e->ctl->sample_ctr);
}

int sactd3_rb_sample_with_indices(sactd3_engine* e, const int64_t* idx, int n) {
  if (!e || !idx) return SACTD3_EINVAL;
  USE_DEVICE(e);
  CHAIN_BREAK(e);
  if (n != e->B) return e->fail(SACTD3_EINVAL, "rb_sample_with_indices: n must equal batch_size");
  std::vector<int> h(n);
  for (int i = 0; i < n; ++i) {
    if (idx[i] < 0 || idx[i] >= e->rb_len) return e->fail(SACTD3_EINVAL, "rb_sample_with_indices: index out of range");
    h[i] = (int)idx[i];
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(e->idx, h.data(), sizeof(int) * n, hipMemcpyHostToDevice));
  slot_refilled(e, false, false);
  EnqCtx x{e, e->stream};
  RCCHK(set_flag(x, &e->ctl->inject_idx, 1));
  RCCHK(enqueue_gather(x, e->ring, -1));
  return set_flag(x, &e->ctl->inject_idx, 0);
}

int sactd3_load_batch(sactd3_engine* e, const float* obs, const float* act, const float* rew, const float* nobs, const uint8_t* dones, int n) {
  if (!e || !obs || !act || !rew || !nobs || !dones) return SACTD3_EINVAL;
  USE_DEVICE(e);
  CHAIN_BREAK(e);
  if (n != e->B) return e->fail(SACTD3_EINVAL, "load_batch: n must equal batch_size");
  HIPCHK(hipStreamSynchronize(e->stream));
  slot_refilled(e, false, false);
  std::vector<int> h(n);
  for (int i = 0; i < n; ++i) {
    pack_record(e, e->h_batch + (size_t)i * e->rec_f, obs + (size_t)i * e->o, act + (size_t)i * e->a, rew[i], nobs + (size_t)i * e->o, dones[i]);
    h[i] = i;
  }
  HIPCHK(hipMemcpy(e->stage_dev, e->h_batch, sizeof(float) * (size_t)n * e->rec_f, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->idx, h.data(), sizeof(int) * n, hipMemcpyHostToDevice));
  EnqCtx x{e, e->stream};
  RCCHK(set_flag(x, &e->ctl->inject_idx, 1));
  RCCHK(enqueue_gather(x, e->stage_dev, n));
  return set_flag(x, &e->ctl->inject_idx, 0);
}

// ---- the device boundary: the caller's five arrays are already in this device's memory (include/sactd3.h)
// THE rule for a caller's pointer, for every entry point from here on: device memory of the engine's device
static int device_ptr_check(sactd3_engine* e, const void* p, const char* what, const char* name) {
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != e->cfg.device_id) {
    (void)hipGetLastError();
    e->err = std::string(what) + ": `" + name + "` is not device memory of the engine's device";
    return SACTD3_EINVAL;
  }
  return 0;
}
// one row per field of a caller's field block.  Inputs (`required`): a NULL pointer is refused; outputs: it is a field not wanted
struct FieldRow { const void* p; int64_t ld; int width; const char* name; };
// none_wanted: the refusal when every pointer of an output block is NULL (NULL: the caller has its own rule for that)
static int field_rows_check(sactd3_engine* e, const FieldRow* rows, int count, bool required, const char* what, const char* none_wanted) {
  int wanted = 0;
  for (const FieldRow* x = rows; x != rows + count; ++x) {
    if (!x->p && !required) continue;
    if (!x->p) { e->err = std::string(what) + ": `" + x->name + "` is NULL"; return SACTD3_EINVAL; }
    ++wanted;
    if (x->ld < x->width) { e->err = std::string(what) + ": row stride of `" + x->name + "` is below its width"; return SACTD3_EINVAL; }
    RCCHK(device_ptr_check(e, x->p, what, x->name));
  }
  if (!wanted && none_wanted) { e->err = std::string(what) + ": " + none_wanted; return SACTD3_EINVAL; }
  return 0;
}
static int fields_check(sactd3_engine* e, const sactd3_device_fields* f, const char* what) {
  const FieldRow rows[5] = {
      {f->obs, f->obs_ld, e->o, "obs"}, {f->actions, f->actions_ld, e->a, "actions"}, {f->rewards, f->rewards_ld, 1, "rewards"},
      {f->next_obs, f->next_obs_ld, e->o, "next_obs"}, {f->dones, f->dones_ld, 1, "dones"}};
  return field_rows_check(e, rows, 5, true, what, nullptr);
}
// the *_stats getters: four host counters; or host counters and words the kernels keep on the device (stats_with_words)
static int host_stats(const sactd3_engine* e, int64_t (sactd3_engine::*stats)[4], int64_t out[4]) {
  if (!e || !out) return SACTD3_EINVAL;
  for (int i = 0; i < 4; ++i) out[i] = (e->*stats)[i];
  return 0;
}
// out[at, at + nw) = the nw adjacent device words at `words`, read behind a stream sync -- or 0 where the feature's state does not exist
// yet (words == NULL); the other entries = the 4 - nw host counters, in their order
static int stats_with_words(sactd3_engine* e, const int64_t* host, const int* words, int nw, int at, int64_t out[4]) {
  USE_DEVICE(e);
  int w[4] = {0, 0, 0, 0};
  if (words) {
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(w, words, sizeof(int) * nw, hipMemcpyDeviceToHost));
  }
  for (int i = 0; i < 4; ++i) out[i] = (i >= at && i < at + nw) ? w[i - at] : *host++;
  return 0;
}
static FieldSrc field_src(const sactd3_engine* e, const sactd3_device_fields* f, int64_t row0) {
  FieldSrc s{};
  s.obs = f->obs + row0 * f->obs_ld; s.act = f->actions + row0 * f->actions_ld; s.rew = f->rewards + row0 * f->rewards_ld;
  s.nobs = f->next_obs + row0 * f->next_obs_ld; s.done = f->dones + row0 * f->dones_ld;
  s.obs_ld = (long)f->obs_ld; s.act_ld = (long)f->actions_ld; s.rew_ld = (long)f->rewards_ld; s.nobs_ld = (long)f->next_obs_ld; s.done_ld = (long)f->dones_ld;
  s.o = e->o; s.a = e->a; s.cx = e->cx; s.cn = e->cn;
  return s;
}
// SACTD3_SRC_ORDERED, first half: the learner stream waits for what the caller has queued on its producer stream so far
static int src_order_begin(sactd3_engine* e, hipStream_t producer, int flags) {
  if (!(flags & SACTD3_SRC_ORDERED)) return 0;
  if (!e->ev_src_ready) HIPCHK(hipEventCreateWithFlags(&e->ev_src_ready, hipEventDisableTiming));
  if (!e->ev_src_read) HIPCHK(hipEventCreateWithFlags(&e->ev_src_read, hipEventDisableTiming));
  HIPCHK(hipEventRecord(e->ev_src_ready, producer));
  HIPCHK(hipStreamWaitEvent(e->stream, e->ev_src_ready, 0));
  return 0;
}
// ... second half: whatever the caller queues there next (an overwrite, the reuse of the freed block) waits for the read
static int src_order_end(sactd3_engine* e, hipStream_t producer, int flags) {
  if (!(flags & SACTD3_SRC_ORDERED)) return 0;
  HIPCHK(hipEventRecord(e->ev_src_read, e->stream));
  HIPCHK(hipStreamWaitEvent(producer, e->ev_src_read, 0));
  ++e->bnd_stats[3];
  return 0;
}
static int launch_ingest_fields(EnqCtx& x, const FieldSrc& src, int chunk) {
  sactd3_engine* e = x.e;
  IngestFieldsArgs g{};
  const RingSpan sp = ring_append(e, chunk);
  g.ring = sp.ring; g.rec4 = e->rec4; g.n = chunk; g.cursor = sp.cursor; g.cap = sp.cap;
  g.len_cursor = &e->ctl->rb_len; g.new_len = sp.new_len; g.new_cursor = sp.new_cursor;
  const long chunks = (long)chunk * e->rec4;
  LAUNCH_ON(k_rb_ingest_fields, dim3(cpt_blocks(chunks, FIELDS_CPT)), dim3(256), FIELD_ARGS(src), g);
  return prio_after_append(x, sp.first, chunk);
}
static int launch_batch_fields(EnqCtx& x, const FieldSrc& src) {
  sactd3_engine* e = x.e;
  const sactd3_engine::BatchSlot& S = e->bs[0];
  BatchFieldsArgs g{};
  g.X = (float4*)S.X; g.Xn = (float4*)S.Xn; g.rew = S.rew; g.done = S.done; g.idx = S.idx; g.B = e->B;
  const long chunks = (long)e->B * (e->cx + e->cn + 1);      // (< B * rec4 < 2^31: create_impl)
  LAUNCH_ON(k_batch_from_fields, dim3(cpt_blocks(chunks, FIELDS_CPT)), dim3(256), FIELD_ARGS(src), g);
  return 0;
}

// rb.extend (orchestrator.py:100-113) with the TensorDict's fields where they are, in device memory: one k_rb_ingest_fields launch
// per at most rb_capacity rows, no host pack, no copy, no wait on the host.
int sactd3_rb_extend_fields_device(sactd3_engine* e, const sactd3_device_fields* f, int n, void* producer_stream, int flags) {
  if (!e) return SACTD3_EINVAL;
  if (!f || n < 0) return e->fail(SACTD3_EINVAL, "rb_extend_fields_device: bad argument");
  USE_DEVICE(e);
  CHAIN_BREAK(e);
  RCCHK(fields_check(e, f, "rb_extend_fields_device"));
  const hipStream_t producer = (hipStream_t)producer_stream;
  const int64_t per_launch = std::min<int64_t>(ring_region(e), ((1ll << 31) - 1) / e->rec4);
  EnqCtx x{e, e->stream};
  if (n > 0) RCCHK(src_order_begin(e, producer, flags));
  for (int done_rows = 0; done_rows < n;) {
    const int chunk = (int)std::min<int64_t>(n - done_rows, per_launch);
    RCCHK(launch_ingest_fields(x, field_src(e, f, done_rows), chunk));
    done_rows += chunk;
  }
  if (n > 0) RCCHK(src_order_end(e, producer, flags));
  ++e->bnd_stats[0]; e->bnd_stats[1] += n;
  return 0;
}

// sactd3_rb_extend_device for a slab a producer stream is still writing (a GPU-resident env's step, include/sactd3_rollout.h): the same
// launch_ingest per ring region, bracketed by the two events of SACTD3_SRC_ORDERED.  Every refusal comes before the first side effect.
int sactd3_rb_extend_records_device(sactd3_engine* e, const float* records, int n, void* producer_stream, int flags) {
  if (!e) return SACTD3_EINVAL;
  if (!records || n < 0) return e->fail(SACTD3_EINVAL, "rb_extend_records_device: bad argument");
  if (flags & ~SACTD3_SRC_ORDERED) return e->fail(SACTD3_EINVAL, "rb_extend_records_device: unknown flag");
  if ((uintptr_t)records % 16) return e->fail(SACTD3_EINVAL, "rb_extend_records_device: `records` is not 16-byte aligned");
  USE_DEVICE(e);
  RCCHK(device_ptr_check(e, records, "rb_extend_records_device", "records"));
  if (n == 0) return 0;
  CHAIN_BREAK(e);
  const hipStream_t producer = (hipStream_t)producer_stream;
  const int64_t int_rows = ((1ll << 31) - 1) / e->rec4;      // (k_rb_ingest counts float4 chunks in an int)
  EnqCtx x{e, e->stream};
  RCCHK(src_order_begin(e, producer, flags));
  for (int done_rows = 0; done_rows < n;) {
    const int chunk = (int)std::min<int64_t>(std::min<int64_t>(n - done_rows, int_rows), ring_region(e));
    RCCHK(launch_ingest(x, records + (size_t)done_rows * e->rec_f, chunk, 1024));
    done_rows += chunk;
  }
  RCCHK(src_order_end(e, producer, flags));
  return 0;
}

// a caller-owned DEVICE batch (what update_qnets(batch) / update_actor(batch) receive in the reference, agents/agent.py:183,245):
// one k_batch_from_fields launch fills batch slot 0 as sactd3_load_batch would have.
int sactd3_load_batch_device(sactd3_engine* e, const sactd3_device_fields* f, int n, void* producer_stream, int flags) {
  if (!e) return SACTD3_EINVAL;
  if (!f) return e->fail(SACTD3_EINVAL, "load_batch_device: bad argument");
  USE_DEVICE(e);
  CHAIN_BREAK(e);
  if (n != e->B) return e->fail(SACTD3_EINVAL, "load_batch_device: n must equal batch_size");
  RCCHK(fields_check(e, f, "load_batch_device"));
  const hipStream_t producer = (hipStream_t)producer_stream;
  RCCHK(src_order_begin(e, producer, flags));
  slot_refilled(e, false, false);
  EnqCtx x{e, e->stream};
  RCCHK(launch_batch_fields(x, field_src(e, f, 0)));
  RCCHK(src_order_end(e, producer, flags));
  ++e->bnd_stats[2];
  return 0;
}

int sactd3_boundary_stats(const sactd3_engine* e, int64_t out[4]) { return host_stats(e, &sactd3_engine::bnd_stats, out); }

int sactd3_read_batch(sactd3_engine* e, float* obs, float* act, float* rew, float* nobs, uint8_t* dones, int64_t* idx) {
  if (!e) return SACTD3_EINVAL;
  USE_DEVICE(e);
  const int B = e->B;
  HIPCHK(hipStreamSynchronize(e->stream));
  std::vector<float> hx((size_t)B * e->ldc), hn((size_t)B * e->ldc), hr(B), hd(B);
  std::vector<int> hi(B);
  const sactd3_engine::BatchSlot& S = e->bs[e->slot.cur];      // the slot of the most recent iteration
  HIPCHK(hipMemcpy(hx.data(), S.X, sizeof(float) * hx.size(), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hn.data(), S.Xn, sizeof(float) * hn.size(), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hr.data(), S.rew, sizeof(float) * B, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hd.data(), S.done, sizeof(float) * B, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hi.data(), S.idx, sizeof(int) * B, hipMemcpyDeviceToHost));
  for (int b = 0; b < B; ++b) {
    if (obs) memcpy(obs + (size_t)b * e->o, hx.data() + (size_t)b * e->ldc, sizeof(float) * e->o);
    if (act) memcpy(act + (size_t)b * e->a, hx.data() + (size_t)b * e->ldc + e->o, sizeof(float) * e->a);
    if (nobs) memcpy(nobs + (size_t)b * e->o, hn.data() + (size_t)b * e->ldc, sizeof(float) * e->o);
    if (rew) rew[b] = hr[b];
    if (dones) dones[b] = hd[b] != 0.f;
    if (idx) idx[b] = hi[b];
  }
  return 0;
}

// ---- the device boundary, outwards: a batch slot / ring rows into the caller's six arrays in this device's memory (include/sactd3.h)
static int fields_out_check(sactd3_engine* e, const sactd3_device_fields_out* f, const char* what) {
  const FieldRow rows[6] = {
      {f->obs, f->obs_ld, e->o, "obs"}, {f->actions, f->actions_ld, e->a, "actions"}, {f->rewards, f->rewards_ld, 1, "rewards"},
      {f->next_obs, f->next_obs_ld, e->o, "next_obs"}, {f->dones, f->dones_ld, 1, "dones"}, {f->index, f->index_ld, 1, "index"}};
  return field_rows_check(e, rows, 6, false, what, "all six destinations (obs, actions, rewards, next_obs, dones, index) are NULL");
}
static FieldDst field_dst(const sactd3_engine* e, const sactd3_device_fields_out* f, int64_t row0) {
  FieldDst d{};
  d.obs = f->obs ? f->obs + row0 * f->obs_ld : nullptr; d.act = f->actions ? f->actions + row0 * f->actions_ld : nullptr;
  d.rew = f->rewards ? f->rewards + row0 * f->rewards_ld : nullptr; d.nobs = f->next_obs ? f->next_obs + row0 * f->next_obs_ld : nullptr;
  d.done = f->dones ? f->dones + row0 * f->dones_ld : nullptr; d.index = f->index ? (long long*)f->index + row0 * f->index_ld : nullptr;
  d.obs_ld = (long)f->obs_ld; d.act_ld = (long)f->actions_ld; d.rew_ld = (long)f->rewards_ld; d.nobs_ld = (long)f->next_obs_ld;
  d.done_ld = (long)f->dones_ld; d.index_ld = (long)f->index_ld;
  d.o = e->o; d.a = e->a; d.cx = e->cx; d.cn = e->cn;
  return d;
}
static int launch_batch_out(EnqCtx& x, const FieldDst& dst) {
  sactd3_engine* e = x.e;
  const sactd3_engine::BatchSlot& S = e->bs[e->slot.cur];      // the slot sactd3_read_batch reports
  const BatchOutArgs g{(const float4*)S.X, (const float4*)S.Xn, S.rew, S.done, S.idx, e->B};
  const long chunks = (long)e->B * (e->cx + e->cn + 1);      // (< B * rec4 < 2^31: create_impl)
  LAUNCH_ON(k_batch_to_fields, dim3(cpt_blocks(chunks, TOFIELDS_CPT)), dim3(256), dst, g);
  return 0;
}
// rows [0, n) of `idx` (n * rec4 < 2^31), `len` = the ring length the indices are checked against
static int launch_rows_out(EnqCtx& x, const FieldDst& dst, const long long* idx, int64_t idx_ld, int n, int len) {
  sactd3_engine* e = x.e;
  RowsOutArgs g{};
  g.ring = (const float4*)e->ring; g.rec4 = e->rec4; g.n = n; g.len = len; g.idx = idx; g.idx_ld = (long)idx_ld;
  const long chunks = (long)n * e->rec4;
  g.rec4_magic = magic_div((unsigned)e->rec4, (unsigned long long)chunks + 1);
  const unsigned blocks = gather_blocks(chunks);
  g.cpb = (int)((chunks + 256L * blocks - 1) / (256L * blocks));
  g.refused = &e->ctl->readout_refused;
  LAUNCH_ON(k_rows_to_fields, dim3(blocks), dim3(256), dst, g);
  return 0;
}

// rb.sample()'s batch as the reference hands it out -- on the device (main.py:167-171, orchestrator.py:338): one k_batch_to_fields launch
// on the learner stream copies the current slot to the caller's arrays.  No host wait, no copy command; it changes nothing an update
// or a precomputed opening pair depends on, so the run-ahead chain stays intact.
int sactd3_read_batch_device(sactd3_engine* e, const sactd3_device_fields_out* f, void* consumer_stream, int flags) {
  if (!e) return SACTD3_EINVAL;
  if (!f) return e->fail(SACTD3_EINVAL, "read_batch_device: bad argument");
  USE_DEVICE(e);
  if (flags & ~SACTD3_DST_ORDERED) return e->fail(SACTD3_EINVAL, "read_batch_device: unknown flag");
  RCCHK(fields_out_check(e, f, "read_batch_device"));
  const hipStream_t consumer = (hipStream_t)consumer_stream;
  EnqCtx x{e, e->stream};
  RCCHK(src_order_begin(e, consumer, flags));
  RCCHK(launch_batch_out(x, field_dst(e, f, 0)));
  RCCHK(src_order_end(e, consumer, flags));
  ++e->ro_stats[0];
  return 0;
}

// ring records by index, for a sampler the engine does not own (prioritised / n-step / hindsight: it reads the rows it relabels or
// chains where they are): one k_rows_to_fields launch per at most (2^31 - 1) / rec4 rows.
int sactd3_rb_read_rows_device(sactd3_engine* e, const int64_t* idx, int64_t idx_ld, int n, const sactd3_device_fields_out* f,
                               void* consumer_stream, int flags) {
  if (!e) return SACTD3_EINVAL;
  if (!f || !idx) return e->fail(SACTD3_EINVAL, "rb_read_rows_device: bad argument (`idx` or the field block is NULL)");
  USE_DEVICE(e);
  if (n < 1) return e->fail(SACTD3_EINVAL, "rb_read_rows_device: n >= 1 required");
  if (flags & ~SACTD3_DST_ORDERED) return e->fail(SACTD3_EINVAL, "rb_read_rows_device: unknown flag");
  if (idx_ld < 1) return e->fail(SACTD3_EINVAL, "rb_read_rows_device: row stride of `idx` is below its width");
  RCCHK(fields_out_check(e, f, "rb_read_rows_device"));
  RCCHK(device_ptr_check(e, idx, "rb_read_rows_device", "idx"));
  if (e->rb_len <= 0) return e->fail(SACTD3_ESTATE, "rb_read_rows_device: buffer is empty");
  const hipStream_t consumer = (hipStream_t)consumer_stream;
  const int64_t per_launch = ((1ll << 31) - 1) / e->rec4;
  EnqCtx x{e, e->stream};
  RCCHK(src_order_begin(e, consumer, flags));
  for (int done_rows = 0; done_rows < n;) {
    const int chunk = (int)std::min<int64_t>(n - done_rows, per_launch);
    RCCHK(launch_rows_out(x, field_dst(e, f, done_rows), (const long long*)idx + (int64_t)done_rows * idx_ld, idx_ld, chunk, (int)e->rb_len));
    done_rows += chunk;
  }
  RCCHK(src_order_end(e, consumer, flags));
  ++e->ro_stats[1]; e->ro_stats[2] += n;
  return 0;
}

int sactd3_readout_stats(sactd3_engine* e, int64_t out[4]) { return (!e || !out) ? SACTD3_EINVAL : stats_with_words(e, e->ro_stats, &e->ctl->readout_refused, 1, 3, out); }

// ---- ring rows into batch slot 0, all on the device (include/sactd3.h): the caller's rows or the engine's draw, one row each or chained
// into n-step returns, with or without loss weights.  One request, one routine; the entry points below only fill the request in.
struct StageReq {
  const char* name;                            // the entry point's name, for messages
  int kind = SACTD3_DRAW_UNIFORM;              // the engine's draw: uniform at the sample counter (chained or hindsight form only: the 1-step
                                               // uniform sample is sactd3_rb_sample's gather), or by the priority table (beta) ...
  bool callers = false; CallerRows rows; int n = 0;      // ... or none: the caller's n rows, staged plainly (kind uniform) or relabelled (hindsight)
  float beta = 0.f;                            // SACTD3_DRAW_PRIORITIZED: the exponent of the importance weights
  bool chain = false; int steps = 0, stride = 0;      // chain: k_batch_from_index_nstep over (steps, stride); otherwise k_batch_from_index
  void* caller_stream = nullptr; int flags = 0;       // SACTD3_SRC_ORDERED and the stream it orders against
  bool internal = false;                       // a timing body: the index array is the engine's own (no pointer check) and no host counter moves
};
// The whole protocol, always in this order:
//   1. refusals, the first fault wins: `idx` NULL, unknown flag, n, stride of `idx`, of `w`, of `choice` (the caller's arrays); beta
//      (priority draw); steps, stride (chained); `idx`, `w`, `choice` not device memory of this device; then the ring's state
//      (draw_state_refusal: priorities not enabled; a chain over pinned rows; hindsight not configured, or over pinned rows; ring empty).
//      A refused call has changed nothing -- a precomputed opening pair (chain_ready) stays valid across it
//   2. CHAIN_BREAK                     3. allocations at first use (draw_alloc)                       4. src_order_begin
//   5. the launches, on the learner stream (draw_launches): [k_prio_draw, k_prio_weights, or k_mix_draw, which ticks the sample counter,]
//      the staging kernel [, k_tick of the sample counter behind a uniform draw it made itself]
//   6. src_order_end                   7. slot_refilled                                               8. the host counters (7, 8: draw_issued)
static int stage_ring_rows(EnqCtx& x, const StageReq& q) {
  sactd3_engine* e = x.e;
  const auto refuse = [&](int code, const char* what) { e->err = std::string(q.name) + ": " + what; return code; };
  const CallerRows& r = q.rows;
  if (q.callers) {
    if (!r.idx) return refuse(SACTD3_EINVAL, "`idx` is NULL");
    if (q.flags & ~SACTD3_SRC_ORDERED) return refuse(SACTD3_EINVAL, "unknown flag");
    if (q.n != e->B) return refuse(SACTD3_EINVAL, "n must equal batch_size");
    if (r.idx_ld < 1) return refuse(SACTD3_EINVAL, "row stride of `idx` is below its width");
    if (r.w && r.w_ld < 1) return refuse(SACTD3_EINVAL, "row stride of `w` is below its width");
    if (r.choice && r.choice_ld < 1) return refuse(SACTD3_EINVAL, "row stride of `choice` is below its width");
  }
  if (q.kind == SACTD3_DRAW_PRIORITIZED && (!(q.beta >= 0.f) || !std::isfinite(q.beta))) return refuse(SACTD3_EINVAL, "beta must be finite and >= 0");
  if (q.chain && (q.steps < 1 || q.steps > NS_MAX)) return refuse(SACTD3_EINVAL, "steps must be in [1, 16]");
  if (q.chain && q.stride < 1) return refuse(SACTD3_EINVAL, "stride must be at least 1");
  if (q.kind == SACTD3_DRAW_UNIFORM && !q.callers && !q.chain) return refuse(SACTD3_EINVAL, "the uniform 1-step sample is sactd3_rb_sample");      // (no entry point asks)
  if (q.callers && !q.internal) {
    RCCHK(device_ptr_check(e, r.idx, q.name, "idx"));
    if (r.w) RCCHK(device_ptr_check(e, r.w, q.name, "w"));
    if (r.choice) RCCHK(device_ptr_check(e, r.choice, q.name, "choice"));
  }
  const Draw d{q.kind, q.beta, q.chain ? q.steps : 0, q.chain ? q.stride : 0, q.callers ? &r : nullptr};      // the arguments hold
  if (const char* why = draw_state_refusal(e, d)) return refuse(SACTD3_ESTATE, why);
  CHAIN_BREAK(e);
  RCCHK(draw_alloc(e, d));
  const hipStream_t caller = (hipStream_t)q.caller_stream;
  RCCHK(src_order_begin(e, caller, q.flags));
  RCCHK(draw_launches(x, d));
  RCCHK(src_order_end(e, caller, q.flags));
  if (q.internal) slot_refilled(e, d.weighted(), d.chain());      // (a timing body moves no counter)
  else draw_issued(e, d, false);
  return 0;
}

static int stage_call(sactd3_engine* e, const StageReq& q) {      // what the entry points below end with
  USE_DEVICE(e);
  EnqCtx x{e, e->stream};
  return stage_ring_rows(x, q);
}
// rb.sample() with the caller's indices and importance weights: one k_batch_from_index launch fills slot 0 as the index-injected gather
// of sactd3_rb_sample_with_indices does, plus the slot's w.  No host wait, no copy command, no sample-counter tick.
int sactd3_rb_sample_indices_device(sactd3_engine* e, const int64_t* idx, int64_t idx_ld, const float* w, int64_t w_ld, int n,
                                    void* caller_stream, int flags) {
  if (!e) return SACTD3_EINVAL;
  StageReq q{"rb_sample_indices_device"};
  q.callers = true; q.rows = {(const long long*)idx, idx_ld, w, w_ld, nullptr, 1, true}; q.n = n;
  q.caller_stream = caller_stream; q.flags = flags;
  return stage_call(e, q);
}
// ... with the chain: one k_batch_from_index_nstep launch
int sactd3_rb_sample_nstep_device(sactd3_engine* e, const int64_t* idx, int64_t idx_ld, const float* w, int64_t w_ld, int n, int steps,
                                  int stride, void* caller_stream, int flags) {
  if (!e) return SACTD3_EINVAL;
  StageReq q{"rb_sample_nstep_device"};
  q.callers = true; q.rows = {(const long long*)idx, idx_ld, w, w_ld, nullptr, 1, true}; q.n = n;
  q.chain = true; q.steps = steps; q.stride = stride; q.caller_stream = caller_stream; q.flags = flags;
  return stage_call(e, q);
}
// sactd3_rb_sample with the chain: the start slots are the uniform draw at the current sample counter, which then advances once
int sactd3_rb_sample_nstep(sactd3_engine* e, int steps, int stride) {
  if (!e) return SACTD3_EINVAL;
  StageReq q{"rb_sample_nstep"};
  q.chain = true; q.steps = steps; q.stride = stride;
  return stage_call(e, q);
}
// rb.sample by priority: k_prio_draw, k_prio_weights, k_batch_from_index.  The uniform sampler's counter is not touched.
int sactd3_rb_sample_prioritized(sactd3_engine* e, float beta) {
  if (!e) return SACTD3_EINVAL;
  StageReq q{"rb_sample_prioritized"};
  q.kind = SACTD3_DRAW_PRIORITIZED; q.beta = beta;
  return stage_call(e, q);
}
// ... with the chain: the n-step staging kernel on the drawn slots
int sactd3_rb_sample_prioritized_nstep(sactd3_engine* e, float beta, int steps, int stride) {
  if (!e) return SACTD3_EINVAL;
  StageReq q{"rb_sample_prioritized_nstep"};
  q.kind = SACTD3_DRAW_PRIORITIZED; q.beta = beta; q.chain = true; q.steps = steps; q.stride = stride;
  return stage_call(e, q);
}

// ---- prior data under an online run (include/sactd3.h): pinned rows and the mixed draw
// Slots [0, n) become rows no append overwrites.  Host state only: nothing is launched unless the cursor has to leave the pinned rows
// (a ring that is exactly full and has not wrapped stands at cursor 0), which republishes the ring state.
int sactd3_rb_pin(sactd3_engine* e, int64_t n) {
  if (!e) return SACTD3_EINVAL;
  USE_DEVICE(e);
  const int64_t cap = e->cfg.rb_capacity;
  if (n < 0 || n > e->rb_len || n >= cap) return e->fail(SACTD3_EINVAL, "rb_pin: 0 <= n <= rb_len and n < rb_capacity required");
  if (e->pt_on) return e->fail(SACTD3_ESTATE, "rb_pin: priorities are enabled (a pinned ring has no priority table yet)");
  // where the cursor of a ring that has never overwritten a row stands: behind its rows, or, exactly full, at the first live slot.
  // (Elsewhere: sactd3_rb_fill_synthetic below rows an append wrote -- the order of the rows is gone.)
  const int64_t unwrapped_cursor = e->rb_len < cap ? e->rb_len : e->rb_pinned;
  if (e->rb_wrapped || e->rb_cursor != unwrapped_cursor)
    return e->fail(SACTD3_ESTATE, "rb_pin: the ring has wrapped: the oldest rows are no longer the first ones");
  CHAIN_BREAK(e);
  e->rb_pinned = n;
  if (e->rb_len == cap && e->rb_cursor != n) {      // full, never wrapped: the next append overwrites the oldest LIVE row
    e->rb_cursor = n;
    EnqCtx x{e, e->stream};
    RCCHK(publish_rb_state(x));
  }
  return 0;
}
int64_t sactd3_rb_pinned(const sactd3_engine* e) { return e ? e->rb_pinned : SACTD3_EINVAL; }

// m of the mixed draw: host state; the device's copy is published in front of the next launch that reads it (mix_publish)
int sactd3_rb_set_mix(sactd3_engine* e, int prior_rows) {
  if (!e) return SACTD3_EINVAL;
  if (prior_rows < 0 || prior_rows > e->cfg.batch_size) return e->fail(SACTD3_EINVAL, "rb_set_mix: prior_rows must be in [0, batch_size]");
  e->mix_m = prior_rows;
  return 0;
}

// rb.sample(batch_size) with m rows from the pinned rows and B - m from the live ones: k_mix_draw (which ticks the sample counter),
// then k_batch_from_index on the drawn slots.  Refusals first; a refused call has changed nothing.
int sactd3_rb_sample_mixed(sactd3_engine* e) {
  if (!e) return SACTD3_EINVAL;
  USE_DEVICE(e);
  const Draw d{SACTD3_DRAW_MIXED};
  if (const char* why = draw_state_refusal(e, d)) return state_refusal(e, "rb_sample_mixed", why);
  CHAIN_BREAK(e);
  RCCHK(draw_alloc(e, d));      // (the staging kernel always writes the slot's weights: all 1, and the slot does not carry them)
  EnqCtx x{e, e->stream};
  RCCHK(draw_launches(x, d));
  draw_issued(e, d, false);
  return 0;
}

int sactd3_mix_stats(sactd3_engine* e, int64_t out[4]) { return host_stats(e, &sactd3_engine::mix_stats, out); }

// ---- hindsight relabelling at staging (include/sactd3.h)
// Host state only: no launch, and a precomputed opening pair stays valid across it (nothing it depends on changes).  A CHANGED config
// drops the four graphs of sactd3_step_sampled when they were captured for SACTD3_DRAW_HINDSIGHT (the stream drains first); the same
// config again drops nothing.
int sactd3_hindsight_configure(sactd3_engine* e, const sactd3_hindsight_config* c) {
  if (!e) return SACTD3_EINVAL;
  if (!c) return e->fail(SACTD3_EINVAL, "hindsight_configure: the config is NULL");
  if (c->goal_dim < 1 || c->goal_dim > HS_MAX_GOAL) return e->fail(SACTD3_EINVAL, "hindsight_configure: goal_dim must be in [1, 8]");
  const int o = e->o, G = c->goal_dim;
  if (c->ag_off < 0 || c->ag_off > o - G || c->dg_off < 0 || c->dg_off > o - G)
    return e->fail(SACTD3_EINVAL, "hindsight_configure: a goal range lies outside [0, ob_dim)");
  if (c->ag_off < c->dg_off + G && c->dg_off < c->ag_off + G)
    return e->fail(SACTD3_EINVAL, "hindsight_configure: the achieved and the desired goal overlap");
  if (c->window < 1 || c->window > HS_MAX_WINDOW) return e->fail(SACTD3_EINVAL, "hindsight_configure: window must be in [1, 64]");
  if (c->stride < 1) return e->fail(SACTD3_EINVAL, "hindsight_configure: stride must be at least 1");
  if (!(c->threshold >= 0.f) || !std::isfinite(c->threshold)) return e->fail(SACTD3_EINVAL, "hindsight_configure: threshold must be finite and >= 0");
  if (!(c->ratio >= 0.f && c->ratio <= 1.f)) return e->fail(SACTD3_EINVAL, "hindsight_configure: ratio must be in [0, 1]");
  // the graph forms hold the config by value: graphs captured for the hindsight draw under another config are dropped
  const sactd3_hindsight_config& h = e->hs_cfg;
  const bool same = e->hs_on && h.ag_off == c->ag_off && h.dg_off == c->dg_off && h.goal_dim == c->goal_dim && h.window == c->window &&
                    h.stride == c->stride && memcmp(&h.threshold, &c->threshold, sizeof(float)) == 0 && memcmp(&h.ratio, &c->ratio, sizeof(float)) == 0;
  if (!same && e->ss_draw.kind == SACTD3_DRAW_HINDSIGHT) {
    USE_DEVICE(e);
    RCCHK(drop_graphs(e, G_SAMPLED, 4));
  }
  e->hs_cfg = *c;
  e->hs_on = true;
  return 0;
}

// Both are stage_ring_rows: the uniform draw (with nothing pinned the slots of sactd3_rb_sample) relabelled by k_hindsight_stage, or the
// caller's rows and, with them, the caller's choices.
int sactd3_rb_sample_hindsight(sactd3_engine* e) {
  if (!e) return SACTD3_EINVAL;
  StageReq q{"rb_sample_hindsight"};
  q.kind = SACTD3_DRAW_HINDSIGHT;
  return stage_call(e, q);
}
int sactd3_rb_sample_hindsight_device(sactd3_engine* e, const int64_t* idx, int64_t idx_ld, const int32_t* choice, int64_t choice_ld, int n,
                                      void* caller_stream, int flags) {
  if (!e) return SACTD3_EINVAL;
  StageReq q{"rb_sample_hindsight_device"};
  q.kind = SACTD3_DRAW_HINDSIGHT; q.callers = true; q.rows = {(const long long*)idx, idx_ld, nullptr, 1, (const int*)choice, choice_ld, false}; q.n = n;
  q.caller_stream = caller_stream; q.flags = flags;
  return stage_call(e, q);
}
// the offset and the goal's ring slot of every row of a hindsight slot, left in the caller's device arrays: one k_nstep_info launch (the
// kernel copies two per-row int32 arrays, whatever they mean) on the learner stream.  No CHAIN_BREAK.
int sactd3_hindsight_info_device(sactd3_engine* e, int32_t* offset, int64_t offset_ld, int32_t* goal_slot, int64_t goal_slot_ld, void* caller_stream,
                                 int flags) {
  if (!e) return SACTD3_EINVAL;
  if (!offset && !goal_slot) return e->fail(SACTD3_EINVAL, "hindsight_info_device: `offset` and `goal_slot` are both NULL");
  USE_DEVICE(e);
  if (flags & ~SACTD3_DST_ORDERED) return e->fail(SACTD3_EINVAL, "hindsight_info_device: unknown flag");
  if ((offset && offset_ld < 1) || (goal_slot && goal_slot_ld < 1)) return e->fail(SACTD3_EINVAL, "hindsight_info_device: a row stride is below 1");
  if (offset) RCCHK(device_ptr_check(e, offset, "hindsight_info_device", "offset"));
  if (goal_slot) RCCHK(device_ptr_check(e, goal_slot, "hindsight_info_device", "goal_slot"));
  if (!e->slot.hindsight || e->slot.cur != 0)
    return e->fail(SACTD3_ESTATE, "hindsight_info_device: the batch slot was not filled by a hindsight staging call");
  const hipStream_t caller = (hipStream_t)caller_stream;
  RCCHK(src_order_begin(e, caller, flags));
  const NstepInfoArgs g{e->hs_off, e->hs_gs, e->B, offset, (long)offset_ld, goal_slot, (long)goal_slot_ld};
  EnqCtx x{e, e->stream};
  LAUNCH_ON(k_nstep_info, dim3((unsigned)((e->B + 255) / 256)), dim3(256), g);
  RCCHK(src_order_end(e, caller, flags));
  return 0;
}
// {native draws, rows relabelled, rows refused, rows whose relabelled reward is 0}: the last three are device words
int sactd3_hindsight_stats(sactd3_engine* e, int64_t out[4]) {
  return (!e || !out) ? SACTD3_EINVAL : stats_with_words(e, &e->hs_calls, e->hs_ctr, 3, 1, out);
}

// loss weights for whatever slot 0 holds (a caller-owned device batch, an index-staged one); NULL drops them
int sactd3_batch_weights_device(sactd3_engine* e, const float* w, int64_t w_ld, int n, void* caller_stream, int flags) {
  if (!e) return SACTD3_EINVAL;
  USE_DEVICE(e);
  if (flags & ~SACTD3_SRC_ORDERED) return e->fail(SACTD3_EINVAL, "batch_weights_device: unknown flag");
  if (n != e->B) return e->fail(SACTD3_EINVAL, "batch_weights_device: n must equal batch_size");
  if (!w) { slot_set_weighted(e, false); return 0; }
  if (w_ld < 1) return e->fail(SACTD3_EINVAL, "batch_weights_device: row stride of `w` is below its width");
  RCCHK(device_ptr_check(e, w, "batch_weights_device", "w"));
  CHAIN_BREAK(e);
  RCCHK(slot_weights_alloc(e));
  const hipStream_t caller = (hipStream_t)caller_stream;
  EnqCtx x{e, e->stream};
  RCCHK(src_order_begin(e, caller, flags));
  RCCHK(launch_batch_weights(x, w, w_ld));
  RCCHK(src_order_end(e, caller, flags));
  slot_set_weighted(e, true);
  ++e->prio_stats[1];
  return 0;
}

// q_k(i) - y(i) of the most recent critic update, left in the caller's device array: one k_td_to_field launch on the learner stream.
// Reads e->q / e->y only; no CHAIN_BREAK: a precomputed opening pair stays valid across it.
int sactd3_td_errors_device(sactd3_engine* e, float* td, int64_t td_ld, int64_t td_ns, void* caller_stream, int flags) {
  if (!e) return SACTD3_EINVAL;
  if (!td) return e->fail(SACTD3_EINVAL, "td_errors_device: `td` is NULL");
  USE_DEVICE(e);
  if (flags & ~SACTD3_DST_ORDERED) return e->fail(SACTD3_EINVAL, "td_errors_device: unknown flag");
  if (td_ld < 1 || td_ns < 1) return e->fail(SACTD3_EINVAL, "td_errors_device: a stride of `td` is below 1");
  RCCHK(device_ptr_check(e, td, "td_errors_device", "td"));
  if (!e->slot.td_valid) return e->fail(SACTD3_ESTATE, "td_errors_device: no critic update has run on the rows now in the batch slot");
  const hipStream_t caller = (hipStream_t)caller_stream;
  EnqCtx x{e, e->stream};
  RCCHK(src_order_begin(e, caller, flags));
  RCCHK(launch_td_out(x, td, td_ld, td_ns));
  RCCHK(src_order_end(e, caller, flags));
  ++e->prio_stats[2];
  return 0;
}

int sactd3_priority_stats(sactd3_engine* e, int64_t out[4]) { return (!e || !out) ? SACTD3_EINVAL : stats_with_words(e, e->prio_stats, &e->ctl->priority_refused, 1, 3, out); }

// ---- proportional prioritised replay as engine state (include/sactd3.h: sactd3_prio_*; the sample itself: stage_ring_rows)
// One leaf per ring slot plus the group sums, built for the rows the ring holds now (priority 1 = the starting maximum).
int sactd3_prio_enable(sactd3_engine* e, float alpha, float eps) {
  if (!e) return SACTD3_EINVAL;
  USE_DEVICE(e);
  if (!(alpha >= 0.f) || !std::isfinite(alpha)) return e->fail(SACTD3_EINVAL, "prio_enable: alpha must be finite and >= 0");
  if (!(eps > 0.f) || !std::isfinite(eps)) return e->fail(SACTD3_EINVAL, "prio_enable: eps must be finite and > 0");
  if (e->pt_on) return (alpha == e->pt_alpha && eps == e->pt_eps) ? 0 : e->fail(SACTD3_ESTATE, "prio_enable: already enabled with other values");
  if (e->rb_pinned > 0) return e->fail(SACTD3_ESTATE, "prio_enable: rows are pinned (sactd3_rb_pin): the priority refresh assumes one wrap point, at slot 0");
  const int64_t groups = ((int64_t)e->cfg.rb_capacity + PRIO_G - 1) / PRIO_G, chunks = (groups + PRIO_G - 1) / PRIO_G;
  RCCHK(first_use_alloc(e, &e->pt_leaf, (size_t)groups * PRIO_G)); RCCHK(first_use_alloc(e, &e->pt_sums, (size_t)chunks * PRIO_G));
  RCCHK(first_use_alloc(e, &e->pt_ctl, 1, false));      // (never zeroed: the copy below, done when it returns, writes all of it)
  RCCHK(first_use_alloc(e, &e->pt_idx, (size_t)e->B)); RCCHK(first_use_alloc(e, &e->pt_dleaf, (size_t)e->B)); RCCHK(first_use_alloc(e, &e->pt_w, (size_t)e->B));
  RCCHK(first_use_alloc(e, &e->pt_total, 4)); RCCHK(first_use_alloc(e, &e->pt_u, (size_t)e->B));
  RCCHK(slot_weights_alloc(e));
  PrioCtl h{};
  h.max_prio = 1.f;
  HIPCHK(hipMemcpy(e->pt_ctl, &h, sizeof(h), hipMemcpyHostToDevice));
  e->pt_groups = (int)groups; e->pt_alpha = alpha; e->pt_eps = eps; e->pt_on = true;
  EnqCtx x{e, e->stream};
  return prio_after_append(x, 0, e->rb_len);
}

int sactd3_prio_set_uniforms(sactd3_engine* e, const float* u, int n) {
  if (!e) return SACTD3_EINVAL;
  USE_DEVICE(e);
  if (!e->pt_on) return state_refusal(e, "prio_set_uniforms", PRIO_OFF);
  if (!u) { e->pt_inject = false; return 0; }
  if (n != e->B) return e->fail(SACTD3_EINVAL, "prio_set_uniforms: n must equal batch_size");
  std::vector<float> h((size_t)n);
  for (int i = 0; i < n; ++i) h[i] = u[i] >= 0.f ? std::min(u[i], 0x1.fffffep-1f) : 0.f;      // into [0, 1); NaN -> 0
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(e->pt_u, h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice));
  e->pt_inject = true;
  return 0;
}

static inline void prio_update_issued(sactd3_engine* e) { ++e->pt_host[1]; }      // a write-back was launched (pt_host: {samples, write-backs, ..})
// The write-back from the critic update that just ran on the batch slot: one k_prio_update launch.  It reads e->q / e->y and the slot's
// ring indices and writes the priority table only: no CHAIN_BREAK, a precomputed opening pair of sactd3_step_period stays valid.
int sactd3_prio_update_from_td(sactd3_engine* e) {
  if (!e) return SACTD3_EINVAL;
  USE_DEVICE(e);
  if (!e->pt_on) return state_refusal(e, "prio_update_from_td", PRIO_OFF);
  if (!e->slot.td_valid) return e->fail(SACTD3_ESTATE, "prio_update_from_td: no critic update has run on the rows now in the batch slot");
  EnqCtx x{e, e->stream};
  RCCHK(launch_prio_update(x, prio_td_args(e, e->slot.cur)));
  prio_update_issued(e);
  return 0;
}

int sactd3_prio_update_device(sactd3_engine* e, const int64_t* idx, int64_t idx_ld, const float* prio, int64_t prio_ld, int n,
                              void* caller_stream, int flags) {
  if (!e) return SACTD3_EINVAL;
  if (!idx || !prio) return e->fail(SACTD3_EINVAL, "prio_update_device: `idx` or `prio` is NULL");
  USE_DEVICE(e);
  if (flags & ~SACTD3_SRC_ORDERED) return e->fail(SACTD3_EINVAL, "prio_update_device: unknown flag");
  if (n < 1) return e->fail(SACTD3_EINVAL, "prio_update_device: n must be at least 1");
  if (idx_ld < 1 || prio_ld < 1) return e->fail(SACTD3_EINVAL, "prio_update_device: a row stride is below 1");
  RCCHK(device_ptr_check(e, idx, "prio_update_device", "idx"));
  RCCHK(device_ptr_check(e, prio, "prio_update_device", "prio"));
  if (!e->pt_on) return state_refusal(e, "prio_update_device", PRIO_OFF);
  const hipStream_t caller = (hipStream_t)caller_stream;
  EnqCtx x{e, e->stream};
  RCCHK(src_order_begin(e, caller, flags));
  PrioUpdateArgs g{};
  g.n = n; g.idx = (const long long*)idx; g.idx_ld = (long)idx_ld; g.prio = prio; g.prio_ld = (long)prio_ld;
  RCCHK(launch_prio_update(x, g));
  RCCHK(src_order_end(e, caller, flags));
  prio_update_issued(e);
  return 0;
}

int sactd3_prio_stats(sactd3_engine* e, int64_t out[4]) {      // (the device word stands third)
  return (!e || !out) ? SACTD3_EINVAL : stats_with_words(e, e->pt_host, e->pt_on ? &e->pt_ctl->refused : nullptr, 1, 2, out);
}

// k and the last ring slot of every row of an n-step slot, left in the caller's device arrays: one k_nstep_info launch on the learner
// stream.  Reads the two per-slot arrays only; no CHAIN_BREAK.
int sactd3_nstep_info_device(sactd3_engine* e, int32_t* k, int64_t k_ld, int32_t* last, int64_t last_ld, void* caller_stream, int flags) {
  if (!e) return SACTD3_EINVAL;
  if (!k && !last) return e->fail(SACTD3_EINVAL, "nstep_info_device: `k` and `last` are both NULL");
  USE_DEVICE(e);
  if (flags & ~SACTD3_DST_ORDERED) return e->fail(SACTD3_EINVAL, "nstep_info_device: unknown flag");
  if ((k && k_ld < 1) || (last && last_ld < 1)) return e->fail(SACTD3_EINVAL, "nstep_info_device: a row stride is below 1");
  if (k) RCCHK(device_ptr_check(e, k, "nstep_info_device", "k"));
  if (last) RCCHK(device_ptr_check(e, last, "nstep_info_device", "last"));
  if (!e->slot.nstep || e->slot.cur != 0) return e->fail(SACTD3_ESTATE, "nstep_info_device: the batch slot was not filled by an n-step staging call");
  const hipStream_t caller = (hipStream_t)caller_stream;
  RCCHK(src_order_begin(e, caller, flags));
  const NstepInfoArgs g{e->ns_k, e->ns_last, e->B, k, (long)k_ld, last, (long)last_ld};
  EnqCtx x{e, e->stream};
  LAUNCH_ON(k_nstep_info, dim3((unsigned)((e->B + 255) / 256)), dim3(256), g);
  RCCHK(src_order_end(e, caller, flags));
  return 0;
}

int sactd3_nstep_stats(sactd3_engine* e, int64_t out[4]) {
  return (!e || !out) ? SACTD3_EINVAL : stats_with_words(e, e->ns_host, e->ns_ctr, 2, 2, out);
}

int sactd3_rb_fill_synthetic(sactd3_engine* e, int64_t n, uint64_t seed) {
  if (!e) return SACTD3_EINVAL;
  USE_DEVICE(e);
  CHAIN_BREAK(e);
  if (n < 1 || n > e->cfg.rb_capacity) return e->fail(SACTD3_EINVAL, "rb_fill_synthetic: 1 <= n <= rb_capacity");
  if (e->rb_pinned > 0) return e->fail(SACTD3_ESTATE, "rb_fill_synthetic: rows are pinned (sactd3_rb_pin): the fill writes from slot 0");
  FillArgs f{(float4*)e->ring, e->rec4, e->cx, e->cn, e->o, e->a, (long)n, seed, e->min_ac, e->max_ac};
  const long threads = (long)n * e->rec4;
  EnqCtx x{e, e->stream};
  LAUNCH_ON(k_rb_fill, dim3((unsigned)((threads + 255) / 256)), dim3(256), f);
  e->rb_len = std::max<int64_t>(e->rb_len, n);
  e->rb_cursor = n % e->cfg.rb_capacity;
  RCCHK(publish_rb_state(x));
  return prio_after_append(x, 0, n);
}

// ---- noise
int sactd3_set_noise(sactd3_engine* e, int site, const float* eps, int n) {
  if (!e || !eps || site < 0 || site >= SACTD3_NUM_SITES) return SACTD3_EINVAL;
  USE_DEVICE(e);
  CHAIN_BREAK(e);
  if (n < 1 || n > std::max(e->B, e->maxn)) return e->fail(SACTD3_EINVAL, "set_noise: too many rows");
  if (e->act_inflight && site == SACTD3_SITE_PREDICT) return e->fail(SACTD3_ESTATE, "set_noise: an acting call is in flight (sactd3_predict_end first)");
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(e->eps[site], eps, sizeof(float) * (size_t)n * e->a, hipMemcpyHostToDevice));
  if (site == SACTD3_SITE_CRITIC)      // (every batch slot: injected draws are "sticky until cleared", whichever slot an iteration trains on)
    for (int k = 1; k < 4; ++k) HIPCHK(hipMemcpy(e->bs[k].eps_c, eps, sizeof(float) * (size_t)n * e->a, hipMemcpyHostToDevice));
  const int one = 1;
  HIPCHK(hipMemcpy(&e->ctl->inject_eps[site], &one, sizeof(int), hipMemcpyHostToDevice));
  return 0;
}
int sactd3_clear_noise(sactd3_engine* e, int site) {
  if (!e || site >= SACTD3_NUM_SITES) return SACTD3_EINVAL;
  USE_DEVICE(e);
  if (e->act_inflight && (site < 0 || site == SACTD3_SITE_PREDICT)) return e->fail(SACTD3_ESTATE, "clear_noise: an acting call is in flight (sactd3_predict_end first)");
  CHAIN_BREAK(e);
  HIPCHK(hipStreamSynchronize(e->stream));
  const int zeros[8] = {0};
  if (site < 0) HIPCHK(hipMemcpy(&e->ctl->inject_eps[0], zeros, sizeof(int) * 8, hipMemcpyHostToDevice));
  else HIPCHK(hipMemcpy(&e->ctl->inject_eps[site], zeros, sizeof(int), hipMemcpyHostToDevice));
  return 0;
}
int sactd3_read_noise(sactd3_engine* e, int site, float* eps, int n) {
  if (!e || !eps || site < 0 || site >= SACTD3_NUM_SITES || n < 1 || n > std::max(e->B, e->maxn)) return SACTD3_EINVAL;
  USE_DEVICE(e);
  if (e->act_inflight && site == SACTD3_SITE_PREDICT) return e->fail(SACTD3_ESTATE, "read_noise: an acting call is in flight (sactd3_predict_end first)");
  HIPCHK(hipStreamSynchronize(e->stream));
  const float* src = site == SACTD3_SITE_CRITIC ? e->bs[e->slot.cur].eps_c : e->eps[site];
  HIPCHK(hipMemcpy(eps, src, sizeof(float) * (size_t)n * e->a, hipMemcpyDeviceToHost));
  return 0;
}

// ---- updates
// a critic update on the rows a refill left in slot 0 was launched: the critics' gradient arenas were written in full (grads_stale)
static inline void update_qnets_issued(sactd3_engine* e) { e->grads_stale[0] = false; slot_trained(e, 0, false); }
int sactd3_update_qnets(sactd3_engine* e) {
  if (!e) return SACTD3_EINVAL;
  USE_DEVICE(e);
  CHAIN_BREAK(e);
  RCCHK(run_graph(e, e->slot.weighted ? G_QW : G_Q));      // the weighted form: the same sequence with the weighted critic tail, a graph of its own
  update_qnets_issued(e);
  return 0;
}
int sactd3_update_actor(sactd3_engine* e) {
  if (!e) return SACTD3_EINVAL;
  USE_DEVICE(e);
  CHAIN_BREAK(e);
  RCCHK(actor_write_begin(e));
  RCCHK(run_graph(e, G_A));
  e->grads_stale[1] = false;
  return 0;
}
int sactd3_update_targ_nets(sactd3_engine* e, int64_t qnet_updates_so_far) {
  if (!e) return SACTD3_EINVAL;
  USE_DEVICE(e);
  CHAIN_BREAK(e);
  const bool td3 = e->cfg.prefer_td3_over_sac;
  EnqCtx x{e, e->stream};
  if (td3 || qnet_updates_so_far % e->cfg.crit_targ_update_freq == 0) return enqueue_polyak(x, POLYAK_CRITICS | (td3 ? POLYAK_ACTOR : 0));
  return 0;
}
// The schedule of the iteration that brings the critics to their `updates`-th update (orchestrator.py:337-352): does it run the actor
// updates, does it update the targets, and k = 2 act + polyak, its place among the four graphs of G_STEP00 + k / G_SAMPLED + k.
struct IterSchedule { bool act, polyak; int k; };
static IterSchedule iteration_schedule(const sactd3_engine* e, int do_actor, int64_t updates) {
  const bool polyak = e->cfg.prefer_td3_over_sac || (updates % e->cfg.crit_targ_update_freq == 0);
  const bool act = do_actor != 0 && e->cfg.actor_update_delay > 0;
  return {act, polyak, (act ? 2 : 0) + (polyak ? 1 : 0)};
}
// the next iteration as graph `first` + k (G_STEP00, G_SAMPLED, G_CYCLE + 4 exploit), and what it does to the counter and to grads_stale
static int issue_iteration(sactd3_engine* e, int do_actor, int first) {
  const IterSchedule s = iteration_schedule(e, do_actor, e->qnet_updates + 1);
  if (s.act) RCCHK(actor_write_begin(e));      // (a critic-only iteration touches nothing the acting kernels read: no order with them)
  RCCHK(run_graph(e, first + s.k));
  ++e->qnet_updates;      // (the engine's own counter advances only once the iteration has been launched)
  e->grads_stale[0] = false;
  if (s.act) e->grads_stale[1] = false;
  return 0;
}
int sactd3_step(sactd3_engine* e, int do_actor) {
  if (!e) return SACTD3_EINVAL;
  USE_DEVICE(e);
  CHAIN_BREAK(e);
  if (e->rb_len <= 0) return e->fail(SACTD3_ESTATE, "step: buffer is empty");
  RCCHK(issue_iteration(e, do_actor, G_STEP00));
  slot_trained(e, 0, true);
  return 0;
}

// The iteration with a prioritised draw and / or n-step returns as ONE graph launch (include/sactd3.h); preceded by one k_set_int2
// launch only when beta or the injection switch differ from what PrioCtl holds.  Refusals first; a refused call has changed nothing.
int sactd3_step_sampled(sactd3_engine* e, int do_actor, const sactd3_sampling* sm) {
  if (!e) return SACTD3_EINVAL;
  USE_DEVICE(e);
  if (!sm) return e->fail(SACTD3_EINVAL, "step_sampled: the sampling struct is NULL");
  if (sm->draw != SACTD3_DRAW_UNIFORM && sm->draw != SACTD3_DRAW_PRIORITIZED && sm->draw != SACTD3_DRAW_MIXED && sm->draw != SACTD3_DRAW_HINDSIGHT)
    return e->fail(SACTD3_EINVAL, "step_sampled: unknown draw");
  if (sm->n_step < 1 || sm->n_step > NS_MAX) return e->fail(SACTD3_EINVAL, "step_sampled: n_step must be in [1, 16]");
  if (sm->n_step > 1 && sm->stride < 1) return e->fail(SACTD3_EINVAL, "step_sampled: stride must be at least 1");
  const bool prio = sm->draw == SACTD3_DRAW_PRIORITIZED, mixed = sm->draw == SACTD3_DRAW_MIXED, hind = sm->draw == SACTD3_DRAW_HINDSIGHT;
  if (mixed && sm->n_step != 1) return e->fail(SACTD3_EINVAL, "step_sampled: the mixed draw has no n-step form: n_step must be 1");
  if (hind && sm->n_step != 1) return e->fail(SACTD3_EINVAL, "step_sampled: the hindsight draw has no n-step form: n_step must be 1");
  if (!(sm->beta >= 0.f) || !std::isfinite(sm->beta)) return e->fail(SACTD3_EINVAL, "step_sampled: beta must be finite and >= 0");
  const bool chain = sm->n_step > 1;
  const Draw d{sm->draw, sm->beta, chain ? sm->n_step : 0, chain ? sm->stride : 0};
  if (const char* why = draw_state_refusal(e, d)) return state_refusal(e, "step_sampled", why);
  if (!prio && !mixed && !hind && !chain) { RCCHK(sactd3_step(e, do_actor)); ++e->ss_stats[0]; return 0; }
  CHAIN_BREAK(e);
  RCCHK(draw_alloc(e, d));
  EnqCtx x{e, e->stream};      // (the eager launches in front of the graph)
  if (!d.same_graphs(e->ss_draw)) RCCHK(drop_graphs(e, G_SAMPLED, 4));
  e->ss_draw = d;
  if (prio) {
    int32_t bits;
    memcpy(&bits, &sm->beta, sizeof(bits));
    const int inject = e->pt_inject ? 1 : 0;
    if ((int64_t)(uint32_t)bits != e->ss_beta_bits || inject != e->ss_inject) {
      RCCHK(launch_set_int2(x, reinterpret_cast<int*>(&e->pt_ctl->beta), (int)bits, inject));
      e->ss_beta_bits = (int64_t)(uint32_t)bits; e->ss_inject = inject;
    }
  }
  if (mixed) RCCHK(mix_publish(x));      // (P and m as the graph's draw reads them: a launch only when one of them changed)
  if (hind) RCCHK(hindsight_publish(x));      // (the draw counter as the graph's draw reads it: a launch only behind a call-form native draw)
  RCCHK(issue_iteration(e, do_actor, G_SAMPLED));
  ++e->ss_stats[0];
  // the rest of the host state: what the calls of the sequence leave, by their own routines
  draw_issued(e, d, true);
  update_qnets_issued(e);
  if (prio) prio_update_issued(e);
  return 0;
}
int sactd3_step_sampled_stats(sactd3_engine* e, int64_t out[4]) { return host_stats(e, &sactd3_engine::ss_stats, out); }

// Is the period graph built in its pipelined form (see BatchSlot)?  One or two critic-only iterations behind the one with the actor
// updates, and an opening trunk that reads ring rows itself (narrow observations below the large-batch threshold, wide ones at large batch).
// does the actor's weight-gradient launch take the split-M route (k_tn64 + k_adam_red: no T2 / T3 support)?  (launch_tn's rule)
static bool actor_dw_is_tiled64(const sactd3_engine* e) {
  return tn_is_tiled64(e, e->B, tn64_tiles(e->nh, HID) + tn64_tiles(HID, HID) + tn64_tiles(HID, e->La.ld1));   // head, layer 2, layer 1
}
static bool period_is_pipelined(const sactd3_engine* e) {
  const sactd3_config& c = e->cfg;
  if (c.actor_update_delay < 1 || c.actor_update_delay > 2 || !opening_trunk_gathers(e)) return false;
  // SAC: needs the temperature draw's trunk + tail pair at the end of the last actor update (autotune);
  // TD3: the run-ahead through the target actors of the next Polyak updates (T2 / T3 in the k_tn epilogue: no gradient clipping,
  // no split-M route for the actor's weight gradients)
  if (c.prefer_td3_over_sac) return c.clip_norm <= 0.f && !actor_dw_is_tiled64(e);
  return c.autotune != 0;
}
// a period / cut-short period sequence was issued: what debug_read may no longer hand out (sactd3_engine::grads_stale)
static void mark_grads_stale(sactd3_engine* e) {
  if (e->cfg.clip_norm > 0.f) return;
  e->grads_stale[0] = true;
  if (e->cfg.actor_update_delay > 0) e->grads_stale[1] = true;
}
// The first m iterations of a period, m = delay + 1: all of it (sactd3_step_period); fewer: the period graph cut short (pipelined form
// only, sactd3_step_prefix) -- nothing is left behind for a next period.  Pipelined: the iteration with the actor updates on the
// precomputed opening pair of its slot, with the sampling and next-action passes of the m - 1 critic-only iterations behind it run ahead
// (and, the whole period, the next period's opening pair into the other slot); then those iterations on slots 1 .. m - 1.
// variant (pipelined form only): which batch slot the period's first iteration trains on (0: slot 0, 1: slot 3) -- the other one
// receives the opening pair of the NEXT period, so consecutive periods alternate (chain_ready).  The pipelined form assumes its own
// opening pair is already in place: take_opening runs the opening graph first when it is not.
static int enqueue_period(EnqCtx& x, int variant, int m) {
  sactd3_engine* e = x.e;
  const bool pipelined = period_is_pipelined(e), whole = m == e->cfg.actor_update_delay + 1;
  x.lean_stores = e->cfg.clip_norm <= 0.f;      // (see sactd3_engine::grads_stale)
  for (int i = 0; i < m; ++i) {
    IterPlace it;
    it.actor = i == 0 && e->cfg.actor_update_delay > 0; it.targets = true; it.more = i + 1 < m;
    if (pipelined) { it.slot = period_slot(true, variant, i); it.pre_sampled = true; }
    if (pipelined && i == 0) { it.ahead = m - 1; it.chain_slot = whole ? (variant ? 0 : 3) : -1; }
    RCCHK(enqueue_step(x, it));
  }
  return 0;
}
// The opening graph: the opening pair of a period's first iteration into batch slot 0, its counter ticks left to the period graph
static int enqueue_opening(EnqCtx& x) {
  if (!opening_merges_policy(x.e)) return x.e->fail(SACTD3_ESTATE, "opening graph: the policy pass did not merge");
  IterPlace it;
  it.actor = true; it.pre_sampled = true;
  return enqueue_opening_pair(x, it, true);
}

// Runs of whole periods.  The device idles for a few microseconds between the last node of one graph replay and the first of the next
// (DESIGN.md 8), so a loop of period graphs pays that once per period; a graph that holds RUN_PERIODS consecutive pipelined periods
// pays it once per run.  RUN_PERIODS is even, so a run ends on the variant it started on, and at most 8 (make RUN=<R>).
#ifndef SACTD3_RUN_PERIODS
#define SACTD3_RUN_PERIODS 2
#endif
static const int RUN_PERIODS = SACTD3_RUN_PERIODS;
static_assert(RUN_PERIODS >= 2 && RUN_PERIODS <= 8 && RUN_PERIODS % 2 == 0, "SACTD3_RUN_PERIODS: an even number of periods, 2 .. 8");
// RUN_PERIODS pipelined periods from variant v on, as one sequence: what enqueue_period(x, v, n), enqueue_period(x, 1 - v, n), ...
// issue one behind the other -- a period leaves nothing deferred behind, so the launches are those of the single periods, one for one
static int enqueue_period_run(EnqCtx& x, int v) {
  for (int r = 0; r < RUN_PERIODS; ++r) {
    RCCHK(enqueue_period(x, (v + r) & 1, x.e->cfg.actor_update_delay + 1));
    if (x.alpha_pending || x.alpha_tick_owed) return x.e->fail(SACTD3_ESTATE, "period run: a period left a deferred temperature step behind");
  }
  return 0;
}
// What each learner graph holds (see run_graph): one definition for whoever captures it -- its entry point at the first use,
// sactd3_instantiate_graphs ahead of that -- and whoever walks its sequence without a graph (use_graphs == 0, sactd3_time_nodes).
static int enqueue_cycle(EnqCtx& x, const CycleBinding& b, bool explore, bool act, bool polyak);      // (the rollout cycle, at the end of this file)
static int enqueue_graph(EnqCtx& x, int which) {
  sactd3_engine* e = x.e;
  IterPlace api;      // (the API path's updates: no place in a fused iteration)
  api.weighted = which == G_QW;
  switch (which) {
    case G_Q: case G_QW: return enqueue_update_qnets(x, api, false);
    case G_A: return enqueue_update_actor(x, api, 0, false);
    case G_STEP00: case G_STEP01: case G_STEP10: case G_STEP11:      // + IterSchedule::k
      return enqueue_step(x, single_iteration(((which - G_STEP00) & 2) != 0, ((which - G_STEP00) & 1) != 0));
    case G_PERIOD: case G_PERIOD_B: return enqueue_period(x, which - G_PERIOD, e->cfg.actor_update_delay + 1);
    case G_OPENING: return enqueue_opening(x);
    case G_PREFIX: case G_PREFIX + 1: case G_PREFIX + 2: case G_PREFIX + 3: return enqueue_period(x, (which - G_PREFIX) & 1, (which - G_PREFIX) / 2 + 1);
    case G_RUN: case G_RUN + 1: return enqueue_period_run(x, which - G_RUN);
    case G_SAMPLED: case G_SAMPLED + 1: case G_SAMPLED + 2: case G_SAMPLED + 3:      // + IterSchedule::k
      x.graph_form = true;
      return enqueue_step_sampled(x, ((which - G_SAMPLED) & 2) != 0, ((which - G_SAMPLED) & 1) != 0);
  }
  if (which >= G_CYCLE && which < G_CYCLE + 8)      // + (explore ? 0 : 4) + IterSchedule::k, for the binding the engine holds
    return enqueue_cycle(x, e->cyc, which - G_CYCLE < 4, ((which - G_CYCLE) & 2) != 0, ((which - G_CYCLE) & 1) != 0);
  return e->fail(SACTD3_EINVAL, "enqueue_graph: no such graph");
}

// what the period graphs need: every iteration takes the same target-update branch (TD3, or a target update with every critic update)
static bool same_target_branch(const sactd3_engine* e) { return e->cfg.prefer_td3_over_sac || e->cfg.crit_targ_update_freq == 1; }
// the preconditions the period entry points share; `who` is the entry point, for the message
static int period_refusal(sactd3_engine* e, const char* who) {
  if (e->rb_len <= 0) return e->fail(SACTD3_ESTATE, (std::string(who) + ": buffer is empty").c_str());
  if (!same_target_branch(e)) return e->fail(SACTD3_ESTATE, (std::string(who) + ": needs crit_targ_update_freq == 1").c_str());
  return 0;
}
// Chained periods: the opening pair of a pipelined (cut-short) period is either left over from the previous one (chain_ready names the
// variant, *v) or is produced now by the 2- / 3-node opening graph; taken either way -- a failure further on leaves no pair to rely on.
// A period that is not pipelined has no pair: variant 0, and nothing to rely on behind it either.
static int take_opening(sactd3_engine* e, bool pipelined, int* v) {
  const bool have = pipelined && e->chain_ready >= 0;
  *v = have ? e->chain_ready : 0;
  e->chain_ready = -1;
  if (pipelined && !have) RCCHK(run_graph(e, G_OPENING));
  return 0;
}
// what the host knows behind a launch of `periods` periods, the last of them m iterations long on variant v
// (a period's iterations run one behind the other, each writing e->q / e->y in its critic tail; what runs ahead inside the first one
//  -- the later iterations' and the next period's opening passes -- goes through the actor only: the current slot, e->q and e->y all
//  belong to the last iteration issued; m == 1 on variant 1: slot 3)
static void periods_issued(sactd3_engine* e, bool pipelined, int v, int m, int periods = 1) {
  e->qnet_updates += (int64_t)periods * m;
  slot_trained(e, period_slot(pipelined, v, m - 1), true);
}
// k whole periods.  Pipelined: RUN_PERIODS to a graph launch, what is left of k below that through the single-period graphs, each period
// graph leaving the NEXT period's opening pair behind; otherwise G_PERIOD k times.  The host state moves launch by launch, so a launch that
// fails leaves it where the launches that were issued put it.  launches: {run launches, single-period launches}, counted as they go out.
static int issue_periods(sactd3_engine* e, int k, int64_t launches[2]) {
  const bool pipelined = period_is_pipelined(e);
  const int n = e->cfg.actor_update_delay + 1;
  RCCHK(actor_write_begin(e));
  mark_grads_stale(e);
  int v = 0;
  RCCHK(take_opening(e, pipelined, &v));
  for (int left = k; left > 0;) {
    const int periods = pipelined && left >= RUN_PERIODS ? RUN_PERIODS : 1;
    RCCHK(run_graph(e, periods > 1 ? G_RUN + v : G_PERIOD + v));
    ++launches[periods > 1 ? 0 : 1];
    const int last = (v + periods - 1) & 1;      // the variant of the last period issued
    v = pipelined ? 1 - last : 0;
    left -= periods;
    periods_issued(e, pipelined, last, n, periods);
    e->chain_ready = pipelined && left == 0 ? v : -1;      // (named only once the call is through)
  }
  return 0;
}

// One period of the actor schedule (orchestrator.py:345-349: iteration i with i % (delay + 1) == 0 runs the actor updates,
// the next `delay` iterations are critic-only) as ONE graph launch: delay + 1 iterations back to back, no host call and no
// inter-replay gap in between.  Only when every iteration takes the same target-update branch (same_target_branch); otherwise the
// caller gets SACTD3_ESTATE and issues the iterations one by one.
int sactd3_step_period(sactd3_engine* e) {
  if (!e) return SACTD3_EINVAL;
  USE_DEVICE(e);
  RCCHK(period_refusal(e, "step_period"));
  int64_t uncounted[2] = {};      // (run_stats counts what sactd3_step_periods issues)
  return issue_periods(e, 1, uncounted);
}

// The first m iterations of a period (1 <= m <= actor_update_delay) as ONE graph launch: what is left of a run of iterations behind
// its last whole period (orchestrator.py:337-352 for a number of iterations that is not a multiple of the period).  Equal to
// sactd3_step(1) followed by m - 1 sactd3_step(0), bit for bit; in the pipelined form it takes the opening pair exactly as a whole
// period does, and leaves none behind.  Same preconditions as sactd3_step_period.
int sactd3_step_prefix(sactd3_engine* e, int m) {
  if (!e) return SACTD3_EINVAL;
  USE_DEVICE(e);
  if (m < 1 || m > e->cfg.actor_update_delay) return e->fail(SACTD3_EINVAL, "step_prefix: 1 <= m <= actor_update_delay");
  RCCHK(period_refusal(e, "step_prefix"));
  if (!period_is_pipelined(e) || m > 2) {      // no cut-short form: the iterations one by one
    for (int i = 0; i < m; ++i) RCCHK(sactd3_step(e, i == 0));
    return 0;
  }
  RCCHK(actor_write_begin(e));
  mark_grads_stale(e);
  int v = 0;
  RCCHK(take_opening(e, true, &v));
  RCCHK(run_graph(e, G_PREFIX + 2 * (m - 1) + v));
  periods_issued(e, true, v, m);
  return 0;
}

// k whole periods: equal to k sactd3_step_period calls, bit for bit (issue_periods; sactd3_step_period is its k == 1).
int sactd3_step_periods(sactd3_engine* e, int k) {
  if (!e) return SACTD3_EINVAL;
  USE_DEVICE(e);
  if (k < 1) return e->fail(SACTD3_EINVAL, "step_periods: k >= 1");
  RCCHK(period_refusal(e, "step_periods"));
  ++e->run_stats[0];
  return issue_periods(e, k, &e->run_stats[1]);
}
int sactd3_step_periods_stats(sactd3_engine* e, int64_t out[4]) { return host_stats(e, &sactd3_engine::run_stats, out); }

// Capture + instantiate the graphs of sactd3_step (both schedules, with the target update) and of sactd3_step_period / _prefix /
// _periods now instead of at their first use, without launching anything: a caller that times its first iterations (or must not
// stall in the loop) calls this once after sactd3_create.  No-op with use_graphs == 0.
int sactd3_instantiate_graphs(sactd3_engine* e) {
  if (!e) return SACTD3_EINVAL;
  USE_DEVICE(e);
  for (int act = 0; act < 2; ++act) {      // the schedules of the first update and of one with a target update: the same unless that is gated
    RCCHK(run_graph(e, G_STEP00 + iteration_schedule(e, act, 1).k, false));
    RCCHK(run_graph(e, G_STEP00 + iteration_schedule(e, act, e->cfg.crit_targ_update_freq).k, false));
  }
  if (!same_target_branch(e) || e->cfg.actor_update_delay <= 0) return 0;
  RCCHK(run_graph(e, G_PERIOD, false));
  if (!period_is_pipelined(e)) return 0;
  // the other variant, the opening graph, a run from either variant (sactd3_step_periods), and the cut-short periods of m = 1 (, 2)
  const int pipelined_ids[] = {G_PERIOD_B, G_OPENING, G_RUN, G_RUN + 1};
  for (int id : pipelined_ids) RCCHK(run_graph(e, id, false));
  for (int id = G_PREFIX; id < G_PREFIX + 2 * std::min(e->cfg.actor_update_delay, 2); ++id) RCCHK(run_graph(e, id, false));
  return 0;
}

// The acting launches of one call -- trunk (with the exploration draw riding along) + tail (+ a counter kernel behind a multi-block
// tail) -- on stream `s`: the learner's for sactd3_predict, the acting stream for sactd3_predict_begin.  The kernels read the
// observations from, and write the actions to, the pinned host buffers themselves (a few hundred bytes over the host link): two
// kernels and one synchronisation per call, no copy commands, no separate counter kernel.  Nothing in the launches depends on the
// call but (n, explore): they are captured once per pair and replayed, on either stream.
static bool predict_one_block(sactd3_engine* e, int n) {
  return n <= tail_rows_per_block(tail_args(e, e->p_z2, e->Pa, n, 0, 0, SACTD3_SITE_PREDICT, 48u, e->h_act, e->a4, 0, nullptr));
}
// `on_device`: the pair of sactd3_predict_device -- observations from p_x, actions to p_act (both engine-owned device memory), and no
// completion word: nobody on the host waits for it.
static int enqueue_predict(EnqCtx& x, int n, int explore, bool on_device = false) {
  sactd3_engine* e = x.e;
  const bool td3 = e->cfg.prefer_td3_over_sac;
  bool eps_ready = false;
  {
    const TrunkGrp g{on_device ? e->p_x : e->h_obs, e->Pa, e->p_z1, e->p_z2, nullptr, nullptr, nullptr};
    TrunkTicks tk{nullptr, nullptr, nullptr, nullptr, 0.f};
    if (explore) { tk.nnoise = 1; tk.noise[0] = noise_job(e, SACTD3_SITE_PREDICT, 48u, 0, n); tk.noise_taken = &eps_ready; }
    RCCHK(enqueue_trunk(x, e->ldo, e->o, n, e->La, 0, 1, 1, &g, tk));
  }
  const int mode = td3 ? (explore ? 2 : 0) : (explore ? 0 : 1);
  ActorTail t = tail_args(e, e->p_z2, e->Pa, n, mode, 0, SACTD3_SITE_PREDICT, 48u, on_device ? e->p_act : e->h_act, e->a4, 0, nullptr);
  t.eps_ready = eps_ready;
  // the tail reads predict_ctr (its noise stream) and may only advance it itself when it is a single block: with more
  // rows than one block holds, a late block could read the counter after block 0 has bumped it
  const bool one_block = n <= tail_rows_per_block(t);
  if (explore && one_block) t.tick = &e->ctl->predict_ctr;
  if (one_block && !on_device) { t.seq = &e->ctl->predict_seq; t.done_flag = e->h_done; }
  RCCHK(launch_tail(x, t));
  if (explore && !one_block) RCCHK(launch_tick(x, &e->ctl->predict_ctr));
  return 0;
}
static void predict_stage_obs(sactd3_engine* e, const float* obs, int n) {
  // (the pinned staging is free: every call returns -- sactd3_predict_end for a begun one -- only after its own kernels have finished)
  for (int i = 0; i < n; ++i) {
    memset(e->h_obs + (size_t)i * e->ldo, 0, sizeof(float) * e->ldo);
    memcpy(e->h_obs + (size_t)i * e->ldo, obs + (size_t)i * e->o, sizeof(float) * e->o);
  }
}
static int predict_launch(sactd3_engine* e, hipStream_t s, int n, int explore) {
  if (e->predict_graphs.empty()) e->predict_graphs.assign(2 * (size_t)(e->maxn + 1), nullptr);
  return run_graph_slot(e, &e->predict_graphs[(size_t)(explore ? 1 : 0) * (e->maxn + 1) + n], nullptr,
                        [&](EnqCtx& x) { return enqueue_predict(x, n, explore); }, true, s);
}
// completion: a single-block tail publishes the call's sequence number `want` to a pinned host word after its last store; spin on
// it (a stream synchronisation costs a marker packet and a signal wake-up on top of the kernels).  Anything unexpected, or a
// multi-block tail (spin == false): synchronise the stream.  *by_spin: the word ended the wait.
static int predict_wait(sactd3_engine* e, hipStream_t s, bool spin, int want, bool* by_spin) {
  bool done = false;
  *by_spin = false;
  if (spin) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int spins = 0; !done; ++spins) {
      done = __atomic_load_n(e->h_done, __ATOMIC_ACQUIRE) == want;
      if (!done && (spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    *by_spin = done;
    if (!done) {
      HIPCHK(hipStreamSynchronize(s));
      if (__atomic_load_n(e->h_done, __ATOMIC_ACQUIRE) != want) return e->fail(SACTD3_ESTATE, "predict: the acting kernels did not report completion");
      done = true;
    }
  }
  if (!done) HIPCHK(hipStreamSynchronize(s));
  return 0;
}

int sactd3_predict(sactd3_engine* e, const float* obs, int n, int explore, float* actions) {
  if (!e || !obs || !actions) return SACTD3_EINVAL;
  USE_DEVICE(e);
  if (n < 1 || n > e->maxn) return e->fail(SACTD3_EINVAL, "predict: 1 <= n <= max_envs");
  if (e->act_inflight) return e->fail(SACTD3_ESTATE, "predict: an acting call is in flight (sactd3_predict_end first)");
  predict_stage_obs(e, obs, n);
  RCCHK(predict_launch(e, e->stream, n, explore));
  const bool spin = predict_one_block(e, n);
  bool by_spin = false;
  RCCHK(predict_wait(e, e->stream, spin, spin ? ++e->predict_calls : 0, &by_spin));
  for (int i = 0; i < n; ++i) memcpy(actions + (size_t)i * e->a, e->h_act + (size_t)i * e->a4, sizeof(float) * e->a);
  return 0;
}

// sactd3_predict in two halves, the kernels on the acting stream: see include/sactd3.h.  The stream and its two events are made at
// the first call, so an engine that never acts this way holds exactly what it always held.
int sactd3_predict_begin(sactd3_engine* e, const float* obs, int n, int explore, int flags) {
  if (!e || !obs) return e ? e->fail(SACTD3_EINVAL, "predict_begin: null argument") : SACTD3_EINVAL;
  USE_DEVICE(e);
  if (n < 1 || n > e->maxn) return e->fail(SACTD3_EINVAL, "predict_begin: 1 <= n <= max_envs");
  if (flags & ~SACTD3_ACT_AFTER_ALL) return e->fail(SACTD3_EINVAL, "predict_begin: unknown flag");
  if (e->act_inflight) return e->fail(SACTD3_ESTATE, "predict_begin: an acting call is already in flight (sactd3_predict_end first)");
  if (!e->act_stream) {
    HIPCHK(hipStreamCreateWithFlags(&e->act_stream, hipStreamNonBlocking));
    if (!e->ev_learner) HIPCHK(hipEventCreateWithFlags(&e->ev_learner, hipEventDisableTiming));
    if (!e->ev_acting) HIPCHK(hipEventCreateWithFlags(&e->ev_acting, hipEventDisableTiming));
  }
  predict_stage_obs(e, obs, n);
  // learner -> acting: only behind an actor-parameter write (or on request) does the acting stream wait for the learner's
  const bool wait = e->actor_dirty || (flags & SACTD3_ACT_AFTER_ALL);
  if (wait) {
    HIPCHK(hipEventRecord(e->ev_learner, e->stream));
    HIPCHK(hipStreamWaitEvent(e->act_stream, e->ev_learner, 0));
    e->actor_dirty = false;
  }
  RCCHK(predict_launch(e, e->act_stream, n, explore));
  ++e->act_stats[0];
  if (wait) ++e->act_stats[1];
  e->act_spin = predict_one_block(e, n);
  e->act_want = e->act_spin ? ++e->predict_calls : 0;
  e->act_n = n; e->act_inflight = true; e->act_ordered = false;
  return 0;
}

int sactd3_predict_end(sactd3_engine* e, float* actions) {
  if (!e || !actions) return e ? e->fail(SACTD3_EINVAL, "predict_end: null argument") : SACTD3_EINVAL;
  USE_DEVICE(e);
  if (!e->act_inflight) return e->fail(SACTD3_ESTATE, "predict_end: no acting call in flight (sactd3_predict_begin first)");
  bool by_spin = false;
  const int rc = predict_wait(e, e->act_stream, e->act_spin, e->act_want, &by_spin);
  e->act_inflight = false; e->act_ordered = false;      // (whatever happened, the call is over: the engine stays usable)
  RCCHK(rc);
  if (by_spin) ++e->act_stats[3];
  for (int i = 0; i < e->act_n; ++i) memcpy(actions + (size_t)i * e->a, e->h_act + (size_t)i * e->a4, sizeof(float) * e->a);
  return 0;
}

static int launch_obs_pack(EnqCtx& x, const float* obs, int64_t obs_ld, float* rows, int n) {      // rows: n packed rows at ldo
  const ObsFieldArgs g{(float4*)rows, n, x.e->ldo / 4};
  const long chunks = (long)n * g.c4;
  LAUNCH_ON(k_obs_from_field, dim3(cpt_blocks(chunks, OBS_CPT)), dim3(256), obs, (long)obs_ld, x.e->o, g);
  return 0;
}
static int launch_act_unpack(EnqCtx& x, float* actions, int64_t actions_ld, int n) {
  const ActFieldArgs g{(const float4*)x.e->p_act, n, x.e->a4 / 4, x.e->a};
  const long chunks = (long)n * g.c4;
  LAUNCH_ON(k_act_to_field, dim3((unsigned)((chunks + 255) / 256)), dim3(256), actions, (long)actions_ld, g);
  return 0;
}

// The acting pair on n rows of p_x was queued on the learner stream.  The call returns with its kernels still queued, and they use the
// scratch, the draw buffer and the counter that an acting-stream call uses too: the next sactd3_predict_begin has to wait for the
// learner stream, exactly as behind a write of the actor.  pdev_stats: {calls, rows, ordered calls, calls with a multi-block tail}.
static void predict_device_issued(sactd3_engine* e, int n, bool ordered) {
  e->actor_dirty = true;
  ++e->pdev_stats[0]; e->pdev_stats[1] += n;
  if (ordered) ++e->pdev_stats[2];
  if (!predict_one_block(e, n)) ++e->pdev_stats[3];
}
// Agent.predict for observations that are ALREADY in this device's memory, actions left there: include/sactd3.h.  Four launches on
// the learner stream -- pack, the acting pair of sactd3_predict on p_x / p_act (its own (explore, n) graph, or the eager sequence),
// unpack -- five behind an exploring multi-block tail (the counter kernel is part of the pair); the caller's pointers travel by value
// in the two eager launches, so no graph is ever updated or re-instantiated.  Nothing waits on the host.
int sactd3_predict_device(sactd3_engine* e, const float* obs, int64_t obs_ld, int n, int explore, float* actions, int64_t actions_ld,
                          void* caller_stream, int flags) {
  if (!e) return SACTD3_EINVAL;
  if (!obs || !actions) return e->fail(SACTD3_EINVAL, "predict_device: null argument");
  USE_DEVICE(e);
  if (n < 1 || n > e->maxn) return e->fail(SACTD3_EINVAL, "predict_device: 1 <= n <= max_envs");
  if (flags & ~SACTD3_SRC_ORDERED) return e->fail(SACTD3_EINVAL, "predict_device: unknown flag");
  if (obs_ld < e->o) return e->fail(SACTD3_EINVAL, "predict_device: row stride of `obs` is below its width");
  if (actions_ld < e->a) return e->fail(SACTD3_EINVAL, "predict_device: row stride of `actions` is below its width");
  if ((int64_t)n * std::max(e->ldo, e->a4) / 4 >= (1ll << 31)) return e->fail(SACTD3_EINVAL, "predict_device: too many rows for one launch");
  RCCHK(device_ptr_check(e, obs, "predict_device", "obs"));
  RCCHK(device_ptr_check(e, actions, "predict_device", "actions"));
  // (it shares predict_ctr and eps[SITE_PREDICT] with a call on the acting stream)
  if (e->act_inflight) return e->fail(SACTD3_ESTATE, "predict_device: an acting call is in flight (sactd3_predict_end first)");
  const hipStream_t caller = (hipStream_t)caller_stream;
  EnqCtx x{e, e->stream};      // (the two eager launches around the pair's graph)
  RCCHK(src_order_begin(e, caller, flags));
  RCCHK(launch_obs_pack(x, obs, obs_ld, e->p_x, n));
  if (e->predict_dev_graphs.empty()) e->predict_dev_graphs.assign(2 * (size_t)(e->maxn + 1), nullptr);
  RCCHK(run_graph_slot(e, &e->predict_dev_graphs[(size_t)(explore ? 1 : 0) * (e->maxn + 1) + n], nullptr,
                       [&](EnqCtx& xg) { return enqueue_predict(xg, n, explore, true); }));
  RCCHK(launch_act_unpack(x, actions, actions_ld, n));
  RCCHK(src_order_end(e, caller, flags));
  predict_device_issued(e, n, (flags & SACTD3_SRC_ORDERED) != 0);
  return 0;
}

int sactd3_predict_device_stats(const sactd3_engine* e, int64_t out[4]) { return host_stats(e, &sactd3_engine::pdev_stats, out); }

// ---- scoring caller-supplied state-action pairs: Agent.batched_qf / pi of the reference (agents/agent.py:146-163) as a read path.
// A forward-only pass of the twin critics (online or target arena) on Q_CHUNK rows at a time, eager launches on the learner stream:
// pack -> trunk (pinned launch shape, see TrunkTicks::pin_shape) -> head, which stores straight into the caller's array.  The policy
// form (no actions) first runs the online actor's trunk and its exploit-mode tail into the scoring scratch.  It writes its own
// scratch and its own counters only: no CHAIN_BREAK, no counter tick, actor_dirty untouched, no batch slot / noise buffer / p_* use.
static const int Q_CHUNK = 1024;      // rows per pass: what the scoring scratch is sized for
static int q_scratch(sactd3_engine* e, bool policy) {      // (never zeroed: every float a launch reads was written by the one before it)
  RCCHK(first_use_alloc(e, &e->qs_z1, (size_t)2 * Q_CHUNK * HID, false));
  RCCHK(first_use_alloc(e, &e->qs_z2, (size_t)2 * Q_CHUNK * HID, false));
  RCCHK(first_use_alloc(e, &e->qs_sa, (size_t)Q_CHUNK * e->ldc, false));
  if (!policy) return 0;
  RCCHK(first_use_alloc(e, &e->qs_x, (size_t)Q_CHUNK * e->ldo, false));
  RCCHK(first_use_alloc(e, &e->qs_az1, (size_t)Q_CHUNK * HID, false));
  RCCHK(first_use_alloc(e, &e->qs_az2, (size_t)Q_CHUNK * HID, false));
  return first_use_alloc(e, &e->qs_act, (size_t)Q_CHUNK * e->a4, false);
}
static int launch_sa_pack(EnqCtx& x, const float* obs, int64_t obs_ld, const float* act, int64_t act_ld, int m) {
  const SaFieldArgs g{(float4*)x.e->qs_sa, m, x.e->ldc / 4};
  const long chunks = (long)m * g.c4;
  LAUNCH_ON(k_sa_from_fields, dim3(cpt_blocks(chunks, SA_CPT)), dim3(256), obs, (long)obs_ld, act, (long)act_ld, x.e->o, x.e->a, g);
  return 0;
}
static int launch_q_head(EnqCtx& x, const float* P, int m, float* q, int64_t q_ld, int64_t q_ns) {
  sactd3_engine* e = x.e;
  QHead h{};
  h.z2 = e->qs_z2; h.P = P; h.p_ns = e->Lc.size; h.L = e->Lc; h.n = m; h.ln = e->cfg.layer_norm; h.q = q; h.q_ld = (long)q_ld; h.q_ns = (long)q_ns;
  LAUNCH_ON(k_q_head<4>, dim3((unsigned)((m + 3) / 4), 2), dim3(64), h);
  return 0;
}
static int enqueue_qvalues(EnqCtx& x, const float* obs, int64_t obs_ld, const float* act, int64_t act_ld, int n, int which,
                           float* q, int64_t q_ld, int64_t q_ns) {
  sactd3_engine* e = x.e;
  RCCHK(q_scratch(e, act == nullptr));
  TrunkTicks tk{nullptr, nullptr, nullptr, nullptr, 0.f};
  tk.pin_shape = true;
  const float* P = which == SACTD3_Q_TARGET ? e->Tc : e->Pc;
  for (int64_t row0 = 0; row0 < n; row0 += Q_CHUNK) {
    const int m = (int)std::min<int64_t>(Q_CHUNK, n - row0);
    const float* obs_c = obs + row0 * obs_ld;
    if (!act) {      // pi(s): the online actor's exploit action, what sactd3_predict(explore = 0) returns
      RCCHK(launch_obs_pack(x, obs_c, obs_ld, e->qs_x, m));
      const TrunkGrp ga{e->qs_x, e->Pa, e->qs_az1, e->qs_az2, nullptr, nullptr, nullptr};
      RCCHK(enqueue_trunk(x, e->ldo, e->o, m, e->La, 0, 1, 1, &ga, tk));
      // (exploit mode draws nothing: the tail reads neither the draw buffer nor -- for its result -- the counter, and ticks nothing)
      const ActorTail t = tail_args(e, e->qs_az2, e->Pa, m, e->cfg.prefer_td3_over_sac ? 0 : 1, 0, SACTD3_SITE_PREDICT, 48u, e->qs_act, e->a4, 0, nullptr);
      RCCHK(launch_tail(x, t));
      RCCHK(launch_sa_pack(x, obs_c, obs_ld, e->qs_act, e->a4, m));
    } else RCCHK(launch_sa_pack(x, obs_c, obs_ld, act + row0 * act_ld, act_ld, m));
    const TrunkGrp gc{e->qs_sa, P, e->qs_z1, e->qs_z2, nullptr, nullptr, nullptr};
    RCCHK(enqueue_trunk(x, e->ldc, e->o + e->a, m, e->Lc, e->Lc.size, 1, 2, &gc, tk));
    RCCHK(launch_q_head(x, P, m, q + row0 * q_ld, q_ld, q_ns));
  }
  return 0;
}
static int qvalues_args(sactd3_engine* e, const char* what, int n, int which) {
  if (n < 1) { e->err = std::string(what) + ": n >= 1"; return SACTD3_EINVAL; }
  if (which != SACTD3_Q_ONLINE && which != SACTD3_Q_TARGET) { e->err = std::string(what) + ": `which` is SACTD3_Q_ONLINE or SACTD3_Q_TARGET"; return SACTD3_EINVAL; }
  return 0;
}

int sactd3_qvalues_device(sactd3_engine* e, const float* obs, int64_t obs_ld, const float* actions, int64_t actions_ld, int n, int which,
                          float* q, int64_t q_ld, int64_t q_ns, void* caller_stream, int flags) {
  if (!e) return SACTD3_EINVAL;
  if (!obs || !q) return e->fail(SACTD3_EINVAL, "qvalues_device: null argument");
  USE_DEVICE(e);
  RCCHK(qvalues_args(e, "qvalues_device", n, which));
  if (flags & ~SACTD3_SRC_ORDERED) return e->fail(SACTD3_EINVAL, "qvalues_device: unknown flag");
  if (obs_ld < e->o) return e->fail(SACTD3_EINVAL, "qvalues_device: row stride of `obs` is below its width");
  if (actions && actions_ld < e->a) return e->fail(SACTD3_EINVAL, "qvalues_device: row stride of `actions` is below its width");
  if (q_ld < 1 || q_ns < 1) return e->fail(SACTD3_EINVAL, "qvalues_device: strides of `q` are below its width");
  RCCHK(device_ptr_check(e, obs, "qvalues_device", "obs"));
  if (actions) RCCHK(device_ptr_check(e, actions, "qvalues_device", "actions"));      // (NULL: the policy form)
  RCCHK(device_ptr_check(e, q, "qvalues_device", "q"));
  const hipStream_t caller = (hipStream_t)caller_stream;
  EnqCtx x{e, e->stream};
  RCCHK(src_order_begin(e, caller, flags));
  RCCHK(enqueue_qvalues(x, obs, obs_ld, actions, actions_ld, n, which, q, q_ld, q_ns));
  RCCHK(src_order_end(e, caller, flags));
  ++e->q_stats[0]; e->q_stats[1] += n;
  if (flags & SACTD3_SRC_ORDERED) ++e->q_stats[2];
  if (!actions) ++e->q_stats[3];
  return 0;
}

// the same for host arrays: a chunk at a time through device staging of the engine's own (made at the first call)
int sactd3_qvalues(sactd3_engine* e, const float* obs, const float* actions, int n, int which, float* q) {
  if (!e) return SACTD3_EINVAL;
  if (!obs || !q) return e->fail(SACTD3_EINVAL, "qvalues: null argument");
  USE_DEVICE(e);
  RCCHK(qvalues_args(e, "qvalues", n, which));
  RCCHK(first_use_alloc(e, &e->qs_hq, (size_t)2 * Q_CHUNK, false));
  RCCHK(first_use_alloc(e, &e->qs_hobs, (size_t)Q_CHUNK * e->o, false));
  RCCHK(first_use_alloc(e, &e->qs_hact, (size_t)Q_CHUNK * e->a, false));
  EnqCtx x{e, e->stream};
  for (int64_t row0 = 0; row0 < n; row0 += Q_CHUNK) {
    const int m = (int)std::min<int64_t>(Q_CHUNK, n - row0);
    HIPCHK(hipMemcpy(e->qs_hobs, obs + row0 * e->o, sizeof(float) * (size_t)m * e->o, hipMemcpyHostToDevice));
    if (actions) HIPCHK(hipMemcpy(e->qs_hact, actions + row0 * e->a, sizeof(float) * (size_t)m * e->a, hipMemcpyHostToDevice));
    RCCHK(enqueue_qvalues(x, e->qs_hobs, e->o, actions ? e->qs_hact : nullptr, e->a, m, which, e->qs_hq, 1, Q_CHUNK));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int k = 0; k < 2; ++k)
      HIPCHK(hipMemcpy(q + (int64_t)k * n + row0, e->qs_hq + (size_t)k * Q_CHUNK, sizeof(float) * (size_t)m, hipMemcpyDeviceToHost));
  }
  ++e->q_stats[0]; e->q_stats[1] += n;
  if (!actions) ++e->q_stats[3];
  return 0;
}

int sactd3_qvalues_stats(const sactd3_engine* e, int64_t out[4]) { return host_stats(e, &sactd3_engine::q_stats, out); }

// ---- querying the policy on caller-supplied rows: the actor as a read path (include/sactd3.h; device code: policy_kernels.h).
// Q_CHUNK rows at a time, three eager launches per chunk on the learner stream: pack -> actor trunk (pinned launch shape) -> k_pi_head,
// which stores straight into the caller's arrays; a call that drew natively ends with one k_tick of the feature's own counter.  Like a
// scoring call it writes its own scratch and its own words only: no CHAIN_BREAK, actor_dirty untouched, no batch slot / noise buffer /
// p_* use, no sample / noise / predict counter.
static int pi_scratch(sactd3_engine* e) {
  RCCHK(first_use_alloc(e, &e->pi_x, (size_t)Q_CHUNK * e->ldo));
  RCCHK(first_use_alloc(e, &e->pi_z1, (size_t)Q_CHUNK * HID));
  RCCHK(first_use_alloc(e, &e->pi_z2, (size_t)Q_CHUNK * HID));
  return first_use_alloc(e, &e->pi_ctl, 2);
}
// the head of a (narrow: see tail_rows_per_block) actor, in the form of the acting tail of the same head shape
static int launch_pi_head(EnqCtx& x, const PiHead& h) {
  if (x.e->La.nh <= 8 && x.e->a <= 8) LAUNCH_ON(k_pi_head_s, dim3((unsigned)((h.n + 3) / 4)), dim3(64), h);
  else LAUNCH_ON(k_pi_head, dim3((unsigned)((h.n + 15) / 16)), dim3(256), h);
  return 0;
}
// m rows from row `row0` of the arrays in `io`; `draw_row`: the row of the CALL that one is (it numbers the native draws)
static PiHead pi_head_args(sactd3_engine* e, const float* P, PiCtl* pc, int m, int64_t row0, int64_t draw_row, const sactd3_policy_io& io) {
  PiHead h{};
  h.z2 = e->pi_z2; h.P = P; h.L = e->La; h.n = m; h.a = e->a; h.ln = e->cfg.layer_norm; h.sac = !e->cfg.prefer_td3_over_sac;
  h.draw = (io.sample || io.sample_logp || io.eps_out) ? 1 : 0;
  h.scale = e->scale; h.bias = e->bias; h.ctl = e->ctl; h.pc = pc; h.row0 = (long)draw_row;
  auto at = [&](auto* p, int64_t ld) { return p ? p + row0 * ld : p; };
  h.actions = at(io.actions, io.actions_ld); h.actions_ld = (long)io.actions_ld;
  h.eps = at(io.eps, io.eps_ld); h.eps_ld = (long)io.eps_ld;
  h.mode = at(io.mode, io.mode_ld); h.mode_ld = (long)io.mode_ld;
  h.mean = at(io.mean, io.mean_ld); h.mean_ld = (long)io.mean_ld;
  h.log_std = at(io.log_std, io.log_std_ld); h.log_std_ld = (long)io.log_std_ld;
  h.sample = at(io.sample, io.sample_ld); h.sample_ld = (long)io.sample_ld;
  h.sample_logp = at(io.sample_logp, io.sample_logp_ld); h.sample_logp_ld = (long)io.sample_logp_ld;
  h.action_logp = at(io.action_logp, io.action_logp_ld); h.action_logp_ld = (long)io.action_logp_ld;
  h.eps_out = at(io.eps_out, io.eps_out_ld); h.eps_out_ld = (long)io.eps_out_ld;
  return h;
}
// n rows of `obs` and of every array of `io`; their row 0 is row `first` of the call (the host form hands over a chunk at a time)
static int enqueue_policy(EnqCtx& x, const float* obs, int64_t obs_ld, int64_t first, int n, int which, const sactd3_policy_io& io) {
  sactd3_engine* e = x.e;
  TrunkTicks tk{nullptr, nullptr, nullptr, nullptr, 0.f};
  tk.pin_shape = true;
  const float* P = which == SACTD3_PI_TARGET ? e->Ta : e->Pa;
  for (int64_t r0 = 0; r0 < n; r0 += Q_CHUNK) {
    const int m = (int)std::min<int64_t>(Q_CHUNK, n - r0);
    RCCHK(launch_obs_pack(x, obs + r0 * obs_ld, obs_ld, e->pi_x, m));
    const TrunkGrp ga{e->pi_x, P, e->pi_z1, e->pi_z2, nullptr, nullptr, nullptr};
    RCCHK(enqueue_trunk(x, e->ldo, e->o, m, e->La, 0, 1, 1, &ga, tk));
    RCCHK(launch_pi_head(x, pi_head_args(e, P, e->pi_ctl, m, r0, first + r0, io)));
    e->pi_rows = m;
  }
  return 0;
}
static int pi_tick(EnqCtx& x, const sactd3_policy_io& io) {      // behind the last chunk of a call that drew natively
  if (!(io.sample || io.sample_logp || io.eps_out) || io.eps) return 0;
  return launch_tick(x, &x.e->pi_ctl->policy_ctr);
}
// what both forms refuse, pointers aside
static int policy_args(sactd3_engine* e, const char* what, int n, int which, const sactd3_policy_io& io) {
  auto bad = [&](const char* why) { e->err = std::string(what) + ": " + why; return SACTD3_EINVAL; };
  const bool td3 = e->cfg.prefer_td3_over_sac != 0;
  if (n < 1) return bad("n >= 1");
  if (which != SACTD3_PI_ONLINE && which != SACTD3_PI_TARGET) return bad("`which` is SACTD3_PI_ONLINE or SACTD3_PI_TARGET");
  if (which == SACTD3_PI_TARGET && !td3) return bad("SAC has no target actor (SACTD3_PI_TARGET is TD3 only)");
  if (!(io.mode || io.mean || io.log_std || io.sample || io.sample_logp || io.action_logp || io.eps_out)) return bad("no output is set");
  if (td3 && (io.actions || io.eps || io.mean || io.log_std || io.sample || io.sample_logp || io.action_logp || io.eps_out))
    return bad("TD3 has `mode` only (every other field must be NULL)");
  if (io.action_logp && !io.actions) return bad("`action_logp` needs `actions`");
  if ((io.eps || io.eps_out) && !(io.sample || io.sample_logp)) return bad("`eps` / `eps_out` without `sample` or `sample_logp`");
  return 0;
}

int sactd3_policy_device(sactd3_engine* e, const float* obs, int64_t obs_ld, int n, int which, const sactd3_policy_io* io,
                         void* caller_stream, int flags) {
  if (!e) return SACTD3_EINVAL;
  if (!obs || !io) return e->fail(SACTD3_EINVAL, "policy_device: null argument");
  USE_DEVICE(e);
  RCCHK(policy_args(e, "policy_device", n, which, *io));
  if (flags & ~SACTD3_SRC_ORDERED) return e->fail(SACTD3_EINVAL, "policy_device: unknown flag");
  if (obs_ld < e->o) return e->fail(SACTD3_EINVAL, "policy_device: row stride of `obs` is below its width");
  const FieldRow rows[9] = {
      {io->actions, io->actions_ld, e->a, "actions"}, {io->eps, io->eps_ld, e->a, "eps"}, {io->mode, io->mode_ld, e->a, "mode"},
      {io->mean, io->mean_ld, e->a, "mean"}, {io->log_std, io->log_std_ld, e->a, "log_std"}, {io->sample, io->sample_ld, e->a, "sample"},
      {io->sample_logp, io->sample_logp_ld, 1, "sample_logp"}, {io->action_logp, io->action_logp_ld, 1, "action_logp"},
      {io->eps_out, io->eps_out_ld, e->a, "eps_out"}};
  RCCHK(device_ptr_check(e, obs, "policy_device", "obs"));
  RCCHK(field_rows_check(e, rows, 9, false, "policy_device", nullptr));      // (policy_args has refused "no output is set")
  RCCHK(pi_scratch(e));
  const hipStream_t caller = (hipStream_t)caller_stream;
  EnqCtx x{e, e->stream};
  RCCHK(src_order_begin(e, caller, flags));
  RCCHK(enqueue_policy(x, obs, obs_ld, 0, n, which, *io));
  RCCHK(pi_tick(x, *io));
  RCCHK(src_order_end(e, caller, flags));
  ++e->pi_stats[0]; e->pi_stats[1] += n;
  return 0;
}

// the same for host arrays: a chunk at a time through device staging of the engine's own (made at the first call); the chunk's rows keep
// their row numbers of the call, so the native draws are those of the device call
int sactd3_policy(sactd3_engine* e, const float* obs, int n, int which, const sactd3_policy_io* hio) {
  if (!e) return SACTD3_EINVAL;
  if (!obs || !hio) return e->fail(SACTD3_EINVAL, "policy: null argument");
  USE_DEVICE(e);
  RCCHK(policy_args(e, "policy", n, which, *hio));
  RCCHK(pi_scratch(e));
  const int a = e->a;
  RCCHK(first_use_alloc(e, &e->pi_hobs, (size_t)Q_CHUNK * e->o, false));
  RCCHK(first_use_alloc(e, &e->pi_hio, (size_t)Q_CHUNK * (7 * a + 2), false));
  EnqCtx x{e, e->stream};
  // device staging of one chunk: [actions | eps | mode | mean | log_std | sample | eps_out] each [Q_CHUNK, a], then the two [Q_CHUNK] columns
  float* const base = e->pi_hio;
  auto slab = [&](int k) { return base + (size_t)k * Q_CHUNK * a; };
  float* const lp_s = slab(7), * const lp_a = slab(7) + Q_CHUNK;
  for (int64_t row0 = 0; row0 < n; row0 += Q_CHUNK) {
    const int m = (int)std::min<int64_t>(Q_CHUNK, n - row0);
    const size_t wide = sizeof(float) * (size_t)m * a;
    HIPCHK(hipMemcpy(e->pi_hobs, obs + row0 * e->o, sizeof(float) * (size_t)m * e->o, hipMemcpyHostToDevice));
    if (hio->actions) HIPCHK(hipMemcpy(slab(0), hio->actions + row0 * a, wide, hipMemcpyHostToDevice));
    if (hio->eps) HIPCHK(hipMemcpy(slab(1), hio->eps + row0 * a, wide, hipMemcpyHostToDevice));
    sactd3_policy_io d{};      // the chunk's staging, for the fields the caller gave / wants
    auto staged = [](float* p, const void* wanted) -> float* { return wanted ? p : nullptr; };
    d.actions = staged(slab(0), hio->actions); d.eps = staged(slab(1), hio->eps);
    d.mode = staged(slab(2), hio->mode); d.mean = staged(slab(3), hio->mean);
    d.log_std = staged(slab(4), hio->log_std); d.sample = staged(slab(5), hio->sample);
    d.eps_out = staged(slab(6), hio->eps_out);
    d.sample_logp = staged(lp_s, hio->sample_logp); d.action_logp = staged(lp_a, hio->action_logp);
    d.actions_ld = d.eps_ld = d.mode_ld = d.mean_ld = d.log_std_ld = d.sample_ld = d.eps_out_ld = a;
    d.sample_logp_ld = d.action_logp_ld = 1;
    RCCHK(enqueue_policy(x, e->pi_hobs, e->o, row0, m, which, d));
    if (row0 + m >= n) RCCHK(pi_tick(x, *hio));
    HIPCHK(hipStreamSynchronize(e->stream));
    auto back = [&](float* dst, const float* src, int width) -> hipError_t {
      return dst ? hipMemcpy(dst + row0 * width, src, sizeof(float) * (size_t)m * width, hipMemcpyDeviceToHost) : hipSuccess;
    };
    HIPCHK(back(hio->mode, slab(2), a)); HIPCHK(back(hio->mean, slab(3), a)); HIPCHK(back(hio->log_std, slab(4), a));
    HIPCHK(back(hio->sample, slab(5), a)); HIPCHK(back(hio->eps_out, slab(6), a));
    HIPCHK(back(hio->sample_logp, lp_s, 1)); HIPCHK(back(hio->action_logp, lp_a, 1));
  }
  ++e->pi_stats[0]; e->pi_stats[1] += n;
  return 0;
}

int sactd3_policy_stats(sactd3_engine* e, int64_t out[4]) {      // (PiCtl::clamped and ::nan_rows are adjacent)
  return (!e || !out) ? SACTD3_EINVAL : stats_with_words(e, e->pi_stats, e->pi_ctl ? &e->pi_ctl->clamped : nullptr, 2, 2, out);
}

int sactd3_acting_stats(const sactd3_engine* e, int64_t out[4]) { return host_stats(e, &sactd3_engine::act_stats, out); }

int sactd3_read_metrics(sactd3_engine* e, float out[SACTD3_NUM_METRICS]) {
  if (!e || !out) return SACTD3_EINVAL;
  USE_DEVICE(e);
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(out, e->ctl->metrics, sizeof(float) * SACTD3_NUM_METRICS, hipMemcpyDeviceToHost));
  return 0;
}

// TD3+BC: republish (bc_alpha, bc_weight) -- DevCtl::bc, two adjacent words -- with one single-thread launch on the learner stream, as
// `beta` of the prioritised draw is.  The kernels read the words there, no graph holds a value, and nothing that ran ahead (the opening
// pair of the next period: a next-action pass and a policy pass) depends on them: no CHAIN_BREAK, no capture.
int sactd3_set_bc(sactd3_engine* e, float bc_alpha, float bc_weight) {
  if (!e) return SACTD3_EINVAL;
  USE_DEVICE(e);
  if (!e->bc_on) return e->fail(SACTD3_ESTATE, "set_bc: the engine was created with bc_alpha == 0 (the kernel forms are chosen at create)");
  if (!(bc_alpha > 0.f) || !std::isfinite(bc_alpha)) return e->fail(SACTD3_EINVAL, "set_bc: bc_alpha must be finite and > 0");
  if (!(bc_weight >= 0.f) || !std::isfinite(bc_weight)) return e->fail(SACTD3_EINVAL, "set_bc: bc_weight must be finite and >= 0");
  int bits[2];
  memcpy(&bits[0], &bc_alpha, sizeof(int)); memcpy(&bits[1], &bc_weight, sizeof(int));
  EnqCtx x{e, e->stream};
  RCCHK(launch_set_int2(x, reinterpret_cast<int*>(e->ctl->bc), bits[0], bits[1]));
  e->bc_alpha = bc_alpha; e->bc_weight = bc_weight;
  return 0;
}

int sactd3_get_bc(sactd3_engine* e, float out[2]) {
  if (!e || !out) return SACTD3_EINVAL;
  USE_DEVICE(e);
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(out, e->ctl->bc, sizeof(float) * 2, hipMemcpyDeviceToHost));
  return 0;
}

int sactd3_device_handles(sactd3_engine* e, void** stream, float** metrics) {
  if (!e) return SACTD3_EINVAL;
  if (stream) *stream = (void*)e->stream;
  if (metrics) *metrics = e->ctl->metrics;
  return 0;
}

// Wait for the engine's stream: poll it for up to 2 ms (a blocking hipStreamSynchronize sleeps on an interrupt and wakes up tens of
// microseconds after the last kernel has finished -- as long as an iteration takes), then block.
static int stream_wait(sactd3_engine* e) {
  const auto t0 = std::chrono::steady_clock::now();
  for (int spins = 0;; ++spins) {
    const hipError_t q = hipStreamQuery(e->stream);
    if (q == hipSuccess) return 0;
    if (q != hipErrorNotReady) return e->fail(SACTD3_EHIP, "hipStreamQuery", q);
    if ((spins & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

int sactd3_sync(sactd3_engine* e) {
  if (!e) return SACTD3_EINVAL;
  USE_DEVICE(e);
  RCCHK(stream_wait(e));
  if (e->act_stream) HIPCHK(hipStreamSynchronize(e->act_stream));      // (a begun call stays begun: sactd3_predict_end still collects it)
  return 0;
}

// ---- introspection
// THE list of what sactd3_debug_read hands out, in the order sactd3_debug_names spells it.  A name carries its kind -- a plain buffer, a
// gradient arena (read in the reference's unpadded layout), a word of the priority table (refused until sactd3_prio_enable), the policy
// query's last chunk (refused until a query has run) -- and `stale`: the grads_stale family it belongs to, or -1.  dbg_table(e) is that
// list for an engine; on an engine that holds nothing it still names everything, which is what sactd3_debug_names reads.
enum { DBG_PLAIN, DBG_GRAD, DBG_PRIO, DBG_PI_Z2 };
struct DbgEntry { const char* name; const float* ptr; int64_t n; int kind = DBG_PLAIN; int stale = -1; };
static std::vector<DbgEntry> dbg_table(const sactd3_engine* e) {
  const int64_t B = e->B, BH = B * HID;
  const sactd3_engine::BatchSlot& S = e->bs[e->slot.cur];
  return {
      {"X", S.X, B * e->ldc}, {"Xn", S.Xn, B * e->ldc}, {"Xp", e->Xp, B * e->ldc}, {"rew", S.rew, B}, {"done", S.done, B},
      {"logp_next", S.logp_n, B}, {"logp_pi", e->logp_pi, B}, {"logp_alpha", e->logp_al, B},
      {"a_xh1", e->a_xh1, BH}, {"a_h1", e->a_h1, BH}, {"a_z2", e->a_z2, BH}, {"a_h2", e->a_h2, BH},
      {"a_xh2", e->a_xh2, BH}, {"a_rs2", e->a_rs2, B}, {"a_tg", e->a_tg, B * 4 * e->a4}, {"a_du", e->a_du, B * e->ldu},
      {"a_dz2", e->a_dz2, BH}, {"a_dh1", e->a_dh1, BH}, {"a_dz1", e->a_dz1, BH, DBG_PLAIN, 1},
      {"c_xh1", e->c_xh1, 2 * BH}, {"c_h1", e->c_h1, 2 * BH}, {"c_z2", e->c_z2, 2 * BH}, {"c_dz2", e->c_dz2, 2 * BH},
      {"c_dh1", e->c_dh1, 2 * BH}, {"c_dz1", e->c_dz1, 2 * BH, DBG_PLAIN, 0}, {"t_z2", e->t_z2, 2 * BH},
      {"q", e->q, 2 * B}, {"q_target", e->qt, 2 * B}, {"targ_q", e->y, B}, {"q_pi", e->q_pi, 2 * B}, {"dA", e->dA, 2 * B * e->a4},
      {"grad_actor", e->Ga, ref_count(e->La, e->cfg.layer_norm), DBG_GRAD, 1},
      {"grad_critics", e->Gc, 2 * ref_count(e->Lc, e->cfg.layer_norm), DBG_GRAD, 0},
      {"prio_leaf", e->pt_leaf, e->cfg.rb_capacity, DBG_PRIO}, {"prio_sums", e->pt_sums, e->pt_groups, DBG_PRIO},      // (the one level above the leaves)
      {"prio_max", e->pt_ctl ? &e->pt_ctl->max_prio : nullptr, 1, DBG_PRIO},
      {"prio_weights", e->bs[0].w, B, DBG_PRIO},      // (the loss weights batch slot 0 carries)
      {"pi_z2", e->pi_z2, (int64_t)e->pi_rows * HID, DBG_PI_Z2},      // the last chunk of the last policy query
  };
}
const char* sactd3_debug_names(void) {
  static const std::string names = [] {
    const sactd3_engine none;
    std::string s;
    for (const DbgEntry& d : dbg_table(&none)) s += (s.empty() ? "" : " ") + std::string(d.name);
    return s;
  }();
  return names.c_str();
}
int64_t sactd3_debug_read(sactd3_engine* e, const char* name, float* dst, int64_t max_floats) {
  if (!e || !name) return SACTD3_EINVAL;
  USE_DEVICE(e);
  for (const DbgEntry& d : dbg_table(e)) {
    if (strcmp(d.name, name)) continue;
    if (d.stale >= 0 && e->grads_stale[d.stale])
      return e->fail(SACTD3_ESTATE, "debug_read: period graphs do not store this buffer; run an API-path update or sactd3_step first");
    if (d.kind == DBG_PRIO && !e->pt_on) return e->fail(SACTD3_ESTATE, "debug_read: priorities are not enabled");
    if (d.kind == DBG_PI_Z2 && !e->pi_rows) return e->fail(SACTD3_ESTATE, "debug_read: no policy query has run (sactd3_policy_device first)");
    if (!dst) return d.n;
    if (max_floats < d.n) return e->fail(SACTD3_EINVAL, "debug_read: buffer too small");
    if (d.kind == DBG_GRAD) { RCCHK(read_arena(e, d.ptr, d.stale ? e->La : e->Lc, d.stale ? 1 : 2, dst)); return d.n; }
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(dst, d.ptr, sizeof(float) * d.n, hipMemcpyDeviceToHost));
    return d.n;
  }
  return e->fail(SACTD3_EINVAL, "debug_read: unknown buffer name");
}

int sactd3_graph_kernel_count(sactd3_engine* e, int which_graph) {
  if (!e) return SACTD3_EINVAL;
  static const int map[9] = {G_Q, G_A, G_STEP01, G_STEP11, G_PERIOD, G_OPENING, G_PREFIX, G_PREFIX + 2, G_QW};
  // 16 + 2 do_actor + target update: the graphs of sactd3_step_sampled for its current (draw, n_step, stride); 0: not captured
  if (which_graph >= 16 && which_graph < 20) return e->graph_nodes[G_SAMPLED + which_graph - 16];
  if (which_graph == 10) return e->graph_nodes[e->graphs[G_RUN] ? G_RUN : G_RUN + 1];      // the run graph of sactd3_step_periods; 0: not captured
  if (which_graph < 0 || which_graph > 8) return SACTD3_EINVAL;
  int w = map[which_graph];
  if (!e->graphs[w] && (which_graph == 2 || which_graph == 3)) w -= 1;   // the no-Polyak variant, if that is the one in use
  return e->graph_nodes[w];
}

// sactd3_time_kernel("rows_to_fields"): the current slot's idx widened to int64 in a device array of the engine's own (made at the
// first use), folded into [0, rb_len) so that a slot filled by sactd3_load_batch on a short ring does not count as refused rows
static int time_rows_indices(sactd3_engine* e) {
  if (e->rb_len <= 0) return e->fail(SACTD3_ESTATE, "time_kernel: buffer is empty");
  RCCHK(first_use_alloc(e, &e->time_idx, (size_t)e->B));
  std::vector<int> h(e->B);
  std::vector<long long> w(e->B);
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(h.data(), e->bs[e->slot.cur].idx, sizeof(int) * h.size(), hipMemcpyDeviceToHost));
  for (int b = 0; b < e->B; ++b) w[b] = (long long)((h[b] < 0 ? 0 : h[b]) % e->rb_len);
  HIPCHK(hipMemcpy(e->time_idx, w.data(), sizeof(long long) * w.size(), hipMemcpyHostToDevice));
  return 0;
}

// ---- sactd3_time_kernel: the bodies, one launch sequence each, and the table that names them
// (slot_refilled: only where the kernel being timed overwrites batch slot 0)
static int time_gather(EnqCtx& x) {   // a fresh index draw per launch (k_tick bumps the sample counter): rows come from HBM, not from the caches
  slot_refilled(x.e, false, false);
  RCCHK(enqueue_gather(x, x.e->ring, -1));
  return launch_tick(x, &x.e->ctl->sample_ctr);
}
static int time_polyak(EnqCtx& x) { return enqueue_polyak(x, POLYAK_CRITICS | (x.e->cfg.prefer_td3_over_sac ? POLYAK_ACTOR : 0)); }
static int time_trunk_critics(EnqCtx& x) {   // the 4-net hidden-layer launch of update_qnets (no state is modified)
  sactd3_engine* e = x.e;
  const TrunkGrp g[2] = {{e->Xn, e->Tc, e->t_z1, e->t_z2, nullptr, nullptr, nullptr},
                         {e->X, e->Pc, e->c_z1, e->c_z2, e->c_xh1, e->c_h1, e->c_rs1}};
  return enqueue_trunk(x, e->ldc, e->o + e->a, e->B, e->Lc, e->Lc.size, 2, 2, g, TrunkTicks{nullptr, nullptr, nullptr, nullptr, 0.f});
}
// the engine's own staging slab as six strided fields, one record per row: [s | a] [s'] [r] [d, as the float's first byte] and the index
// in the two pad floats behind [r, d], which are 8-byte aligned
static sactd3_device_fields_out slab_fields(const sactd3_engine* e) {
  sactd3_device_fields_out f{};
  f.obs = e->stage_dev; f.actions = e->stage_dev + e->o; f.next_obs = e->stage_dev + e->ldc; f.rewards = e->stage_dev + e->ldc + e->ldo;
  f.dones = (uint8_t*)(e->stage_dev + e->ldc + e->ldo + 1);
  f.obs_ld = f.actions_ld = f.next_obs_ld = f.rewards_ld = e->rec_f; f.dones_ld = 4 * (int64_t)e->rec_f;
  f.index = (int64_t*)(e->stage_dev + e->ldc + e->ldo + 2); f.index_ld = e->rec_f / 2;
  return f;
}
// the device-boundary pack kernels, fed from the slab read as five strided fields (batch_size rows into the batch slot / an env step's
// max_envs rows into the ring: both are overwritten)
static FieldSrc slab_src(const sactd3_engine* e) {
  const sactd3_device_fields_out o = slab_fields(e);
  const sactd3_device_fields f{o.obs, o.obs_ld, o.actions, o.actions_ld, o.rewards, o.rewards_ld, o.next_obs, o.next_obs_ld, o.dones, o.dones_ld};
  return field_src(e, &f, 0);
}
static int time_batch_from_fields(EnqCtx& x) { slot_refilled(x.e, false, false); return launch_batch_fields(x, slab_src(x.e)); }
static int time_rb_ingest_fields(EnqCtx& x) {
  return launch_ingest_fields(x, slab_src(x.e), (int)std::min<int64_t>(std::min(x.e->maxn, x.e->B), ring_region(x.e)));
}
// the pack / unpack kernels of sactd3_predict_device on max_envs rows: observations read from the ring's records (the s columns,
// row stride = the record), actions written to the acting scratch p_z1 (row stride = its 256 columns; the next trunk overwrites it)
static int time_obs_from_field(EnqCtx& x) {
  return launch_obs_pack(x, x.e->ring, x.e->rec_f, x.e->p_x, (int)std::min<int64_t>(x.e->maxn, x.e->cfg.rb_capacity));
}
static int time_act_to_field(EnqCtx& x) { return launch_act_unpack(x, x.e->p_z1, HID, x.e->maxn); }
// the read-out kernels on batch_size rows, written into the slab as six strided fields (the mirror image of the pack kernels' sources);
// the rows kernel takes its indices from time_idx (the current slot's idx, widened: prepared before anything is timed)
static FieldDst slab_dst(const sactd3_engine* e) { const sactd3_device_fields_out f = slab_fields(e); return field_dst(e, &f, 0); }
static int time_batch_to_fields(EnqCtx& x) { return launch_batch_out(x, slab_dst(x.e)); }
static int time_rows_to_fields(EnqCtx& x) { return launch_rows_out(x, slab_dst(x.e), x.e->time_idx, 1, x.e->B, (int)x.e->rb_len); }
// the pack / head kernels of sactd3_qvalues_device on Q_CHUNK rows of the scoring scratch: [s | a] read from the ring's records (row
// stride = the record); the head on whatever the scratch's z2 holds, its values written over the scratch's z1
static int time_q_kernels(EnqCtx& x, bool head) {
  sactd3_engine* e = x.e;
  RCCHK(q_scratch(e, false));
  const int m = (int)std::min<int64_t>(Q_CHUNK, e->cfg.rb_capacity);
  return head ? launch_q_head(x, e->Pc, m, e->qs_z1, 1, Q_CHUNK) : launch_sa_pack(x, e->ring, e->rec_f, e->ring + e->o, e->rec_f, m);
}
// the head kernel of sactd3_policy_device alone on Q_CHUNK rows of its scratch: whatever z2 holds (zeros before the first call), the
// given actions zeros, native draws, every output into a scratch of this timing's own; its row counters are a second PiCtl's
static int time_pi_head(EnqCtx& x) {
  sactd3_engine* e = x.e;
  RCCHK(pi_scratch(e));
  const int a = e->a;
  RCCHK(first_use_alloc(e, &e->pi_time, (size_t)Q_CHUNK * (6 * a + 2)));
  auto slab = [&](int k) { return e->pi_time + (size_t)k * Q_CHUNK * a; };
  sactd3_policy_io io{};
  io.mode = slab(1); io.mode_ld = a;
  if (!e->cfg.prefer_td3_over_sac) {
    io.actions = slab(0); io.mean = slab(2); io.log_std = slab(3); io.sample = slab(4); io.eps_out = slab(5);
    io.sample_logp = slab(6); io.action_logp = slab(6) + Q_CHUNK;
    io.actions_ld = io.mean_ld = io.log_std_ld = io.sample_ld = io.eps_out_ld = a; io.sample_logp_ld = io.action_logp_ld = 1;
  }
  return launch_pi_head(x, pi_head_args(e, e->Pa, e->pi_ctl + 1, Q_CHUNK, 0, 0, io));
}
// the TD read-out kernel: the TD errors of whatever e->q / e->y hold, written into the engine's own staging slab
static int time_td_to_field(EnqCtx& x) { return launch_td_out(x, x.e->stage_dev, 1, x.e->B); }
// the draw kernel of sactd3_rb_sample_mixed alone (call form, the current P and m; the sample counter advances, the slot stays)
static int time_mix_draw(EnqCtx& x) {
  if (const char* why = mix_refusal(x.e)) { x.e->err = std::string("time_kernel: ") + why; return SACTD3_ESTATE; }
  RCCHK(mix_alloc(x.e));
  return launch_mix_draw(x, x.e->rb_pinned, x.e->mix_m);
}
// the engine-owned priorities (SACTD3_ESTATE before sactd3_prio_enable)
static int time_prio_refusal(sactd3_engine* e) {
  if (!e->pt_on) return e->fail(SACTD3_ESTATE, "time_kernel: priorities are not enabled");
  if (e->rb_len <= 0) return e->fail(SACTD3_ESTATE, "time_kernel: buffer is empty");
  return 0;
}
// "prio_update": the write-back kernel on batch_size rows, indices as for "rows_to_fields", every priority 1 (those rows' priorities ARE overwritten)
static int time_prio_update(EnqCtx& x) {
  sactd3_engine* e = x.e;
  RCCHK(time_prio_refusal(e));
  if (!e->pt_ones) {
    RCCHK(first_use_alloc(e, &e->pt_ones, (size_t)e->B, false));
    const std::vector<float> one((size_t)e->B, 1.f);
    HIPCHK(hipMemcpy(e->pt_ones, one.data(), sizeof(float) * one.size(), hipMemcpyHostToDevice));
  }
  PrioUpdateArgs g{};
  g.n = e->B; g.idx = e->time_idx; g.idx_ld = 1; g.prio = e->pt_ones; g.prio_ld = 1;
  return launch_prio_update(x, g);
}
// the staging calls, batch slot 0 overwritten: stage_ring_rows itself, without its counters.  "batch_from_index" / "_nstep" (steps 3,
// stride 1): the one staging kernel on batch_size rows, indices from time_idx (as "rows_to_fields"), no weights; "prio_sample": one
// whole sactd3_rb_sample_prioritized (beta 0.4: three launches, the draw counter advanced)
static int time_stage(EnqCtx& x, bool prio_sample, bool chain) {
  StageReq q{"time_kernel"};
  q.internal = true;
  if (prio_sample) { RCCHK(time_prio_refusal(x.e)); q.kind = SACTD3_DRAW_PRIORITIZED; q.beta = 0.4f; }
  else { q.callers = true; q.rows.idx = x.e->time_idx; q.n = x.e->B; }
  if (chain) { q.chain = true; q.steps = 3; q.stride = 1; }
  return stage_ring_rows(x, q);
}
// needs_row_indices: time_rows_indices runs once in front of the warm-up
struct TimedKernel { const char* name; bool needs_row_indices; int (*body)(EnqCtx&); };
static const TimedKernel TIMED_KERNELS[] = {
    {"gather", false, time_gather}, {"polyak", false, time_polyak}, {"trunk_critics", false, time_trunk_critics},
    {"batch_from_fields", false, time_batch_from_fields}, {"rb_ingest_fields", false, time_rb_ingest_fields},
    {"obs_from_field", false, time_obs_from_field}, {"act_to_field", false, time_act_to_field},
    {"batch_to_fields", false, time_batch_to_fields}, {"rows_to_fields", true, time_rows_to_fields},
    {"sa_from_fields", false, [](EnqCtx& x) { return time_q_kernels(x, false); }}, {"q_head", false, [](EnqCtx& x) { return time_q_kernels(x, true); }},
    {"batch_from_index", true, [](EnqCtx& x) { return time_stage(x, false, false); }}, {"td_to_field", false, time_td_to_field},
    {"prio_sample", false, [](EnqCtx& x) { return time_stage(x, true, false); }}, {"prio_update", true, time_prio_update},
    {"batch_from_index_nstep", true, [](EnqCtx& x) { return time_stage(x, false, true); }}, {"mix_draw", false, time_mix_draw},
    {"pi_head", false, time_pi_head},
};

int sactd3_time_kernel(sactd3_engine* e, const char* kernel, int iters, float* usec) {
  if (!e || !kernel || !usec || iters < 1) return SACTD3_EINVAL;
  USE_DEVICE(e);
  CHAIN_BREAK(e);
  const TimedKernel* k = std::find_if(std::begin(TIMED_KERNELS), std::end(TIMED_KERNELS), [&](const TimedKernel& t) { return !strcmp(t.name, kernel); });
  if (k == std::end(TIMED_KERNELS)) {
    std::string names;
    for (const TimedKernel& t : TIMED_KERNELS) names += (names.empty() ? "" : " | ") + std::string(t.name);
    return e->fail(SACTD3_EINVAL, ("time_kernel: unknown kernel (" + names + ")").c_str());
  }
  hipEvent_t t0, t1;
  HIPCHK(hipEventCreate(&t0)); HIPCHK(hipEventCreate(&t1));
  EnqCtx x{e, e->stream};
  int rc = k->needs_row_indices ? time_rows_indices(e) : 0;
  for (int i = 0; i < 3 && rc == 0; ++i) rc = k->body(x);   // warm-up
  if (rc == 0) {
    hipEventRecord(t0, e->stream);
    for (int i = 0; i < iters && rc == 0; ++i) rc = k->body(x);
    hipEventRecord(t1, e->stream);
    hipEventSynchronize(t1);
    float ms = 0.f;
    hipEventElapsedTime(&ms, t0, t1);
    *usec = ms * 1000.f / (float)iters;
  }
  hipEventDestroy(t0); hipEventDestroy(t1);
  return rc;
}

// Per-node device time of one fused iteration.  The enqueue sequence of sactd3_step(do_actor) is walked once to list
// its kernel launches (node registry), then each launch alone is issued `iters` times back to back between two HIP
// events on the engine's stream (the other launches of the sequence are skipped).  The learner's state is consumed by
// this (optimiser steps repeat on stale gradients): use a scratch engine.
int sactd3_time_nodes(sactd3_engine* e, int do_actor, int iters, int max_nodes, char* names, int names_cap,
                      float* usec, double* flops, double* bytes, int64_t* threads) {
  if (!e || iters < 1 || max_nodes < 1 || !usec) return SACTD3_EINVAL;
  USE_DEVICE(e);
  CHAIN_BREAK(e);
  if (e->rb_len <= 0) return e->fail(SACTD3_ESTATE, "time_nodes: buffer is empty");
  slot_refilled(e, false, false);
  const bool act = do_actor != 0 && e->cfg.actor_update_delay > 0;
  const bool period = do_actor == 2 && e->cfg.actor_update_delay > 0 && same_target_branch(e);
  if (act || period) RCCHK(actor_write_begin(e));
  if (period) mark_grads_stale(e);
  std::vector<NodeInfo> log;
  auto seq = [&](int only, std::vector<NodeInfo>* into = nullptr) -> int {      // the sequence with launch `only` alone issued (-1: all of them)
    EnqCtx x{e, e->stream};
    x.node_only = only; x.node_log = into;
    return enqueue_end(x, enqueue_graph(x, period ? G_PERIOD : act ? G_STEP11 : G_STEP01));
  };
  int rc = seq(1 << 30, &log);               // list only, launch nothing
  if (rc != 0) return rc;
  const int n = (int)log.size();
  if (n > max_nodes) return e->fail(SACTD3_EINVAL, "time_nodes: max_nodes too small");
  std::string joined;
  for (int k = 0; k < n; ++k) { joined += log[k].name; joined += '\n'; }
  if (names) {
    if ((int)joined.size() + 1 > names_cap) return e->fail(SACTD3_EINVAL, "time_nodes: names buffer too small");
    memcpy(names, joined.c_str(), joined.size() + 1);
  }
  hipEvent_t t0, t1;
  HIPCHK(hipEventCreate(&t0)); HIPCHK(hipEventCreate(&t1));
  // clocks up before anything is timed (an engine is usually created just before this call: the GPU has been idle), then
  // every node in 3 batches of `iters` launches, the fastest batch counting (a batch hit by a clock ramp or by another
  // process's work on the card would otherwise show up as a 100x outlier)
  for (int i = 0; i < 60 && rc == 0; ++i) rc = seq(-1);
  for (int k = 0; k < n && rc == 0; ++k) {
    for (int i = 0; i < 3 && rc == 0; ++i) rc = seq(k);
    float best = 0.f;
    for (int rep = 0; rep < 3 && rc == 0; ++rep) {
      hipEventRecord(t0, e->stream);
      for (int i = 0; i < iters && rc == 0; ++i) rc = seq(k);
      hipEventRecord(t1, e->stream);
      if (hipEventSynchronize(t1) != hipSuccess) rc = e->fail(SACTD3_EHIP, "time_nodes: hipEventSynchronize");
      float ms = 0.f;
      hipEventElapsedTime(&ms, t0, t1);
      if (rep == 0 || ms < best) best = ms;
    }
    usec[k] = best * 1000.f / (float)iters;
    if (flops) flops[k] = log[k].flops;
    if (bytes) bytes[k] = log[k].bytes;
    if (threads) threads[k] = log[k].threads;
  }
  hipEventDestroy(t0); hipEventDestroy(t1);
  return rc == 0 ? n : rc;
}

int sactd3_time_gather_sweep(sactd3_engine* e, int batch, int iters, float* usec, double* algo_bytes) {
  if (!e || !usec || batch < 1 || iters < 1) return SACTD3_EINVAL;
  USE_DEVICE(e);
  CHAIN_BREAK(e);
  if (e->rb_len <= 0) return e->fail(SACTD3_ESTATE, "gather sweep: buffer is empty");
  if ((long long)batch * e->rec4 >= (1ll << 31)) return e->fail(SACTD3_EINVAL, "gather sweep: batch too large");
  float *X = nullptr, *Xn = nullptr, *rw = nullptr, *dn = nullptr; int* ix = nullptr;
  const size_t rows = batch;
  hipError_t he = hipSuccess;
  auto A = [&](void** p, size_t bytes) { if (he == hipSuccess) he = hipMalloc(p, bytes); };
  A((void**)&X, rows * e->ldc * 4); A((void**)&Xn, rows * e->ldc * 4);
  A((void**)&rw, rows * 4); A((void**)&dn, rows * 4); A((void**)&ix, rows * 4);
  int rc = 0;
  if (he != hipSuccess) rc = e->fail(SACTD3_EHIP, "gather sweep: hipMalloc", he);
  if (rc == 0) {
    GatherArgs g{};
    g.ring = (const float4*)e->ring; g.rec4 = e->rec4; g.cx = e->cx; g.cn = e->cn; g.ctl = e->ctl; g.idx = ix;
    g.X = (float4*)X; g.Xn = (float4*)Xn; g.rew = rw; g.done = dn; g.B = batch; g.len_override = -1;
    g.rec4_magic = magic_div((unsigned)e->rec4, (unsigned long long)batch * e->rec4 + 1);
    const dim3 grid(gather_blocks((long)batch * e->rec4));
    g.cpb = (int)(((long)batch * e->rec4 + 256L * grid.x - 1) / (256L * grid.x));
    hipEvent_t t0, t1;
    hipEventCreate(&t0); hipEventCreate(&t1);
    EnqCtx x{e, e->stream};
    const auto gather = [&](bool tick) -> int {
      LAUNCH_ON(k_gather, grid, dim3(256), g);
      return tick ? launch_tick(x, &e->ctl->sample_ctr) : 0;
    };
    for (int i = 0; i < 2 && rc == 0; ++i) rc = gather(false);
    hipEventRecord(t0, e->stream);
    for (int i = 0; i < iters && rc == 0; ++i) rc = gather(true);
    hipEventRecord(t1, e->stream);
    he = hipEventSynchronize(t1);
    float ms = 0.f;
    hipEventElapsedTime(&ms, t0, t1);
    *usec = ms * 1000.f / (float)iters;
    hipEventDestroy(t0); hipEventDestroy(t1);
    if (rc == 0 && he != hipSuccess) rc = e->fail(SACTD3_EHIP, "gather sweep", he);
    // 2*B*T + 4*B with T = 4*(2o+a+1)+1 bytes
    if (algo_bytes) *algo_bytes = 2.0 * batch * (4.0 * (2 * e->o + e->a + 1) + 1.0) + 4.0 * batch;
  }
  hipFree(X); hipFree(Xn); hipFree(rw); hipFree(dn); hipFree(ix);
  return rc;
}

// ---- initialise / reset the networks on the device (include/sactd3_init.h)
// the weight matrices of `what`, each with its id and its fixed place in the scratch buffer (whatever else the call holds); -> floats of
// scratch all nine need
static long init_mats(sactd3_engine* e, uint32_t what, InitMat* out, int* count) {
  long off = 0; int n = 0;
  for (int net = 0; net < 3; ++net) {      // 0: the actor; 1, 2: the critics
    const NetLayout& L = net ? e->Lc : e->La;
    float* P = net ? e->Pc + (size_t)(net - 1) * L.size : e->Pa;
    const int woff[3] = {L.W1, L.W2, L.Wh}, ld[3] = {L.ld1, HID, HID}, rows[3] = {HID, HID, L.nh}, cols[3] = {L.K, HID, HID};
    for (int l = 0; l < 3; ++l) {
      if (what & (net ? SACTD3_INIT_CRITICS : SACTD3_INIT_ACTOR)) out[n++] = InitMat{P + woff[l], ld[l], rows[l], cols[l], 3 * net + l, off};
      off += (long)rows[l] * cols[l];
    }
  }
  *count = n;
  return off;
}
static InitFanFam init_family(sactd3_engine* e, bool actor) {
  const NetLayout& L = actor ? e->La : e->Lc;
  InitFanFam f{};
  f.P = actor ? e->Pa : e->Pc; f.T = actor ? e->Ta : e->Tc; f.T2 = actor ? e->Ta2 : nullptr; f.T3 = actor ? e->Ta3 : nullptr;
  f.M = actor ? e->Ma : e->Mc; f.V = actor ? e->Va : e->Vc; f.nets = actor ? 1 : 2;
  f.size = L.size; f.b1 = L.b1; f.g1 = L.g1; f.W2 = L.W2; f.b2 = L.b2; f.g2 = L.g2; f.Wh = L.Wh; f.bh = L.bh;
  f.t = actor ? &e->ctl->t_a : &e->ctl->t_q; f.pw = actor ? e->ctl->pw_a : e->ctl->pw_q;
  return f;
}

int sactd3_init_params(sactd3_engine* e, uint32_t what, uint64_t seed, uint32_t epoch) {
  if (!e) return SACTD3_EINVAL;
  // refusals first: a refused call has launched, allocated, counted and marked nothing
  const uint32_t known = SACTD3_INIT_ACTOR | SACTD3_INIT_CRITICS | SACTD3_INIT_ALPHA;
  if (what == 0 || (what & ~known)) return e->fail(SACTD3_EINVAL, "init_params: `what` is a non-empty sum of SACTD3_INIT_ACTOR, _CRITICS, _ALPHA");
  if ((what & SACTD3_INIT_ALPHA) && e->cfg.prefer_td3_over_sac) return e->fail(SACTD3_EINVAL, "init_params: a TD3 engine has no temperature (SACTD3_INIT_ALPHA)");
  if (std::max(e->o + e->a, HID) > PI_MAX_TALL) return e->fail(SACTD3_EINVAL, "init_params: ob_dim + ac_dim is above what one workgroup orthogonalises");
  if (e->act_inflight) return e->fail(SACTD3_ESTATE, "init_params: an acting call is in flight (sactd3_predict_end first)");
  USE_DEVICE(e);
  InitOrthArgs g{};
  const long scratch = init_mats(e, what, g.m, &g.n);
  RCCHK(first_use_alloc(e, &e->init_scratch, (size_t)scratch, false));      // (never zeroed: a call draws every G it reads)
  RCCHK(first_use_alloc(e, &e->init_redrawn, 4));
  CHAIN_BREAK(e);
  if (what & SACTD3_INIT_ACTOR) RCCHK(actor_write_begin(e));                // the next acting call waits for this one
  if (what & SACTD3_INIT_CRITICS) e->grads_stale[0] = true;                 // the gradient arenas no longer belong to these parameters
  if (what & SACTD3_INIT_ACTOR) e->grads_stale[1] = true;
  g.seed = seed; g.epoch = epoch; g.scratch = e->init_scratch; g.redrawn = e->init_redrawn;
  if (g.n > 0) {
    const hipError_t he = param_init_orth_launch(g, e->stream);
    if (he != hipSuccess) return e->fail(SACTD3_EHIP, "init_params: k_init_orth", he);
  }
  InitFanArgs f{};
  if (what & SACTD3_INIT_ACTOR) f.f[f.nf++] = init_family(e, true);
  if (what & SACTD3_INIT_CRITICS) f.f[f.nf++] = init_family(e, false);
  if (what & SACTD3_INIT_ALPHA) { f.la = e->la; f.la0 = logf(e->cfg.alpha_init); f.t_l = &e->ctl->t_l; f.pw_l = e->ctl->pw_l; }      // (sactd3_create's value)
  const hipError_t he = param_init_fanout_launch(f, e->stream);
  if (he != hipSuccess) return e->fail(SACTD3_EHIP, "init_params: k_init_fanout", he);
  ++e->init_host[0]; e->init_host[1] = g.n;
  return 0;
}

int sactd3_init_stats(sactd3_engine* e, int64_t out[4]) {
  if (!e || !out) return SACTD3_EINVAL;
  const int64_t host[3] = {e->init_host[0], e->init_host[1], 0};
  return stats_with_words(e, host, e->init_redrawn, 1, 2, out);
}

}  // extern "C"
#pragma GCC visibility pop

// ------------------------------------------------------------------------------------------------ the rollout cycle (rollout_cycle.h)
// Not part of the C ABI of this file: include/sactd3_rollout_cycle.h is the rollout handle's (env.hip), which calls in here.
// THE sequence of a cycle, for the graph and for use_graphs == 0 alike: what sactd3_rollout_advance, sactd3_rollout_choose and
// sactd3_step launch, in their order, on one stream -- with the append in the form that reads its cursor on the device.
static_assert(offsetof(DevCtl, rb_len) % 8 == 0 && offsetof(DevCtl, rb_cursor) == offsetof(DevCtl, rb_len) + 4,
              "k_rb_ingest_g reads {rb_len, rb_cursor} as one 8-byte word");
static int launch_ingest_g(EnqCtx& x, const float* records, int n) {
  sactd3_engine* e = x.e;
  IngestArgsG g{};
  g.src = (const float4*)records; g.ring = (float4*)e->ring; g.rec4 = e->rec4; g.n = n; g.cap = e->cfg.rb_capacity;
  g.ring_words = &e->ctl->rb_len; g.clamped = e->cyc_ctr;
  const unsigned blocks = std::min(1024u, ingest_g_blocks(n, e->rec4));      // (k_rb_ingest's bound for a device slab)
  g.publish = blocks == 1 ? 1 : 0;
  hipError_t he = rb_ingest_g_launch(g, blocks, x.s);
  if (he == hipSuccess && !g.publish) he = rb_publish_g_launch(g, x.s);
  return he == hipSuccess ? 0 : e->fail(SACTD3_EHIP, "rollout cycle: k_rb_ingest_g", he);
}
static int enqueue_cycle(EnqCtx& x, const CycleBinding& b, bool explore, bool act, bool polyak) {
  sactd3_engine* e = x.e;
  if (const int he = b.env_step(b.ctx, x.s)) return e->fail(SACTD3_EHIP, "rollout cycle: k_env_step_rec", (hipError_t)he);
  RCCHK(launch_ingest_g(x, b.records, b.n));
  RCCHK(launch_obs_pack(x, b.obs, b.obs_ld, e->p_x, b.n));
  RCCHK(enqueue_predict(x, b.n, explore ? 1 : 0, true));
  RCCHK(launch_act_unpack(x, b.actions, b.actions_ld, b.n));
  return enqueue_step(x, single_iteration(act, polyak));
}

int engine_rollout_cycle(sactd3_engine* e, const CycleBinding& b, int explore, int do_actor) {
  if (!e) return SACTD3_EINVAL;
  // refusals first (the mode's came in front of the call): a refused call has changed nothing, on either side
  if (b.n < 1 || b.n > e->maxn) return e->fail(SACTD3_EINVAL, "rollout_cycle: 1 <= num_envs <= max_envs");
  if (b.n > e->cfg.rb_capacity) return e->fail(SACTD3_EINVAL, "rollout_cycle: num_envs is above rb_capacity (one append launch holds the slab)");
  if ((int64_t)b.n * std::max(std::max(e->ldo, e->a4) / 4, e->rec4) >= (1ll << 31)) return e->fail(SACTD3_EINVAL, "rollout_cycle: too many rows for one launch");
  if (e->rb_pinned > 0) return e->fail(SACTD3_ESTATE, "rollout_cycle: rows are pinned (sactd3_rb_pin): the append's graph form goes round the whole ring");
  if (e->pt_on) return e->fail(SACTD3_ESTATE, "rollout_cycle: priorities are enabled (sactd3_prio_enable): the append would owe their launches");
  if (e->act_inflight) return e->fail(SACTD3_ESTATE, "rollout_cycle: an acting call is in flight (sactd3_predict_end first)");
  USE_DEVICE(e);
  if (e->cyc.owner != b.owner) RCCHK(drop_graphs(e, G_CYCLE, 8));      // the nodes hold the other binding's buffers
  e->cyc = b;      // (a dozen words, every call: the sequence is always enqueued from the binding of the call that asks for it)
  RCCHK(first_use_alloc(e, &e->cyc_ctr, 4));      // (in front of the capture: first_use_alloc)
  const int first = G_CYCLE + (explore ? 0 : 4), id = first + iteration_schedule(e, do_actor, e->qnet_updates + 1).k;
  RCCHK(run_graph(e, id, false));      // capture at the first use (counted in b.stats[1]); nothing is launched yet
  // The rollout's stream around the cycle, once (the pair of SACTD3_SRC_ORDERED): the cycle behind what that stream holds -- a reset, a
  // write of the buffers -- and whatever that stream is given next -- env calls, reads of the buffers -- behind the cycle.
  RCCHK(src_order_begin(e, b.stream, SACTD3_SRC_ORDERED));
  CHAIN_BREAK(e);                                     // the host state of the three calls, by their own routines: sactd3_rb_extend_records_device
  (void)ring_append(e, b.n);                          // ... rb_len, the cursor, rb_wrapped
  predict_device_issued(e, b.n, true);                // sactd3_predict_device
  RCCHK(issue_iteration(e, do_actor, first));         // sactd3_step: THE launch of graph `id` (use_graphs == 0: the sequence itself)
  slot_trained(e, 0, true);
  RCCHK(src_order_end(e, b.stream, SACTD3_SRC_ORDERED));
  ++b.stats[0];
  b.stats[2] = e->graph_nodes[id];
  if (!e->cfg.use_graphs) ++b.stats[3];
  return 0;
}

void engine_rollout_cycle_release(sactd3_engine* e, const void* owner) {
  if (!e || e->cyc.owner != owner) return;
  if (hipSetDevice(e->cfg.device_id) == hipSuccess) (void)drop_graphs(e, G_CYCLE, 8);
  e->cyc = CycleBinding{};
}

int engine_rollout_cycle_clamped(sactd3_engine* e, int64_t* out) {
  if (!e || !out) return SACTD3_EINVAL;
  const int64_t none[4] = {0, 0, 0, 0};
  int64_t got[4];
  RCCHK(stats_with_words(e, none, e->cyc_ctr, 1, 0, got));      // (0 where no cycle was ever issued)
  *out = got[0];
  return 0;
}

// ---- the evaluation rollout (include/sactd3_eval.h), the engine's half: eval_rollout.h.  Like a scoring call it writes its own scratch and
// its own words only: no CHAIN_BREAK, actor_dirty untouched, no batch slot / noise buffer / p_* use, no sample / noise / predict / policy
// counter.  The kernel reads the online actor on the learner stream, behind every update issued so far.
int engine_eval_fail(sactd3_engine* e, int code, const char* what) { return e ? e->fail(code, what) : code; }

int engine_eval_open(sactd3_engine* e, int ob, int ac, int device, int sample, int soft, int64_t rows, void* caller_stream, int flags, EvalActor* out) {
  if (!e) return SACTD3_EINVAL;
  if (!out || ob != e->o || ac != e->a || device != e->cfg.device_id) return e->fail(SACTD3_EINVAL, "eval_rollout: the env does not match the engine");
  if (e->cfg.prefer_td3_over_sac && (sample || soft)) return e->fail(SACTD3_EINVAL, "eval_rollout: SACTD3_EVAL_SAMPLE and soft are SAC only");
  if (rows < 1) return e->fail(SACTD3_EINVAL, "eval_rollout: nothing to roll");
  USE_DEVICE(e);
  RCCHK(first_use_alloc(e, &e->ev_ctr, 32));
  if (rows > e->ev_rows) {      // (never zeroed: the backward pass reads what the forward loop of the same launch wrote)
    float *rew = nullptr, *lp = nullptr;
    RCCHK(first_use_alloc(e, &rew, (size_t)rows, false));
    RCCHK(first_use_alloc(e, &lp, (size_t)rows, false));
    e->ev_rew = rew; e->ev_lp = lp; e->ev_rows = rows;
  }
  RCCHK(src_order_begin(e, (hipStream_t)caller_stream, flags & SACTD3_SRC_ORDERED));
  const NetLayout& L = e->La;
  EvalActor A{};
  A.P = e->Pa; A.ld1 = L.ld1; A.W1 = L.W1; A.b1 = L.b1; A.g1 = L.g1; A.be1 = L.be1; A.W2 = L.W2; A.b2 = L.b2; A.g2 = L.g2; A.be2 = L.be2;
  A.Wh = L.Wh; A.bh = L.bh; A.ln = e->cfg.layer_norm; A.sac = !e->cfg.prefer_td3_over_sac;
  A.scale = e->scale; A.bias = e->bias; A.log_alpha = A.sac ? e->la : nullptr;
  A.seed = &e->ctl->seed; A.eval_ctr = e->ev_ctr; A.rew = e->ev_rew; A.lp = e->ev_lp; A.stream = e->stream;
  *out = A;
  return 0;
}

int engine_eval_close(sactd3_engine* e, int drew, int64_t rows, void* caller_stream, int flags) {
  if (!e) return SACTD3_EINVAL;
  EnqCtx x{e, e->stream};
  if (drew) RCCHK(launch_tick(x, e->ev_ctr));
  RCCHK(src_order_end(e, (hipStream_t)caller_stream, flags & SACTD3_SRC_ORDERED));
  ++e->ev_stats[0]; e->ev_stats[1] += rows;
  if (drew) ++e->ev_stats[2];
  return 0;
}

int engine_eval_stats(sactd3_engine* e, int64_t out[4]) {
  return (!e || !out) ? SACTD3_EINVAL : stats_with_words(e, e->ev_stats, e->ev_ctr, 1, 3, out);
}

// ---- the collected rollout segment (include/sactd3_rollout_collect.h), the engine's half: collect_rollout.h.  The launch reads the online
// actor on the learner stream, behind every update issued so far, and writes the caller's slab; the append that follows is the public
// sactd3_rb_extend_records_device on the same stream (which breaks the run-ahead chain, as every append does).  No sample, noise, predict or
// policy counter moves: the draws are numbered by cl_ctr alone.
int engine_collect_open(sactd3_engine* e, int ob, int ac, int device, int64_t rows, void* rollout_stream, CollectActor* out) {
  if (!e) return SACTD3_EINVAL;
  if (!out || ob != e->o || ac != e->a || device != e->cfg.device_id) return e->fail(SACTD3_EINVAL, "rollout_collect: the env does not match the engine");
  if (rows < 1) return e->fail(SACTD3_EINVAL, "rollout_collect: nothing to roll");
  if (rows > ring_region(e))
    return e->fail(SACTD3_EINVAL, "rollout_collect: steps * num_envs is above the ring slots an append may use (rb_capacity minus the pinned rows)");
  if (e->act_inflight) return e->fail(SACTD3_ESTATE, "rollout_collect: an acting call is in flight (sactd3_predict_end first)");
  USE_DEVICE(e);
  RCCHK(first_use_alloc(e, &e->cl_ctr, 32));
  RCCHK(src_order_begin(e, (hipStream_t)rollout_stream, SACTD3_SRC_ORDERED));
  const NetLayout& L = e->La;
  EvalActor A{};
  A.P = e->Pa; A.ld1 = L.ld1; A.W1 = L.W1; A.b1 = L.b1; A.g1 = L.g1; A.be1 = L.be1; A.W2 = L.W2; A.b2 = L.b2; A.g2 = L.g2; A.be2 = L.be2;
  A.Wh = L.Wh; A.bh = L.bh; A.ln = e->cfg.layer_norm; A.sac = !e->cfg.prefer_td3_over_sac;
  A.scale = e->scale; A.bias = e->bias; A.log_alpha = nullptr;
  A.seed = &e->ctl->seed; A.eval_ctr = e->cl_ctr; A.rew = nullptr; A.lp = nullptr; A.stream = e->stream;
  out->A = A;
  out->noise_std = e->cfg.actor_noise_std;
  return 0;
}

int engine_collect_close(sactd3_engine* e, int drew, void* rollout_stream) {
  if (!e) return SACTD3_EINVAL;
  EnqCtx x{e, e->stream};
  if (drew) RCCHK(launch_tick(x, e->cl_ctr));
  return src_order_end(e, (hipStream_t)rollout_stream, SACTD3_SRC_ORDERED);
}

int engine_collect_stats(sactd3_engine* e, const int64_t host[3], int64_t out[4]) {
  return (!e || !host || !out) ? SACTD3_EINVAL : stats_with_words(e, host, e->cl_ctr, 1, 3, out);
}

#ifdef SACTD3_STAMPS
// diagnostic builds only (make stamps; tools/blocks_probe.py): the per-block begin / end stamps of the last stamped launch
extern "C" __attribute__((visibility("default"))) int sactd3_debug_blocks(sactd3_engine* e, long long* out, int n) {
  if (!e || !out || n < 1 || n > 4096) return SACTD3_EINVAL;
  USE_DEVICE(e);
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_blk), sizeof(long long) * 2 * n));
  return 0;
}
extern "C" __attribute__((visibility("default"))) int sactd3_debug_blocks_select(sactd3_engine* e, int kernel) {
  if (!e) return SACTD3_EINVAL;
  USE_DEVICE(e);
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_blk_kernel), &kernel, sizeof(int)));
  std::vector<long long> z(4096 * 8, 0);
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_blk), z.data(), sizeof(long long) * 4096 * 2));
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_ph), z.data(), sizeof(long long) * 4096 * 8));
  return 0;
}
extern "C" __attribute__((visibility("default"))) int sactd3_debug_phases(sactd3_engine* e, long long* out, int n) {
  if (!e || !out || n < 1 || n > 4096) return SACTD3_EINVAL;
  USE_DEVICE(e);
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ph), sizeof(long long) * 8 * n));
  return 0;
}
#endif
