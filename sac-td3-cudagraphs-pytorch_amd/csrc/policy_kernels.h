// Querying the policy on caller-supplied rows (include/sactd3.h: sactd3_policy_device): device code.
// Included by engine.hip behind mix_kernels.h.  The two kernels are plain ones, like k_actor_tail: they stand with the plain kernels in
// front of every template instance, and csrc/kernel_instances.inc -- whose last lines tests/test_prior_data_host.py pins -- stays as it is.
//
// k_pi_head is the forward half of the acting tail and nothing else, on the z2 rows the actor trunk left in the feature's own scratch:
// layer-2 LayerNorm + ReLU (ln_fwd), the head product u = h2 Wh^T + bh, then per action dimension j (float32, one rounding per
// written operation; sc / bi = the engine's action_scale / action_bias, C = 0.9189385332046727f):
//   SAC (nh = 2a; mean_j = u_j, raw_j = u_{a+j})
//     tt = tanhf(raw), log_std = -5 + 3.5 (tt + 1), sd = expf(log_std)
//     mode   = tanhf(mean) sc + bi
//     sample: x = mean + e sd, y = tanhf(x), sample = y sc + bi, dx = x - mean,
//             el = -(dx dx) / (2 sd sd) - logf(sd) - C - logf(sc (1 - y y) + 1e-6f);   sample_logp = sum_j el_j
//     given action g (the inverse squash):
//             v = (g - bi) / sc, c = min(max(v, -M), M) with M = float32(1 - 1e-6) = 0x3F7FFFEF,
//             x' = 0.5f (logf(1 + c) - logf(1 - c)), d' = x' - mean,
//             el' = -(d' d') / (2 sd sd) - logf(sd) - C - logf(sc (1 - c c) + 1e-6f);  action_logp = sum_j el'_j
//             a row with any |v_j| > M is counted once as clamped; a row with a NaN component gets a quiet-NaN action_logp and is
//             counted once as NaN -- no other output of the row, and no other row, is affected
//   TD3 (nh = a): mode = tanhf(u) sc + bi only.
// The head product and the row sums are formed the way the acting tail of the same head shape forms them, so that `mode` has the bits
// of that tail's exploit action for the same z2 row and `sample` / `sample_logp` those of its exploring one for the same draw:
//   k_pi_head_s    narrow heads (nh <= 8 and a <= 8, where launch_tails takes k_actor_tail_s): 16 threads per row, a row in one wave,
//                  every head output row16_sum(row_dot(h, w_n)) + bh
//   k_pi_head      every other head (k_actor_tail): MFMA with K split over the four waves, ((u_w0 + u_w1) + (u_w2 + u_w3)) + bh
// and both sum el over j with row16_sum (a second element of a lane, j >= 16, is added to the lane's first beforehand).
// Draws e: the caller's `eps`, or -- eps == NULL -- philox_normal on the stream SACTD3_STREAM_POLICY with counter words
// (policy_ctr, 0, 0x400, element >> 2), element = row_of_call a + j.  The kernel only reads policy_ctr (PiCtl, a line of the
// feature's own); the host advances it behind the last chunk of a call that drew natively (k_tick).
// Memory discipline as in kernels.h: all loads go out before the first global store, addresses are clamped and never derived from a
// row's data; plain vector stores, each output only inside its [n, width] window at the caller's stride, none for a NULL output; the
// only atomics are one atomicAdd per counted row on PiCtl::clamped / nan_rows.
#pragma once

struct PiCtl {
  int policy_ctr;     // stream counter of the native draws: advanced once per call that draws natively
  int clamped;        // rows with a given action component outside [-M, M] after unscaling
  int nan_rows;       // rows with a NaN component in their given action
  int pad[29];
};
static_assert(sizeof(PiCtl) == 128, "one line");

struct PiHead {
  const float* z2;                       // [n][HID] pre-LN output of hidden layer 2
  const float* P; NetLayout L;           // actor parameter block (online; TD3: online or target)
  int n, a, ln, sac;
  int draw;                              // a sample is wanted (sample, sample_logp or eps_out)
  const float* scale; const float* bias;
  const DevCtl* ctl; PiCtl* pc;          // seed; the feature's counter and row counters
  long row0;                             // row of the call that row 0 of this launch is (the chunk's offset)
  const float* actions; long actions_ld; // in : [n][a] or NULL
  const float* eps; long eps_ld;         // in : [n][a] or NULL (native draws)
  float* mode; long mode_ld;
  float* mean; long mean_ld;
  float* log_std; long log_std_ld;
  float* sample; long sample_ld;
  float* sample_logp; long sample_logp_ld;
  float* action_logp; long action_logp_ld;
  float* eps_out; long eps_out_ld;
};

struct PiEl { float mode, mean, log_std, sample, el, elp; bool clamped, isnan; };
// one action dimension: u0 / u1 = the head outputs (bias added), e the draw, g the given action
__device__ __forceinline__ PiEl pi_element(float u0, float u1, float sc, float bi, float e, float g, int sac) {
  PiEl r;
  r.mode = tanhf(u0) * sc + bi;
  r.mean = u0; r.log_std = 0.f; r.sample = 0.f; r.el = 0.f; r.elp = 0.f; r.clamped = false; r.isnan = false;
  if (sac) {
    const float tt = tanhf(u1);
    const float log_std = -5.0f + 3.5f * (tt + 1.0f);
    const float sd = expf(log_std);
    const float x = u0 + e * sd;
    const float yt = tanhf(x);
    r.sample = yt * sc + bi;
    const float dx = x - u0;
    float l = -(dx * dx) / (2.0f * sd * sd) - logf(sd) - 0.9189385332046727f;
    l -= logf(sc * (1.0f - yt * yt) + 1e-6f);
    r.el = l; r.log_std = log_std;
    const float M = __uint_as_float(0x3F7FFFEFu);      // float32(1 - 1e-6)
    const float v = (g - bi) / sc;
    const float c = fminf(fmaxf(v, -M), M);
    const float xp = 0.5f * (logf(1.0f + c) - logf(1.0f - c));
    const float dp = xp - u0;
    r.elp = -(dp * dp) / (2.0f * sd * sd) - logf(sd) - 0.9189385332046727f - logf(sc * (1.0f - c * c) + 1e-6f);
    r.clamped = fabsf(v) > M;
    r.isnan = g != g;
  }
  return r;
}

template <int RPB>
__device__ __forceinline__ void pi_head_body(const PiHead& p) {
  constexpr bool WIDE = RPB == 16;
  static_assert(RPB == 4 || RPB == 16, "4 rows per wave-sized block (narrow heads) or 16 per 256 threads");
  const int t = threadIdx.x, row = t >> 4, sub = t & 15;
  const int b = blockIdx.x * RPB + row, bc = min(b, p.n - 1);
  const bool valid = b < p.n;
  const int nh = p.L.nh;
  const float* Wh = p.P + p.L.Wh;
  // ---- loads: stream state, my row, LN affine, head weights, the operands of this thread's one or two output elements
  const bool native = p.draw && !p.eps;            // (uniform)
  unsigned long long seed = 0ull; int ctr = 0;
  if (native) { seed = p.ctl->seed; ctr = p.pc->policy_ctr; }
  const Row16 z = row_ld(p.z2 + (long)bc * HID, sub);
  const Row16 g = row_ld(p.P + (p.ln ? p.L.g2 : 0), sub), be = row_ld(p.P + (p.ln ? p.L.be2 : 0), sub);
  const bool two = WIDE && p.a > 16;               // (uniform) a second element per thread: ac_dim in 17 .. 32
  int jc[2]; float bh0[2], bh1[2], sc[2], bi[2], gin[2], ein[2], enat[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    jc[k] = min(sub + 16 * k, p.a - 1);
    bh0[k] = bh1[k] = sc[k] = bi[k] = gin[k] = ein[k] = enat[k] = 0.f;
    if (k == 0 || two) {
      bh0[k] = p.P[p.L.bh + jc[k]]; bh1[k] = p.sac ? p.P[p.L.bh + p.a + jc[k]] : 0.f;
      sc[k] = p.scale[jc[k]]; bi[k] = p.bias[jc[k]];
      if (p.actions) gin[k] = p.actions[(long)bc * p.actions_ld + jc[k]];
      if (p.eps) ein[k] = p.eps[(long)bc * p.eps_ld + jc[k]];
      if (native) enat[k] = philox_normal(seed, (unsigned)ctr, SACTD3_STREAM_POLICY, (unsigned)((p.row0 + bc) * p.a + jc[k]));
    }
  }
  float u0[2] = {0.f, 0.f}, u1[2] = {0.f, 0.f};
  if constexpr (!WIDE) {
    Row16 w[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) w[n] = row_ld(Wh + (long)min(n, nh - 1) * HID, sub);   // unconditional, row clamped
    Row16 xh, y, h; float rstd;
    ln_fwd(z, g, be, p.ln, xh, y, rstd);
#pragma unroll
    for (int q = 0; q < 4; ++q) h.v[q] = relu4(y.v[q]);
    float d0 = 0.f, d1 = 0.f;
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      row_pin(w[n]);
      const float tot = row16_sum(row_dot(h, w[n]));
      if (n < nh) { d0 = (n == sub) ? tot : d0; d1 = (n == p.a + sub) ? tot : d1; }
    }
    u0[0] = d0 + bh0[0]; u1[0] = d1 + bh1[0];
  } else {
    __shared__ __attribute__((aligned(16))) float Hs[16 * AS];
    __shared__ float Up[4 * 16 * 64];
    const int lane = t & 63, wave = t >> 6, r = lane & 15, kq = lane >> 4;
    const int T = (nh + 15) >> 4;                  // head column tiles (<= 4)
    float4 wf[4][4];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) wf[tt][ci] = ld4(Wh + (long)min(tt * 16 + r, nh - 1) * HID + (4 * wave + ci) * 16 + 4 * kq);
    Row16 xh, y, h; float rstd;
    ln_fwd(z, g, be, p.ln, xh, y, rstd);
#pragma unroll
    for (int q = 0; q < 4; ++q) h.v[q] = relu4(y.v[q]);
    row_st(Hs + row * AS, sub, h);
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) {
        PIN(wf[tt][ci].x); PIN(wf[tt][ci].y); PIN(wf[tt][ci].z); PIN(wf[tt][ci].w);
        if (tt * 16 + r >= nh) wf[tt][ci] = f4(0.f);
      }
    __syncthreads();
    {
      f32x4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) {
        const float4 av = ld4(Hs + r * AS + (4 * wave + ci) * 16 + 4 * kq);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
          if (tt < T) { MFMA4(acc[tt], av, wf[tt][ci]); }
      }
#pragma unroll
      for (int tt = 0; tt < 4; ++tt)
        if (tt < T)
#pragma unroll
          for (int i = 0; i < 4; ++i) Up[(wave * 16 + 4 * kq + i) * 64 + tt * 16 + r] = acc[tt][i];
    }
    __syncthreads();
    const float* u = Up + row * 64;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int j = jc[k], ja = min(p.a + j, 63);
      u0[k] = ((u[j] + u[1024 + j]) + (u[2048 + j] + u[3072 + j])) + bh0[k];
      u1[k] = p.sac ? ((u[ja] + u[1024 + ja]) + (u[2048 + ja] + u[3072 + ja])) + bh1[k] : 0.f;
    }
  }
  // everything requested above is here before the first store goes out
#pragma unroll
  for (int k = 0; k < 2; ++k) { PIN(bh0[k]); PIN(bh1[k]); PIN(sc[k]); PIN(bi[k]); PIN(gin[k]); PIN(ein[k]); }
  float lp = 0.f, lpa = 0.f, ncl = 0.f, nnan = 0.f;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int j = sub + 16 * k;
    if ((k == 0 || two) && j < p.a) {
      const float e = p.draw ? (p.eps ? ein[k] : enat[k]) : 0.f;
      const PiEl r = pi_element(u0[k], u1[k], sc[k], bi[k], e, gin[k], p.sac);
      lp += r.el; lpa += r.elp;
      ncl += r.clamped ? 1.f : 0.f; nnan += r.isnan ? 1.f : 0.f;
      if (valid) {
        if (p.mode) p.mode[(long)b * p.mode_ld + j] = r.mode;
        if (p.mean) p.mean[(long)b * p.mean_ld + j] = r.mean;
        if (p.log_std) p.log_std[(long)b * p.log_std_ld + j] = r.log_std;
        if (p.sample) p.sample[(long)b * p.sample_ld + j] = r.sample;
        if (p.eps_out) p.eps_out[(long)b * p.eps_out_ld + j] = e;
      }
    }
  }
  if (p.sac) {                                     // (uniform)
    lp = row16_sum(lp);
    if (p.sample_logp && sub == 0 && valid) p.sample_logp[(long)b * p.sample_logp_ld] = lp;
    if (p.actions) {
      lpa = row16_sum(lpa); ncl = row16_sum(ncl); nnan = row16_sum(nnan);
      if (sub == 0 && valid) {
        if (p.action_logp) p.action_logp[(long)b * p.action_logp_ld] = nnan > 0.f ? __uint_as_float(0x7FC00000u) : lpa;
        if (ncl > 0.f) atomicAdd(&p.pc->clamped, 1);
        if (nnan > 0.f) atomicAdd(&p.pc->nan_rows, 1);
      }
    }
  }
}
__global__ __launch_bounds__(256) void k_pi_head(PiHead p) { pi_head_body<16>(p); }
__global__ __launch_bounds__(64) void k_pi_head_s(PiHead p) { pi_head_body<4>(p); }
