// k_actor_head_bwd (HB_BC 0) and k_actor_head_bwd_bc (HB_BC 1: TD3+BC, see BcArgs), one body
#if HB_BC
__global__ __launch_bounds__(256) void k_actor_head_bwd_bc(ActorHeadBwd p, BcArgs bk) {
  __shared__ float bcs[4];
#else
__global__ __launch_bounds__(256) void k_actor_head_bwd(ActorHeadBwd p) {
#endif
  __shared__ __attribute__((aligned(16))) float cs[2 * 16 * HID];   // also holds dh2 [16][AS] before the column sums
  __shared__ __attribute__((aligned(16))) float Du[16 * 68];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int row = t >> 4, sub = t & 15, r = lane & 15, kq = lane >> 4;
  const int b = blockIdx.x * 16 + row, bc = min(b, p.B - 1);
  const bool valid = b < p.B;
  const int nh = p.L.nh, C = (nh + 15) >> 4;      // k chunks of the head-backward product (<= 4)
  const float* Wh = p.P + p.L.Wh;
  // loads first
  const long ro = (long)bc * HID;
  const Row16 hh = row_ld(p.h2 + ro, sub), xh = row_ld(p.xh2 + ro, sub);
  Row16 g;
  if (p.ln) g = row_ld(p.P + p.L.g2, sub);
  const float rstd = p.ln ? p.rstd2[bc] : 1.f;
  float4 wf[4][4];                       // B operand of dh2 = du Wh: Wh[k = 16c + 4kq + jj][n = (4*tt + wave)*16 + r]
#pragma unroll
  for (int tt = 0; tt < 4; ++tt)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int n = (4 * tt + wave) * 16 + r, k = 16 * c + 4 * kq;
      wf[tt][c] = f4(0.f);
      if (c < C) {
        if (k < nh) wf[tt][c].x = Wh[(long)k * HID + n];
        if (k + 1 < nh) wf[tt][c].y = Wh[(long)(k + 1) * HID + n];
        if (k + 2 < nh) wf[tt][c].z = Wh[(long)(k + 2) * HID + n];
        if (k + 3 < nh) wf[tt][c].w = Wh[(long)(k + 3) * HID + n];
      }
    }
  // operands of this thread's first head element (j = sub), requested with the rest (see k_actor_tail)
  const int j0 = min(sub, p.a - 1);
  const float* tgr = p.tg + (long)bc * 4 * p.a4;
  float la = p.sac ? *p.log_alpha : 0.f;
  float o_dA = p.dA[(long)bc * p.ldA + j0], o_dA1 = p.nq == 2 ? p.dA[p.dA_ns + (long)bc * p.ldA + j0] : 0.f;
  float o_sc = p.scale[j0], o_t0 = tgr[j0];
  float o_t1 = 0.f, o_t2 = 0.f, o_e = 0.f;
  if (p.sac) { o_t1 = tgr[p.a4 + j0]; o_t2 = tgr[2 * p.a4 + j0]; o_e = p.eps[(long)bc * p.a + j0]; }
#if HB_BC
  // the BC operands, requested with the rest: pi_bj, a_bj, (bc_alpha, bc_weight), this lane's share of |q_pi[0][0 .. B)|
  const float* pir = bk.pi + (long)bc * bk.ld + bk.off;
  const float* abr = bk.act + (long)bc * bk.ld + bk.off;
  float o_pi = pir[j0], o_ab = abr[j0];
  float bk_al = bk.ctl[0], bk_w = bk.ctl[1];
  float bk_q = bc_abs_partial(bk.q, p.B, lane);
#endif
  for (int j = sub; j < 64; j += 16) Du[row * 68 + j] = 0.f;
  PIN(la); PIN(o_dA); PIN(o_dA1); PIN(o_sc); PIN(o_t0); PIN(o_t1); PIN(o_t2); PIN(o_e);
#if HB_BC
  PIN(o_pi); PIN(o_ab); PIN(bk_al); PIN(bk_w); PIN(bk_q);
#endif
  __syncthreads();
#if HB_BC
  const float lam = bc_lambda(bk_al, wave_sum(bk_q), p.B);      // (every wave of every block: the same sum, the same bits)
  float e2 = 0.f;
  auto mix = [&](float dAj, float pi, float ab) {
    const float dif = pi - ab;
    if (valid) e2 += dif * dif;
    return bc_mix(lam, dAj, bk_w, bk.inv_ba, dif);
  };
#endif
  const float dlogp = p.sac ? expf(la) / (float)p.B : 0.f;
  auto element = [&](int j, float dAj, float sc, float t0, float t1, float t2, float e) {
    float g_mean, g_raw = 0.f;
    if (p.sac) {
      const float tt = t0, sd = t1, yt = t2;
      const float omy2 = 1.0f - yt * yt;
      const float g0 = dAj * sc * omy2 + dlogp * (2.0f * sc * yt * omy2) / (sc * omy2 + 1e-6f);
      g_mean = g0;
      g_raw = (g0 * e * sd - dlogp) * 3.5f * (1.0f - tt * tt);
    } else {
      const float th = t0;
      g_mean = dAj * sc * (1.0f - th * th);
    }
    if (!valid) { g_mean = 0.f; g_raw = 0.f; }
    Du[row * 68 + j] = g_mean;
    if (p.sac) Du[row * 68 + p.a + j] = g_raw;
    if (valid) {
      p.du[(long)b * p.ldu + j] = g_mean;
      if (p.sac) p.du[(long)b * p.ldu + p.a + j] = g_raw;
    }
  };
#if HB_BC
  if (sub < p.a) element(sub, mix(o_dA + o_dA1, o_pi, o_ab), o_sc, o_t0, o_t1, o_t2, o_e);
#else
  if (sub < p.a) element(sub, o_dA + o_dA1, o_sc, o_t0, o_t1, o_t2, o_e);
#endif
  for (int j = sub + 16; j < p.a; j += 16) {            // ac_dim > 16 only
    float dAj = p.dA[(long)bc * p.ldA + j];
    if (p.nq == 2) dAj += p.dA[p.dA_ns + (long)bc * p.ldA + j];
#if HB_BC
    dAj = mix(dAj, pir[j], abr[j]);
#endif
    element(j, dAj, p.scale[j], tgr[j], p.sac ? tgr[p.a4 + j] : 0.f, p.sac ? tgr[2 * p.a4 + j] : 0.f, p.sac ? p.eps[(long)bc * p.a + j] : 0.f);
  }
#if HB_BC
  e2 = wave_sum(e2);                       // this wave's rows' share of sum (pi - a)^2
  if (lane == 0) bcs[wave] = e2;
#endif
  __syncthreads();
#if HB_BC
  if (t == 0) { bk.part[blockIdx.x] = (bcs[0] + bcs[1]) + (bcs[2] + bcs[3]); if (blockIdx.x == 0) *bk.lam = lam; }
#endif
  // dh2[16][256] = du[16][nh] Wh[nh][256]; wave w owns column tiles w, w+4, w+8, w+12
  float* DH = cs;
#pragma unroll
  for (int tt = 0; tt < 4; ++tt) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) { const float4 av = ld4(Du + r * 68 + 16 * c + 4 * kq); MFMA4(acc, av, wf[tt][c]); }
#pragma unroll
    for (int i = 0; i < 4; ++i) DH[(4 * kq + i) * AS + (4 * tt + wave) * 16 + r] = acc[i];
  }
  __syncthreads();
  const Row16 dh = row_ld(DH + row * AS, sub);
  __syncthreads();                       // DH is reused by the column sums below
  Row16 dy, vals[2];
#pragma unroll
  for (int q = 0; q < 4; ++q) dy.v[q] = gate4(dh.v[q], hh.v[q]);
  const Row16 dz = ln_bwd(dy, xh, rstd, g, p.ln);
  if (valid) row_st(p.dz2 + (long)b * HID, sub, dz);
#pragma unroll
  for (int q = 0; q < 4; ++q) { vals[0].v[q] = dy.v[q] * xh.v[q]; vals[1].v[q] = dy.v[q]; }
  block_colsum<16>(cs, vals, 2, row, sub, p.part + (long)blockIdx.x * NSLOT * HID);
}
