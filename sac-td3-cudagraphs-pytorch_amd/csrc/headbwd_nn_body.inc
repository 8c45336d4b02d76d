// k_headbwd_nn (HB_BC 0) and k_headbwd_nn_bc (HB_BC 1: TD3+BC, see BcArgs), one body
#if HB_BC
__global__ __launch_bounds__(256) void k_headbwd_nn_bc(HeadBwdNn a, BcArgs bk) {
  __shared__ float bcs[4];
#else
__global__ __launch_bounds__(256) void k_headbwd_nn(HeadBwdNn a) {
#endif
  const ActorHeadBwd& p = a.c;
  constexpr int CB = 16;
  __shared__ __attribute__((aligned(16))) float Dz[16 * AS];
  __shared__ __attribute__((aligned(16))) float cs[2 * 16 * CB];
  __shared__ __attribute__((aligned(16))) float red[4 * 64 * 4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, row = t >> 4, sub = t & 15;
  const int r = lane & 15, kq = lane >> 4;
  int tm, tk;
  xcd_tile(blockIdx.x, (p.B + 15) >> 4, HID / CB, a.xr, tm, tk);
  const int b = tm * 16 + row, bc = min(b, p.B - 1), c_lo = tk * CB;
  const bool valid = b < p.B;
  const int nh = p.L.nh;                         // <= 8, and a <= 8
  const float* Wh = p.P + p.L.Wh;
  // ---- loads first (k_actor_head_bwd_s), then this block's W2 fragments (k_nn's B operand)
  const long ro = (long)bc * HID;
  const Row16 hh = row_ld(p.h2 + ro, sub), xh = row_ld(p.xh2 + ro, sub);
  Row16 g;
  if (p.ln) g = row_ld(p.P + p.L.g2, sub);
  const float rstd = p.ln ? p.rstd2[bc] : 1.f;
  Row16 w[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) w[n] = row_ld(Wh + (long)min(n, nh - 1) * HID, sub);   // unconditional, row clamped
  const bool second = sub >= p.a;
  const int j0 = min(second ? sub - p.a : sub, p.a - 1);
  const float* tgr = p.tg + (long)bc * 4 * p.a4;
  float la = p.sac ? *p.log_alpha : 0.f;
  float o_dA = 0.f, o_dA1 = 0.f;
  // (qa.on) the row's partials: thread `sub` takes float4 #sub, #sub + 16, ... of the row's ntile x pqw floats of each critic
  float4 qv[2] = {f4(0.f), f4(0.f)}, qs[2] = {f4(0.f), f4(0.f)};
  float qrs[2] = {1.f, 1.f};
  if (a.qa.on) {
    const int n4 = a.qa.ntile * a.qa.pqw / 4, s4 = a.qa.ntile * 2;     // float4s per row / of a critic's S partials
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (q < p.nq) {
        const float* pr = a.qa.ps + ((long)q * p.B + bc) * (long)n4 * 4;
        float4 v0 = ld4(pr + 4 * sub), v1 = f4(0.f), v2 = f4(0.f), v3 = f4(0.f);
        if (n4 > 16) v1 = ld4(pr + 4 * (sub + 16));
        if (n4 > 32) { v2 = ld4(pr + 4 * (sub + 32)); v3 = ld4(pr + 4 * (sub + 48)); }
        qv[q] = (v0 + v1) + (v2 + v3);
        const float* sr = a.qa.S + (long)q * s4 * 4;
        float4 t0 = ld4(sr + 4 * sub), t1 = f4(0.f);
        if (s4 > 16) t1 = ld4(sr + 4 * (sub + 16));
        qs[q] = t0 + t1;
        if (a.qa.ln) qrs[q] = a.qa.rstd[(long)q * p.B + bc];
      }
  } else {
    o_dA = p.dA[(long)bc * p.ldA + j0]; o_dA1 = p.nq == 2 ? p.dA[p.dA_ns + (long)bc * p.ldA + j0] : 0.f;
  }
  float o_sc = p.scale[j0], o_t0 = tgr[j0];
#if HB_BC
  // the BC operands, requested with the rest: pi_bj, a_bj, (bc_alpha, bc_weight), this lane's share of |q_pi[0][0 .. B)|
  float o_pi = bk.pi[(long)bc * bk.ld + bk.off + j0], o_ab = bk.act[(long)bc * bk.ld + bk.off + j0];
  float bk_al = bk.ctl[0], bk_w = bk.ctl[1];
  float bk_q = bc_abs_partial(bk.q, p.B, lane);
#endif
  float o_t1 = 0.f, o_t2 = 0.f, o_e = 0.f;
  if (p.sac) { o_t1 = tgr[p.a4 + j0]; o_t2 = tgr[2 * p.a4 + j0]; o_e = p.eps[(long)bc * p.a + j0]; }
  const int nb = 64 * wave + 4 * kq;
  float4 bv[4];
  {
    const float* Wc = a.Wt + (long)nb * a.ldw + c_lo + r;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float* wp = Wc + (long)(16 * c) * a.ldw;
      bv[c] = make_float4(wp[0], wp[a.ldw], wp[2 * (long)a.ldw], wp[3 * (long)a.ldw]);
    }
  }
  float fh[4] = {1.f, 1.f, 1.f, 1.f}, fx[4] = {0.f, 0.f, 0.f, 0.f}, fg = 1.f;      // the epilogue's layer-1 operands (wave 0)
  if (a.f.fold && wave == 0) {
    const int col = c_lo + (lane & 15);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long o = (long)min(tm * 16 + 4 * (lane >> 4) + i, p.B - 1) * HID + col;
      fh[i] = a.f.h1[o]; if (a.f.ln) fx[i] = a.f.xh1[o];
    }
    if (a.f.ln) fg = p.P[a.f.g1_off + col];
  }
  __builtin_amdgcn_sched_barrier(0);
  if (a.qa.on) {
    // sum the tiles: the float4s a thread took all hold the same part of a partial (16 is a multiple of pqw / 4), so lanes with equal
    // sub mod (pqw / 4) add up (DPP row rotations); lane g < pqw / 4 then parks part g of the row's sums in LDS for the whole row to read
    float* Vs = red + (row * 2) * 24;                       // [16 rows][2 critics][16 sums | 8 S]
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (q < p.nq) {
        float v[8] = {qv[q].x, qv[q].y, qv[q].z, qv[q].w, qs[q].x, qs[q].y, qs[q].z, qs[q].w};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          if (k >= 4 || a.qa.pqw == 8) v[k] += dpp_mov<0x122>(v[k]);     // row_ror:2 (S partials are 8 floats: parts 0, 1)
          v[k] += dpp_mov<0x124>(v[k]); v[k] += dpp_mov<0x128>(v[k]);       // row_ror:4, row_ror:8
        }
        if (sub < a.qa.pqw / 4) st4(Vs + q * 24 + 4 * sub, make_float4(v[0], v[1], v[2], v[3]));
        if (sub < 2) st4(Vs + q * 24 + 16 + 4 * sub, make_float4(v[4], v[5], v[6], v[7]));
      }
    const int na = a.qa.a;
    float tot = 0.f;
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (q < p.nq) {
        const float* V = Vs + q * 24;
        const float P = V[j0];
        float dq = P;
        if (a.qa.ln) dq = (P - V[na] * (1.0f / HID) * V[16 + j0] - V[2 * na + 1] * (1.0f / HID) * V[na + 1 + j0]) * qrs[q];
        if (a.qa.dA && tk == 0 && valid && sub < na) a.qa.dA[((long)q * p.B + b) * p.ldA + sub] = dq;
        tot += dq;
      }
    o_dA = tot; o_dA1 = 0.f;
  }
  PIN(la); PIN(o_dA); PIN(o_dA1); PIN(o_sc); PIN(o_t0); PIN(o_t1); PIN(o_t2); PIN(o_e);
#if HB_BC
  PIN(o_pi); PIN(o_ab); PIN(bk_al); PIN(bk_w); PIN(bk_q);
  const float lam = bc_lambda(bk_al, wave_sum(bk_q), p.B), dif = o_pi - o_ab;      // (every wave of every block: the same sum, the same bits)
#endif
  const float dlogp = p.sac ? expf(la) / (float)p.B : 0.f;
  float d;                                        // du[sub]
  {
#if HB_BC
    const float dAj = bc_mix(lam, o_dA + o_dA1, bk_w, bk.inv_ba, dif), sc = o_sc;
#else
    const float dAj = o_dA + o_dA1, sc = o_sc;
#endif
    float g_mean, g_raw = 0.f;
    if (p.sac) {
      const float tt = o_t0, sd = o_t1, yt = o_t2;
      const float omy2 = 1.0f - yt * yt;
      const float g0 = dAj * sc * omy2 + dlogp * (2.0f * sc * yt * omy2) / (sc * omy2 + 1e-6f);
      g_mean = g0;
      g_raw = (g0 * o_e * sd - dlogp) * 3.5f * (1.0f - tt * tt);
    } else {
      g_mean = dAj * sc * (1.0f - o_t0 * o_t0);
    }
    d = second ? g_raw : g_mean;
    if (!valid || sub >= nh) d = 0.f;
  }
  Row16 dh;
#pragma unroll
  for (int q = 0; q < 4; ++q) dh.v[q] = f4(0.f);
  auto add_n = [&](float dn, const Row16& wn) {
#pragma unroll
    for (int q = 0; q < 4; ++q) dh.v[q] = dh.v[q] + wn.v[q] * dn;
  };
  row_pin(w[0]); add_n(dpp_mov<0x150>(d), w[0]);           // row_newbcast:n = lane n of every 16-lane row to all of its lanes
  row_pin(w[1]); add_n(dpp_mov<0x151>(d), w[1]);
  row_pin(w[2]); add_n(dpp_mov<0x152>(d), w[2]);
  row_pin(w[3]); add_n(dpp_mov<0x153>(d), w[3]);
  row_pin(w[4]); add_n(dpp_mov<0x154>(d), w[4]);
  row_pin(w[5]); add_n(dpp_mov<0x155>(d), w[5]);
  row_pin(w[6]); add_n(dpp_mov<0x156>(d), w[6]);
  row_pin(w[7]); add_n(dpp_mov<0x157>(d), w[7]);
#pragma unroll
  for (int c = 0; c < 4; ++c) { PIN(bv[c].x); PIN(bv[c].y); PIN(bv[c].z); PIN(bv[c].w); }
  if (tk == 0 && valid && sub < nh) p.du[(long)b * p.ldu + sub] = d;
  Row16 dy, vals[2];
#pragma unroll
  for (int q = 0; q < 4; ++q) dy.v[q] = gate4(dh.v[q], hh.v[q]);
  const Row16 dz = ln_bwd(dy, xh, rstd, g, p.ln);           // (rows beyond the batch: d = 0 -> all zeros)
#pragma unroll
  for (int q = 0; q < 4; ++q) { vals[0].v[q] = dy.v[q] * xh.v[q]; vals[1].v[q] = dy.v[q]; }
  row_st(Dz + row * AS, sub, dz);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int col = 4 * sub + 64 * q;
    if (col >= c_lo && col < c_lo + CB) {
      if (valid) st4_pol<WT_DZ>(p.dz2, (long)b * HID + col, dz.v[q]);
#pragma unroll
      for (int sl = 0; sl < 2; ++sl) st4(cs + (sl * 16 + row) * CB + (col - c_lo), vals[sl].v[q]);
    }
  }
#if HB_BC
  {
    const float e2 = wave_sum((valid && sub < p.a) ? dif * dif : 0.f);      // this wave's rows' share of sum (pi - a)^2
    if (lane == 0) bcs[wave] = e2;
  }
#endif
  __syncthreads();
#if HB_BC
  if (tk == 0 && t == 0) { bk.part[tm] = (bcs[0] + bcs[1]) + (bcs[2] + bcs[3]); if (tm == 0) *bk.lam = lam; }
#endif
  if (t < 2 * CB) {
    const int sl = t / CB, c = t - sl * CB;
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) sum += cs[(sl * 16 + i) * CB + c];
    p.part[((long)tm * NSLOT + sl) * HID + c_lo + c] = sum;
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 4; ++c) { const float4 av = ld4(Dz + r * AS + nb + 16 * c); MFMA4(acc, av, bv[c]); }
  acc = splitk_reduce(red, acc, wave, lane);
  if (wave == 0) {
    const float o[4] = {acc[0], acc[1], acc[2], acc[3]};
    nn_fold_store(a.f, o, fh, fx, fg, a.dX, a.f.ps, a.f.gsnap, tm * 16, p.B, c_lo + (lane & 15), lane);
  }
}
