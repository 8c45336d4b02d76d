// k_tn (FIN_BC 0) and k_tn_bc (FIN_BC 1: the TD3+BC actor launch -- the riding block that finalises the loss takes it from BcFin), one body
template <int KT, bool FOLD = false, bool KEEP_G = true>
#if FIN_BC
__global__ __launch_bounds__(256) void k_tn_bc(int h_tiles, int h_pk_blocks, int h_fin_blocks, int h_nprob, int h_tile1, int h_tile2, int h_tile3, int h_M, TnArgs p, BcFin bf) {
#else
__global__ __launch_bounds__(256) void k_tn(int h_tiles, int h_pk_blocks, int h_fin_blocks, int h_nprob, int h_tile1, int h_tile2, int h_tile3, int h_M, TnArgs p) {
#endif
  __shared__ __attribute__((aligned(16))) float red[KT * 4 * 64 * 4];
  __shared__ __attribute__((aligned(16))) float Ys[256 * YS];
  __shared__ __attribute__((aligned(16))) float Xs[KT * 256 * YS];
  __shared__ float cred[16 * 17];                        // bias gradient: [16 partial groups][16 columns]
  __shared__ __attribute__((aligned(16))) float fsum[FOLD ? 16 * 4 * 8 : 4];   // folded LayerNorm backward: [wave x DPP row][column quad][dgamma 4 | dbeta 4]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, net = blockIdx.z;
  const int r = lane & 15, kq = lane >> 4;
  BLK_MARK(0);
  // role and problem from the launch header (HDR_TN): no load in front of the problem's own batch
  const int tiles = HDR_TN ? h_tiles : p.tiles, pk_blocks = HDR_TN ? h_pk_blocks : p.pk_blocks, fin_blocks = HDR_TN ? h_fin_blocks : p.fin_blocks;
  const int M = HDR_TN ? h_M : p.M;
  if ((int)blockIdx.x >= tiles) {                           // (block-uniform) riding blocks
    const int x = (int)blockIdx.x - tiles;
    if (x < pk_blocks) { if (net == 0) polyak_body(p.pk, x, pk_blocks); }
#if FIN_BC
    else if (x - pk_blocks < fin_blocks) {
      adam_red_tail_body<KEEP_G>(p.fin, x - pk_blocks, net);
      if (x - pk_blocks == fin_blocks - 1 && net == 0) bc_loss_finish(bf);      // (the block of the loss and the tick)
    }
#else
    else if (x - pk_blocks < fin_blocks) adam_red_tail_body<KEEP_G>(p.fin, x - pk_blocks, net);      // (behind them: padding up to a multiple of 8 blocks
#endif
    BLK_MARK(1);                                                                                  //  per net, so that every net's tile ids keep their XCDs)
    return;
  }
  const int nprob = HDR_TN ? h_nprob : p.nprob;
  int pi = 0;
  if (nprob > 1 && (int)blockIdx.x >= (HDR_TN ? h_tile1 : p.pr[1].tile0)) pi = 1;
  if (nprob > 2 && (int)blockIdx.x >= (HDR_TN ? h_tile2 : p.pr[2].tile0)) pi = 2;
  if (nprob > 3 && (int)blockIdx.x >= (HDR_TN ? h_tile3 : p.pr[3].tile0)) pi = 3;
  const TnProb q = p.pr[pi];     // ONE batch of scalar loads for the whole problem (field-by-field they came in 3-4 dependent rounds)
  int ldy = q.ldy, ldx = q.ldx;  // (left alone, the compiler fetches these two again in a round of their own, waited for in front of the first operand load)
  // ... and with them what the requests BEHIND the operand batch need (the optimiser state of the block's elements): integers, and
  // copies of the pointers' bits -- a pointer that went through a pin itself would no longer be known to be global (see k_nt)
  long g_ns = p.g_ns;
  int apply = p.apply;
  unsigned long adam_bits = (unsigned long)p.adam, P_bits = (unsigned long)p.P, Mo_bits = (unsigned long)p.Mo, Vo_bits = (unsigned long)p.Vo, T_bits = (unsigned long)p.T;
  if (HDR_TN) {
    ldy = uni(ldy); ldx = uni(ldx); g_ns = uni(g_ns); apply = uni(apply);
    adam_bits = (unsigned long)uni((long)adam_bits); P_bits = (unsigned long)uni((long)P_bits); Mo_bits = (unsigned long)uni((long)Mo_bits);
    Vo_bits = (unsigned long)uni((long)Vo_bits); T_bits = (unsigned long)uni((long)T_bits);
    asm volatile("" : "+s"(ldy), "+s"(ldx), "+s"(g_ns), "+s"(apply), "+s"(adam_bits), "+s"(P_bits), "+s"(Mo_bits), "+s"(Vo_bits), "+s"(T_bits));
  }
  const int local = blockIdx.x - q.tile0;
  const int kw = q.kw > 0 ? q.kw : q.ldw;                 // columns of this problem's piece of dW
  const int tiles_k = (((kw + 15) >> 4) + KT - 1) / KT;
  int tn, tk;
  xcd_tile(local, (q.N + 15) >> 4, tiles_k, q.xr, tn, tk);
  const int n0 = tn * 16, k0 = tk * 16 * KT;
  const long nbase = net * g_ns;
  // the epilogue's elements: wave kt < KT, lane (j = lane & 15, cq = lane >> 4) owns row n0 + j, columns k0 + 16 kt + 4 cq + i: 16
  // bytes of one weight row (the MFMAs below take X as their A operand, so the accumulator holds the tile transposed), one request
  // per array instead of four.  A piece whose width, row stride or offset is no multiple of 4 takes them one by one (block-uniform)
  const int erow = n0 + (lane & 15), ecol = k0 + 16 * min(wave, KT - 1) + 4 * (lane >> 4);
  const bool vec4 = uni(((kw | q.ldw | q.w_off) & 3) | (int)(g_ns & 3)) == 0;
  AdamState4 st{f4(0.f), f4(0.f), f4(0.f), f4(0.f)};
  const AdamState sv = {0.f, 0.f, 0.f, 0.f};
  STAMP(0); BLK_PH(0);
  // operand tiles are column slices ([M rows][16 floats]): fetched as float4 (64-byte pieces), transposed through LDS
  const float* dYn = q.dY + net * q.dy_ns;
  const float* Xn = q.X + net * q.x_ns;
  const int Nr = (q.N + 3) & ~3, Kr = (q.K + 3) & ~3;     // rows hold at least round4(.) floats
  f32x4 acc[KT];
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) acc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float asum = 0.f;                                       // thread (col = t & 15, part = t >> 4): partial column sums of dY
  float4 vy[4], vx[KT][4];
  const bool fold = FOLD && q.fold != 0, fold_ln = fold && q.f_ln;   // (block-uniform)
  float4 vxh[4], vp1[4], vp2[4], gq = f4(1.f), cg = f4(0.f), cb = f4(0.f);
  float vrs[4];
  auto fetch = [&](int mb) {                      // raw loads; masked when the slab is parked in LDS, a stage later (see ld4_raw)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = t + 256 * u, row = i >> 2, c4 = i & 3, m = mb + row, n = n0 + 4 * c4, k = k0 + 4 * c4;
      const long mc = min(m, M - 1);
      vy[u] = ld4_raw(dYn + mc * ldy, n, Nr);
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) vx[kt][u] = ld4_raw(Xn + mc * ldx, k + 16 * kt, Kr);
      if (fold_ln) {
        const long rn = (long)net * M + mc;
        vxh[u] = ld4(q.f_xh + rn * HID + n);
        vp1[u] = ld4(q.f_ps + rn * PS_W + 4 * c4);
        vp2[u] = ld4(q.f_ps + rn * PS_W + 16 + 4 * c4);
        vrs[u] = q.f_rstd[rn];
      }
    }
  };
  fetch(0);
  if (fold_ln) gq = ld4(q.f_g + net * HID + n0 + 4 * (t & 3));
  const float step = apply ? p.adam[0] : 0.f, sq2 = apply ? p.adam[1] : 1.f;
  // clamped, not predicated (the commit is predicated).  Only the 16-byte form asks here: a second form of this request, joined
  // with it, made the compiler wait for the whole operand batch in front of both (the 4-byte form fetches where it commits)
  if (wave < KT && vec4) st = adam_fetch4(p, nbase + q.w_off + (long)min(erow, q.N - 1) * q.ldw + min(ecol, kw - 4));
  // k-tile-0 blocks also produce the bias gradient of their 16 columns (column sums of dY, collected from the LDS tile in the
  // main loop): wave 3, lanes 0 .. 15 commit it; its optimiser state is requested now
  const int fcol = t & 15, fpart = t >> 4, fn = n0 + fcol;         // (column, partial-group) of this thread
  const bool want_bias = tk == 0 && q.b_off >= 0;
  AdamState fstate = sv;
  long foff = -1;
  if (want_bias && wave == 3 && lane < 16 && fn < q.N) { foff = nbase + q.b_off + fn; fstate = adam_fetch(p, foff); }
  const bool fold_vec = fold_ln && tk == 0;                // dgamma1 / dbeta1 of the 16 columns: wave 3, lanes 16 .. 31 / 32 .. 47
  if (fold_vec && wave == 3 && lane >= 16 && lane < 48) { foff = nbase + (lane < 32 ? q.f_g_off : q.f_be_off) + fn; fstate = adam_fetch(p, foff); }
  for (int mb = 0; mb < M; mb += 256) {
    if (mb) __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
    STAMP(1); BLK_PH(1);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = t + 256 * u, c4 = i & 3;
      const bool row_ok = mb + (i >> 2) < M;
      if (fold) {                                          // N = HID: no column mask
        float4 dz = row_ok ? vy[u] : f4(0.f);
        if (fold_ln) {
          const float a1 = sum4(vp1[u]), a2 = sum4(vp2[u]);                       // 4 of the 16 tile partials each; the quad holds the row
          const float s1 = (dpp_mov<0x00>(a1) + dpp_mov<0x55>(a1)) + (dpp_mov<0xAA>(a1) + dpp_mov<0xFF>(a1));   // quad_perm broadcasts
          const float s2 = (dpp_mov<0x00>(a2) + dpp_mov<0x55>(a2)) + (dpp_mov<0xAA>(a2) + dpp_mov<0xFF>(a2));
          const float m1 = s1 * (1.0f / HID), m2 = s2 * (1.0f / HID);
          const float4 dy = dz;
          cg = cg + dy * vxh[u]; cb = cb + dy;
          dz = (dy * gq - f4(m1) - vxh[u] * m2) * vrs[u];                         // ln_bwd's expression
          if (!row_ok) dz = f4(0.f);
        }
        st4(Ys + (i >> 2) * YS + 4 * c4, dz);
        if (tk == 0 && row_ok && q.f_dz) st4(q.f_dz + ((long)net * M + mb + (i >> 2)) * HID + n0 + 4 * c4, dz);
      } else
      st4(Ys + (i >> 2) * YS + 4 * c4, mask4_cols(vy[u], n0 + 4 * c4, q.N, row_ok));
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) st4(Xs + kt * 256 * YS + (i >> 2) * YS + 4 * c4, mask4_cols(vx[kt][u], k0 + 4 * c4 + 16 * kt, q.K, row_ok));
    }
    __builtin_amdgcn_sched_barrier(0);
    if (mb + 256 < M) fetch(mb + 256);                   // the next slab's rows fly under this slab's MFMAs
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {                          // wave w: 16-row chunks w, w+4, w+8, w+12 of this slab
      const float* y0 = Ys + (16 * (wave + 4 * u) + 4 * kq) * YS + r;
      const float4 a = make_float4(y0[0], y0[YS], y0[2 * YS], y0[3 * YS]);
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        const float* x0 = Xs + kt * 256 * YS + (16 * (wave + 4 * u) + 4 * kq) * YS + r;
        const float4 b = make_float4(x0[0], x0[YS], x0[2 * YS], x0[3 * YS]);
        MFMA4(acc[kt], b, a);                                // D[k][n]: the same products in the same order as D[n][k] of (a, b)
      }
    }
    if (want_bias) {
      const int col = t & 15, part = t >> 4;
#pragma unroll
      for (int i = 0; i < 16; ++i) asum += Ys[(part * 16 + i) * YS + col];
    }
  }
  STAMP(2); BLK_PH(2);
  // sum the 4 waves' accumulators of every tile (split-M); wave kt gets the total of tile kt
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) st4(red + ((kt * 4 + wave) * 64 + lane) * 4, make_float4(acc[kt][0], acc[kt][1], acc[kt][2], acc[kt][3]));
  if (want_bias) cred[fpart * 17 + fcol] = asum;
  if (fold_vec) {                                          // lanes with equal (lane & 3) hold the same 4 columns: sum the 4 of a DPP row,
    float v[8] = {cg.x, cg.y, cg.z, cg.w, cb.x, cb.y, cb.z, cb.w};     // then one partial per (wave, row) into LDS
#pragma unroll
    for (int j = 0; j < 8; ++j) { v[j] += dpp_mov<0x124>(v[j]); v[j] += dpp_mov<0x128>(v[j]); }   // row_ror:4, row_ror:8
    if ((lane & 15) < 4) {
      float* d = fsum + ((wave * 4 + (lane >> 4)) * 4 + (lane & 3)) * 8;
      st4(d, make_float4(v[0], v[1], v[2], v[3])); st4(d + 4, make_float4(v[4], v[5], v[6], v[7]));
    }
  }
  __syncthreads();
  STAMP(3); BLK_PH(3);
  if (!KEEP_G) {          // (without the arena store in front of it, each row's branch below would be the first use of its optimiser
#pragma unroll           //  state, and every group of stores would wait for the previous group's: PIN)
    for (int i = 0; i < 4; ++i) { PIN(f4r(st.w, i)); PIN(f4r(st.m, i)); PIN(f4r(st.v, i)); PIN(f4r(st.t, i)); }
    PIN(fstate.w); PIN(fstate.m); PIN(fstate.v); PIN(fstate.t);
  }
  if (wave < KT && ecol < kw && erow < q.N) {
    const float* rr = red + (wave * 4 * 64 + lane) * 4;
    const float4 a = ld4(rr), b = ld4(rr + 256), c = ld4(rr + 512), d = ld4(rr + 768);
    const float o[4] = {(a.x + b.x) + (c.x + d.x), (a.y + b.y) + (c.y + d.y), (a.z + b.z) + (c.z + d.z), (a.w + b.w) + (c.w + d.w)};
    const float4 g = make_float4(ecol < q.K ? o[0] : 0.f, ecol + 1 < q.K ? o[1] : 0.f, ecol + 2 < q.K ? o[2] : 0.f, ecol + 3 < q.K ? o[3] : 0.f);
    const long off = nbase + q.w_off + (long)erow * q.ldw + ecol;
    if (vec4) adam_commit4<KEEP_G>(p, off, g, st, step, sq2);       // (ecol < kw, both multiples of 4: all 4 columns are the piece's)
    else {                                                          // (no layout the engine builds comes here: rolled, a round trip per element)
#pragma unroll 1
      for (int i = 0; i < 4; ++i) {
        if (ecol + i < kw) adam_commit<KEEP_G>(p, off + i, f4c(g, i), adam_fetch(p, off + i), step, sq2);
      }
    }
  }
  if (foff >= 0) {
    float v = 0.f;
    if (lane < 16) {
#pragma unroll
      for (int i = 0; i < 16; ++i) v += cred[i * 17 + fcol];
    } else {
      const float* f = fsum + (fcol >> 2) * 8 + (lane < 32 ? 0 : 4) + (fcol & 3);
#pragma unroll
      for (int i = 0; i < 16; ++i) v += f[i * 32];
    }
    adam_commit<KEEP_G>(p, foff, v, fstate, step, sq2);
  }
  STAMP(4); BLK_PH(4);
  BLK_MARK(1);
}
