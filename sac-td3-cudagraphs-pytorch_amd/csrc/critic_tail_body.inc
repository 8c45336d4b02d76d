// The body of k_critic_tail<RPB> and of its weighted form k_critic_tail_w<RPB> (kernels.h includes this file once inside each, with TAIL_WEIGHTED 0 / 1):
// `p` is the kernel's CriticTail, `wp` the slot's loss weights [B] (weighted form only).  The weight is loaded with the row's rew / done in
// the first batch of loads and multiplies the row's dq and its err^2, nothing else: the column partials, part_s and dz2 follow from dq.
// A textual include and not a __device__ function template: with the body in a function of its own the compiler emitted other
// instructions for the existing kernel (commuted operands, another schedule), and the unweighted form is to keep its machine code.
  __shared__ __attribute__((aligned(16))) float cs[3 * RPB * HID];
  __shared__ float sc[RPB][2];
  const int t = threadIdx.x, row = t >> 4, sub = t & 15, net = blockIdx.y;
  const int b = blockIdx.x * RPB + row, bc = min(b, p.B - 1);
  const bool valid = b < p.B;
  const float* Pn = p.P + net * p.p_ns;
  STAMP(0);
  // loads first
  const Row16 zt0 = row_ld(p.z2t + (long)bc * HID, sub), zt1 = row_ld(p.z2t + ((long)p.B + bc) * HID, sub);
  const Row16 zo = row_ld(p.z2 + ((long)net * p.B + bc) * HID, sub);
  const Row16 wt0 = row_ld(p.PT + p.L.Wh, sub), wt1 = row_ld(p.PT + p.p_ns + p.L.Wh, sub), wo = row_ld(Pn + p.L.Wh, sub);
  Row16 gt0, bt0, gt1, bt1, go, bo;
  if (p.ln) {
    gt0 = row_ld(p.PT + p.L.g2, sub); bt0 = row_ld(p.PT + p.L.be2, sub);
    gt1 = row_ld(p.PT + p.p_ns + p.L.g2, sub); bt1 = row_ld(p.PT + p.p_ns + p.L.be2, sub);
    go = row_ld(Pn + p.L.g2, sub); bo = row_ld(Pn + p.L.be2, sub);
  }
  const float bht0 = p.PT[p.L.bh], bht1 = p.PT[p.p_ns + p.L.bh], bho = Pn[p.L.bh];
  const float rw = p.rew[bc], dn = p.done[bc];
#if TAIL_WEIGHTED
  const float wt = wp[bc];
#endif
  const float alpha = p.sac ? expf(*p.log_alpha) : 0.f;
  const float lpn = p.sac ? p.logp_next[bc] : 0.f;
  STAMP(1);
  Row16 xh, y, h; float rs;
  ln_fwd(zt0, gt0, bt0, p.ln, xh, y, rs);
#pragma unroll
  for (int q = 0; q < 4; ++q) h.v[q] = relu4(y.v[q]);
  const float qt0 = row16_sum(row_dot(h, wt0)) + bht0;
  ln_fwd(zt1, gt1, bt1, p.ln, xh, y, rs);
#pragma unroll
  for (int q = 0; q < 4; ++q) h.v[q] = relu4(y.v[q]);
  const float qt1 = row16_sum(row_dot(h, wt1)) + bht1;
  const float qmin = fminf(qt0, qt1);
  float qp = p.bcq ? 0.75f * qmin + 0.25f * fmaxf(qt0, qt1) : qmin;
  if (p.sac) qp -= alpha * lpn;
  const float yv = rw + (1.0f - dn) * p.gamma * qp;
  float rstd;
  ln_fwd(zo, go, bo, p.ln, xh, y, rstd);
#pragma unroll
  for (int q = 0; q < 4; ++q) h.v[q] = relu4(y.v[q]);
  const float qv = row16_sum(row_dot(h, wo)) + bho;
  const float err = valid ? qv - yv : 0.f;
#if TAIL_WEIGHTED
  const float dq = wt * (2.0f * err / (float)p.B);
#else
  const float dq = 2.0f * err / (float)p.B;
#endif
  Row16 dy, vals[3];
#pragma unroll
  for (int q = 0; q < 4; ++q) dy.v[q] = gate4(wo.v[q] * dq, y.v[q]);
  const Row16 dz = ln_bwd(dy, xh, rstd, go, p.ln);
#pragma unroll
  for (int q = 0; q < 4; ++q) { vals[0].v[q] = dy.v[q] * xh.v[q]; vals[1].v[q] = dy.v[q]; vals[2].v[q] = h.v[q] * dq; }
  if (valid) {
    row_st(p.dz2 + ((long)net * p.B + b) * HID, sub, dz);
    if (sub == 0) {
      p.q[(long)net * p.B + b] = qv;
      if (net == 0) { p.qt[b] = qt0; p.qt[p.B + b] = qt1; p.y[b] = yv; }
    }
  }
#if TAIL_WEIGHTED
  if (sub == 0) { sc[row][0] = dq; sc[row][1] = wt * (err * err); }
#else
  if (sub == 0) { sc[row][0] = dq; sc[row][1] = err * err; }
#endif
  STAMP(2);
  const long blk = (long)net * p.pstride + blockIdx.x;
  block_colsum<RPB>(cs, vals, 3, row, sub, p.part + blk * NSLOT * HID);   // (has the barrier that publishes sc)
  if (t < 2) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < RPB; ++i) s += sc[i][t];
    p.part_s[blk * 2 + t] = s;
  }
  STAMP(3);
