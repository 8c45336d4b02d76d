// k_adam_red (FIN_BC 0) and k_adam_red_bc (FIN_BC 1: the TD3+BC actor launch on the split-M route), one body
template <bool KEEP_G = true>
#if FIN_BC
__global__ __launch_bounds__(256) void k_adam_red_bc(AdamRedArgs a, BcFin bf) {
#else
__global__ __launch_bounds__(256) void k_adam_red(AdamRedArgs a) {
#endif
  const int net = blockIdx.y, t = threadIdx.x;
  const int main_blocks = (int)((a.g_ns / 4 + 255) / 256);
  const int bx = blockIdx.x;
#if FIN_BC
  if (bx >= main_blocks) {
    adam_red_tail_body<KEEP_G>(a, bx - main_blocks, net);
    if (bx - main_blocks == 4 * a.nvec && net == 0) bc_loss_finish(bf);
    return;
  }
#else
  if (bx >= main_blocks) { adam_red_tail_body<KEEP_G>(a, bx - main_blocks, net); return; }
#endif
  const float step = a.apply ? a.adam[0] : 0.f, sq2 = a.apply ? a.adam[1] : 1.f;
  // slab-sourced elements: one float4 per thread (the vector ranges and the scalar's float4 belong to the tail blocks)
  const long i = ((long)bx * 256 + t) * 4;
  bool mine = i < a.g_ns && !(a.s_off >= 0 && i == a.s_off);
#pragma unroll
  for (int e = 0; e < 5; ++e)
    if (e < a.nvec && i >= a.vec[e].off && i < a.vec[e].off + HID) mine = false;
  if (mine) {
    const long off = net * a.g_ns + i;
    float4 w = f4(0.f), m = f4(0.f), v = f4(0.f), tt = f4(0.f);
    if (a.apply) { w = ld4(a.P + off); m = ld4(a.Mo + off); v = ld4(a.Vo + off); if (a.T) tt = ld4(a.T + off); }
    float4 gs[8];
#pragma unroll
    for (int sl = 0; sl < 8; ++sl) gs[sl] = ld4(a.Gp + ((long)min(sl, a.S - 1) * a.nets + net) * a.g_ns + i);   // all requests first
    float4 g = gs[0];
#pragma unroll
    for (int sl = 1; sl < 8; ++sl) if (sl < a.S) g = g + gs[sl];
    adam_red_commit<KEEP_G>(a, off, g, w, m, v, tt, step, sq2);
  }
}
