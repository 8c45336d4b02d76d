// The body of k_prio_update and k_prio_update_g (prio_kernels.h), included as text: it leaves early for a refused row, and as a function
// inlined into both kernels it would not leave k_prio_update its machine code.  `p`: the PrioUpdateArgs in force.
  __shared__ unsigned long long own[PRIO_G];
  __shared__ float ws[4];
  const int tid = threadIdx.x, b = blockIdx.x;
  int slot_b; float pr_b;
  const bool ok_b = prio_row(p, b, slot_b, pr_b);
  if (!ok_b) {                        // (block-uniform)
    if (tid == 0) atomicAdd(&p.pc->refused, 1);
    return;
  }
  const int g = slot_b / PRIO_G;
  const float4 v = reinterpret_cast<const float4*>(p.leaf)[(long)g * 256 + tid];
#pragma unroll
  for (int k = 0; k < 4; ++k) own[4 * tid + k] = 0ull;
  __syncthreads();
  for (int j = tid; j < p.n; j += 256) {
    int s; float pr;
    const bool ok = prio_row(p, j, s, pr);
    if (ok && s / PRIO_G == g)
      atomicMax(&own[s % PRIO_G], ((unsigned long long)(unsigned)(j + 1) << 32) | (unsigned long long)__float_as_uint(prio_leaf_value(pr, p.alpha)));
  }
  __syncthreads();
  float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned long long o = own[4 * tid + k];
    if (o) vv[k] = __uint_as_float((unsigned)o);
  }
  float tot;
  prio_scan(make_float4(vv[0], vv[1], vv[2], vv[3]), ws, tot);
  if (tid == 0) {
    st1_wt(p.sums + g, tot);
    const unsigned long long o = own[slot_b % PRIO_G];
    if ((unsigned)(o >> 32) == (unsigned)(b + 1)) st1_wt(p.leaf + slot_b, __uint_as_float((unsigned)o));
    atomicMax(reinterpret_cast<int*>(&p.pc->max_prio), __float_as_int(pr_b));
  }
