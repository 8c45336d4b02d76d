// The body of k_batch_from_index_nstep and k_batch_from_index_nstep_g (nstep_kernels.h), included as text (see prio_update_body.inc).
// `p`: the NstepArgs in force.
  __shared__ int s0_s[NS_ROWS];           // slot_0 (0 for a refused row)
  __shared__ int avail_s[NS_ROWS];        // chain slots that exist, <= steps (0: the row is refused)
  __shared__ float w_s[NS_ROWS];
  __shared__ unsigned brk_s[NS_ROWS];     // bit j: link j -> j+1 is broken
  __shared__ float r_s[NS_ROWS][NS_MAX], d_s[NS_ROWS][NS_MAX];
  __shared__ int k_s[NS_ROWS], last_s[NS_ROWS];
  __shared__ float R_s[NS_ROWS], m_s[NS_ROWS];
  const unsigned total = (unsigned)p.B * (unsigned)p.rec4;
  const unsigned c0 = blockIdx.x * (unsigned)p.cpb * 256u;
  if (c0 >= total) return;                                             // (block-uniform)
  const unsigned c1 = min(c0 + (unsigned)p.cpb * 256u, total);
  const unsigned r0 = fast_div(c0, (unsigned)p.rec4, p.rec4_magic), r1 = fast_div(c1 - 1u, (unsigned)p.rec4, p.rec4_magic);
  const int nrows = (int)(r1 - r0) + 1;
  if (nrows > NS_ROWS) return;                                         // (block-uniform; the host never launches such a span)

  // ---- phase 0: the rows' start slots and weights, once, into LDS (k_batch_from_index's two requests per row)
  {
    const bool draw = p.idx == nullptr;
    const unsigned long long seed = p.ctl->seed;
    const int ctr = p.ctl->sample_ctr;
    const long long* const isrc = draw ? reinterpret_cast<const long long*>(p.ctl) : p.idx;      // (a draw: an always-valid address, value dropped)
    const long ild = draw ? 0 : p.idx_ld;
    const float* const wsrc = p.w ? p.w : reinterpret_cast<const float*>(p.ctl);
    const long wld = p.w ? p.w_ld : 0;
    for (int i = threadIdx.x; i < nrows; i += 256) {
      long long id = isrc[(long)(r0 + i) * ild];
      float wi = wsrc[(long)(r0 + i) * wld];
      PIN(wi);
      if (draw) id = (long long)philox_index(seed, (unsigned)ctr, r0 + i, (unsigned)p.len);
      const bool ok = id >= 0 && id < (long long)p.len;
      const int s0 = ok ? (int)id : 0;
      const int age = p.len < p.cap ? s0 : (s0 >= p.cursor ? s0 - p.cursor : s0 - p.cursor + p.cap);
      // slots that exist: j with age + j * stride < len, i.e. j <= (len - 1 - age) / stride (age < len for an accepted row)
      const int avail = ok ? min(p.steps, (p.len - 1 - age) / p.stride + 1) : 0;
      s0_s[i] = s0; avail_s[i] = avail; w_s[i] = p.w ? wi : 1.f;
      brk_s[i] = avail > 0 ? ~0u << (avail - 1) : ~0u;                  // a link into a slot that does not exist is broken
    }
  }
  __syncthreads();

  // ---- phase 1: the links.  Per row (steps - 1) * co compare items (link j, chunk c < co) and `steps` [r, d] items.
  {
    const int co = (p.o + 3) >> 2, ncmp = (p.steps - 1) * co, ipr = ncmp + p.steps;
    const int items = nrows * ipr;
    for (int base = threadIdx.x; base < items; base += 256 * NS_U) {
      int row[NS_U], jj[NS_U], ch[NS_U]; bool on[NS_U], cmp[NS_U]; float4 a[NS_U], b[NS_U];
#pragma unroll
      for (int u = 0; u < NS_U; ++u) {
        const int it = base + u * 256;
        const bool in = it < items;
        const int q = in ? it / ipr : 0, rem = in ? it - q * ipr : ncmp;
        row[u] = q; cmp[u] = rem < ncmp;
        jj[u] = cmp[u] ? rem / co : rem - ncmp;
        ch[u] = cmp[u] ? rem - jj[u] * co : 0;
        const int s0 = s0_s[q], avail = avail_s[q];
        // compare: s' chunk of slot_j against s chunk of slot_{j+1} (both exist iff j + 1 < avail); [r, d]: slot_j (exists iff j < avail)
        on[u] = in && (cmp[u] ? jj[u] + 1 < avail : jj[u] < avail);
        const int sa = on[u] ? nstep_slot(s0, jj[u], p.stride, p.cap) : s0;
        const int sb = on[u] && cmp[u] ? nstep_slot(s0, jj[u] + 1, p.stride, p.cap) : s0;
        a[u] = p.ring[(long)sa * p.rec4 + (cmp[u] ? p.cx + ch[u] : p.cx + p.cn)];
        b[u] = p.ring[(long)sb * p.rec4 + ch[u]];
      }
#pragma unroll
      for (int u = 0; u < NS_U; ++u) { PIN(a[u].x); PIN(a[u].y); PIN(a[u].z); PIN(a[u].w); PIN(b[u].x); PIN(b[u].y); PIN(b[u].z); PIN(b[u].w); }
#pragma unroll
      for (int u = 0; u < NS_U; ++u) {
        if (!on[u]) continue;
        if (cmp[u]) {
          if (nstep_differs(a[u], b[u], ch[u], p.o)) atomicOr(&brk_s[row[u]], 1u << jj[u]);
        } else {
          r_s[row[u]][jj[u]] = a[u].x; d_s[row[u]][jj[u]] = a[u].y;
          if (!(a[u].y == 0.f)) atomicOr(&brk_s[row[u]], 1u << jj[u]);
        }
      }
    }
  }
  __syncthreads();

  // ---- phase 2: one thread per row derives k, R and the mask, in the fixed order
  for (int i = threadIdx.x; i < nrows; i += 256) {
    const int avail = avail_s[i];
    int k = 0, last = -1; float R = 0.f, m = 0.f;
    if (avail > 0) {
      k = __builtin_ctz(brk_s[i] | (1u << (p.steps - 1))) + 1;          // (<= avail: the bits from avail - 1 up are set)
      nstep_return(r_s[i], d_s[i][k - 1], k, p.gamma, R, m);
      last = nstep_slot(s0_s[i], k - 1, p.stride, p.cap);
    }
    k_s[i] = k; last_s[i] = last; R_s[i] = R; m_s[i] = m;
  }
  __syncthreads();

  // ---- phase 3: k_batch_from_index's copy, with Xn taken from slot_{k-1}
  int bb[GATHER_CPT], cc[GATHER_CPT], li[GATHER_CPT]; float4 v[GATHER_CPT]; bool on[GATHER_CPT], ok[GATHER_CPT], first[GATHER_CPT];
#pragma unroll
  for (int u = 0; u < GATHER_CPT; ++u) {            // consecutive threads -> consecutive chunks of a record
    const unsigned g = c0 + (unsigned)u * 256u + threadIdx.x;
    on[u] = u < p.cpb && g < c1;
    const unsigned q = on[u] ? fast_div(g, (unsigned)p.rec4, p.rec4_magic) : r0;
    bb[u] = (int)q; cc[u] = on[u] ? (int)(g - q * (unsigned)p.rec4) : 0;
    li[u] = (int)(q - r0);
    ok[u] = avail_s[li[u]] > 0;
    first[u] = on[u] && cc[u] == 0;
    on[u] = on[u] && cc[u] <= p.cx + p.cn;           // trailing pad chunk(s) are not moved
    const bool nx = on[u] && cc[u] >= p.cx && cc[u] < p.cx + p.cn;
    const int slot = nx && ok[u] ? last_s[li[u]] : s0_s[li[u]];
    v[u] = p.ring[(long)slot * p.rec4 + (on[u] ? cc[u] : 0)];
  }
#pragma unroll
  for (int u = 0; u < GATHER_CPT; ++u) { PIN(v[u].x); PIN(v[u].y); PIN(v[u].z); PIN(v[u].w); }      // every request is out before the first store
#pragma unroll
  for (int u = 0; u < GATHER_CPT; ++u) {
    const int b = bb[u], c = cc[u], i = li[u];
    if (first[u]) {
      const float wv = w_s[i];
      const bool wok = weight_ok(wv);
      const int k = k_s[i];
      p.slot_idx[b] = ok[u] ? s0_s[i] : -1;
      if (p.wdst) p.wdst[b] = (ok[u] && wok) ? wv : 0.f;
      p.nk[b] = k; p.nlast[b] = last_s[i];
      if (!ok[u] || !wok) atomicAdd(p.counters + 1, 1);
      if (ok[u] && k < p.steps) atomicAdd(p.counters, 1);
    }
    if (!on[u]) continue;
    const float4 o4 = ok[u] ? v[u] : make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < p.cx) p.X[(long)b * p.cx + c] = o4;
    else if (c < p.cx + p.cn) p.Xn[(long)b * p.cx + (c - p.cx)] = o4;
    else { p.rew[b] = R_s[i]; p.done[b] = m_s[i]; }
  }
