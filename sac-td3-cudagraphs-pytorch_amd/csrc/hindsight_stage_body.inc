// The body of k_hindsight_stage and k_hindsight_stage_g (hindsight.hip), textually included into both: `p` is a HindsightArgs
// whose len, cursor and hctr are the host's (the call form) or were read from device memory and bounded at entry (the graph form).
// Both kernels switch contraction off in front of it.
  __shared__ int s0_s[HS_ROWS];             // slot_0 (0 for a refused row)
  __shared__ int avail_s[HS_ROWS];          // chain slots that exist, <= window (0: the row is refused)
  __shared__ unsigned brk_s[HS_ROWS][2];    // bit j: link j -> j+1 is broken
  __shared__ unsigned v0_s[HS_ROWS], v1_s[HS_ROWS];
  __shared__ int ch_s[HS_ROWS];             // the injected choice
  __shared__ int j_s[HS_ROWS], gs_s[HS_ROWS];      // the offset (-1: not relabelled), the goal's ring slot (-1)
  __shared__ float rew_s[HS_ROWS];
  __shared__ float g_s[HS_ROWS][HS_MAX_GOAL];
  const unsigned total = (unsigned)p.B * (unsigned)p.rec4;
  const unsigned c0 = blockIdx.x * (unsigned)p.cpb * 256u;
  if (c0 >= total) return;                                             // (block-uniform)
  const unsigned c1 = min(c0 + (unsigned)p.cpb * 256u, total);
  const unsigned r0 = hs_fast_div(c0, (unsigned)p.rec4, p.rec4_magic), r1 = hs_fast_div(c1 - 1u, (unsigned)p.rec4, p.rec4_magic);
  const int nrows = (int)(r1 - r0) + 1;
  if (nrows > HS_ROWS) return;                                         // (block-uniform; the launcher never launches such a span)

  // ---- phase 0: the rows' start slots, choices and draws, once, into LDS
  {
    const int* const csrc = p.choice ? p.choice : reinterpret_cast<const int*>(p.idx);      // (no choice: an always-valid address, value dropped)
    const long cld = p.choice ? p.choice_ld : 0;
    for (int i = threadIdx.x; i < nrows; i += 256) {
      const long long id = p.idx[(long)(r0 + i) * p.idx_ld];
      int ch = csrc[(long)(r0 + i) * cld];
      HS_PIN(ch);
      const Philox4 r = philox4x32_10(p.hctr, 0u, SACTD3_STREAM_HINDSIGHT, r0 + (unsigned)i, (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
      const bool ok = id >= 0 && id < (long long)p.len;
      const int s0 = ok ? (int)id : 0;
      const int age = p.len < p.cap ? s0 : (s0 >= p.cursor ? s0 - p.cursor : s0 - p.cursor + p.cap);
      // slots that exist: j with age + j * stride < len, i.e. j <= (len - 1 - age) / stride (age < len for an accepted row)
      const int avail = ok ? min(p.window, (p.len - 1 - age) / p.stride + 1) : 0;
      const unsigned long long brk = avail > 0 ? ~0ull << (avail - 1) : ~0ull;      // a link into a slot that does not exist is broken
      s0_s[i] = s0; avail_s[i] = avail; ch_s[i] = ch; v0_s[i] = r.v[0]; v1_s[i] = r.v[1];
      brk_s[i][0] = (unsigned)brk; brk_s[i][1] = (unsigned)(brk >> 32);
    }
  }
  __syncthreads();

  // ---- phase 1: the links.  Per row (window - 1) * co compare items (link j, chunk c < co) and window - 1 flag items (link j).
  {
    const int co = (p.o + 3) >> 2, nl = p.window - 1, ncmp = nl * co, ipr = ncmp + nl;
    const int items = nrows * ipr;
    for (int base = threadIdx.x; base < items; base += 256 * HS_U) {
      int row[HS_U], jj[HS_U], ch[HS_U]; bool on[HS_U], cmp[HS_U]; float4 a[HS_U], b[HS_U];
#pragma unroll
      for (int u = 0; u < HS_U; ++u) {
        const int it = base + u * 256;
        const bool in = it < items;
        const int q = in ? it / ipr : 0, rem = in ? it - q * ipr : ncmp;
        row[u] = q; cmp[u] = rem < ncmp;
        jj[u] = cmp[u] ? rem / co : rem - ncmp;
        ch[u] = cmp[u] ? rem - jj[u] * co : 0;
        const int s0 = s0_s[q], avail = avail_s[q];
        // both kinds of item concern link j, which can only hold where slot_{j+1} exists
        on[u] = in && jj[u] + 1 < avail;
        const int sa = on[u] ? hs_slot(s0, jj[u], p.stride, p.cap) : s0;
        const int sb = on[u] && cmp[u] ? hs_slot(s0, jj[u] + 1, p.stride, p.cap) : s0;
        a[u] = p.ring[(long)sa * p.rec4 + (cmp[u] ? p.cx + ch[u] : p.cx + p.cn)];
        b[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (cmp[u]) b[u] = p.ring[(long)sb * p.rec4 + ch[u]];      // (a flag item compares nothing: no second load)
      }
#pragma unroll
      for (int u = 0; u < HS_U; ++u) { HS_PIN(a[u].x); HS_PIN(a[u].y); HS_PIN(a[u].z); HS_PIN(a[u].w); HS_PIN(b[u].x); HS_PIN(b[u].y); HS_PIN(b[u].z); HS_PIN(b[u].w); }
#pragma unroll
      for (int u = 0; u < HS_U; ++u) {
        if (!on[u]) continue;
        const bool broken = cmp[u] ? hs_differs(a[u], b[u], ch[u], p.o) : !(a[u].y == 0.f);
        if (broken) atomicOr(&brk_s[row[u]][jj[u] >> 5], 1u << (jj[u] & 31));
      }
    }
  }
  __syncthreads();

  // ---- phase 2: one thread per row derives L, the offset and the goal, and the relabelled reward in the fixed order
  for (int i = threadIdx.x; i < nrows; i += 256) {
    const int avail = avail_s[i], s0 = s0_s[i];
    const unsigned long long brk = ((unsigned long long)brk_s[i][1] << 32 | brk_s[i][0]) | (1ull << (p.window - 1));
    const int L = __builtin_ctzll(brk) + 1;                              // (<= avail for an accepted row: the bits from avail - 1 up are set)
    const int chv = ch_s[i];
    const bool drawn = p.choice ? chv >= 0 : philox_u01(v0_s[i]) < p.ratio;
    const bool relabel = avail > 0 && drawn;
    const int jd = p.choice ? min(chv, L - 1) : (int)(((unsigned long long)v1_s[i] * (unsigned long long)L) >> 32);
    const int j = relabel ? jd : 0;
    const int gslot = hs_slot(s0, j, p.stride, p.cap);                   // (j < L <= avail: the slot exists; not relabelled: slot_0)
    const float* const own = reinterpret_cast<const float*>(p.ring + (long)s0 * p.rec4 + p.cx) + p.ag_off;
    const float* const fut = reinterpret_cast<const float*>(p.ring + (long)gslot * p.rec4 + p.cx) + p.ag_off;
    float ag[HS_MAX_GOAL], g[HS_MAX_GOAL];
#pragma unroll
    for (int c = 0; c < HS_MAX_GOAL; ++c) { const int cc = c < p.G ? c : 0; ag[c] = own[cc]; g[c] = fut[cc]; }
#pragma unroll
    for (int c = 0; c < HS_MAX_GOAL; ++c) { HS_PIN(ag[c]); HS_PIN(g[c]); }
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < HS_MAX_GOAL; ++c) {
      const float d = ag[c] - g[c];
      const float sq = d * d;
      acc = (c == 0) ? sq : (c < p.G ? acc + sq : acc);
      g_s[i][c] = g[c];
    }
    const float thr2 = p.thr * p.thr;
    rew_s[i] = (acc <= thr2) ? 0.f : -1.f;
    j_s[i] = relabel ? j : -1;
    gs_s[i] = relabel ? gslot : -1;
  }
  __syncthreads();

  // ---- phase 3: k_batch_from_index's copy, with the goal's floats selected in per element
  int bb[HS_CPT], cc[HS_CPT], li[HS_CPT]; float4 v[HS_CPT]; bool on[HS_CPT], ok[HS_CPT], first[HS_CPT];
#pragma unroll
  for (int u = 0; u < HS_CPT; ++u) {              // consecutive threads -> consecutive chunks of a record
    const unsigned g = c0 + (unsigned)u * 256u + threadIdx.x;
    on[u] = u < p.cpb && g < c1;
    const unsigned q = on[u] ? hs_fast_div(g, (unsigned)p.rec4, p.rec4_magic) : r0;
    bb[u] = (int)q; cc[u] = on[u] ? (int)(g - q * (unsigned)p.rec4) : 0;
    li[u] = (int)(q - r0);
    ok[u] = avail_s[li[u]] > 0;
    first[u] = on[u] && cc[u] == 0;
    on[u] = on[u] && cc[u] <= p.cx + p.cn;         // trailing pad chunk(s) are not moved
    v[u] = p.ring[(long)s0_s[li[u]] * p.rec4 + (on[u] ? cc[u] : 0)];
  }
#pragma unroll
  for (int u = 0; u < HS_CPT; ++u) { HS_PIN(v[u].x); HS_PIN(v[u].y); HS_PIN(v[u].z); HS_PIN(v[u].w); }      // every request is out before the first store
#pragma unroll
  for (int u = 0; u < HS_CPT; ++u) {
    const int b = bb[u], c = cc[u], i = li[u];
    const int j = j_s[i];
    const bool relabel = j >= 0;
    if (first[u]) {
      p.slot_idx[b] = ok[u] ? s0_s[i] : -1;
      p.offset[b] = j; p.goal_slot[b] = gs_s[i];
      if (!ok[u]) atomicAdd(p.counters + 1, 1);
      if (relabel) atomicAdd(p.counters, 1);
      if (relabel && rew_s[i] == 0.f) atomicAdd(p.counters + 2, 1);
    }
    if (!on[u]) continue;
    float4 o4 = ok[u] ? v[u] : make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < p.cx + p.cn) {
      const int e = 4 * (c < p.cx ? c : c - p.cx);      // the chunk's first float within [s|a] / within s'
      const float* const g = g_s[i];
      o4.x = hs_pick(o4.x, e + 0, relabel, p.dg_off, p.G, g);
      o4.y = hs_pick(o4.y, e + 1, relabel, p.dg_off, p.G, g);
      o4.z = hs_pick(o4.z, e + 2, relabel, p.dg_off, p.G, g);
      o4.w = hs_pick(o4.w, e + 3, relabel, p.dg_off, p.G, g);
      if (c < p.cx) p.X[(long)b * p.cx + c] = o4;
      else p.Xn[(long)b * p.cx + (c - p.cx)] = o4;
    } else {
      p.rew[b] = relabel ? rew_s[i] : o4.x; p.done[b] = o4.y;
    }
  }
