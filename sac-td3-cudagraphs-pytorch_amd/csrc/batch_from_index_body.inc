// The body of k_batch_from_index (kernels.h) and k_batch_from_index_g (nstep_kernels.h), included as text (see prio_update_body.inc).
// `p`: the IndexBatchArgs in force.
  __shared__ long long ids_s[GATHER_CPT * 256 + 2];
  __shared__ float w_s[GATHER_CPT * 256 + 2];
  const unsigned total = (unsigned)p.B * (unsigned)p.rec4;
  const unsigned c0 = blockIdx.x * (unsigned)p.cpb * 256u;
  if (c0 >= total) return;                                             // (block-uniform)
  const unsigned c1 = min(c0 + (unsigned)p.cpb * 256u, total);
  const unsigned r0 = fast_div(c0, (unsigned)p.rec4, p.rec4_magic), r1 = fast_div(c1 - 1u, (unsigned)p.rec4, p.rec4_magic);
  // both requests of a row go out before the first LDS store: one round trip, not two.  (w == NULL: the weight load reads the first
  // word of the index array instead -- an address that is always valid -- and a select drops the value.)
  const float* const wsrc = p.w ? p.w : reinterpret_cast<const float*>(p.idx);
  const long wld = p.w ? p.w_ld : 0;
  for (unsigned i = threadIdx.x; i <= r1 - r0; i += 256u) {
    long long id = p.idx[(long)(r0 + i) * p.idx_ld];
    float wi = wsrc[(long)(r0 + i) * wld];
    PIN(wi);
    ids_s[i] = id;
    w_s[i] = p.w ? wi : 1.f;
  }
  __syncthreads();
  int bb[GATHER_CPT], cc[GATHER_CPT], slot[GATHER_CPT]; float wv[GATHER_CPT]; float4 v[GATHER_CPT]; bool on[GATHER_CPT], ok[GATHER_CPT], first[GATHER_CPT];
#pragma unroll
  for (int u = 0; u < GATHER_CPT; ++u) {            // consecutive threads -> consecutive chunks of a record
    const unsigned g = c0 + (unsigned)u * 256u + threadIdx.x;
    on[u] = u < p.cpb && g < c1;
    const unsigned q = on[u] ? fast_div(g, (unsigned)p.rec4, p.rec4_magic) : r0;
    bb[u] = (int)q; cc[u] = on[u] ? (int)(g - q * (unsigned)p.rec4) : 0;
    const long long raw = ids_s[q - r0];
    wv[u] = w_s[q - r0];
    ok[u] = raw >= 0 && raw < (long long)p.len;
    slot[u] = ok[u] ? (int)raw : 0;
    first[u] = on[u] && cc[u] == 0;
    on[u] = on[u] && cc[u] <= p.cx + p.cn;           // trailing pad chunk(s) are not moved
  }
#pragma unroll
  for (int u = 0; u < GATHER_CPT; ++u) v[u] = p.ring[(long)slot[u] * p.rec4 + (on[u] ? cc[u] : 0)];
#pragma unroll
  for (int u = 0; u < GATHER_CPT; ++u) { PIN(v[u].x); PIN(v[u].y); PIN(v[u].z); PIN(v[u].w); }      // every request is out before the first store
#pragma unroll
  for (int u = 0; u < GATHER_CPT; ++u) {
    const int b = bb[u], c = cc[u];
    if (first[u]) {
      const bool wok = weight_ok(wv[u]);
      p.slot_idx[b] = ok[u] ? slot[u] : -1;
      p.wdst[b] = (ok[u] && wok) ? wv[u] : 0.f;
      if (!ok[u] || !wok) atomicAdd(p.refused, 1);
    }
    if (!on[u]) continue;
    const float4 o4 = ok[u] ? v[u] : make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < p.cx) p.X[(long)b * p.cx + c] = o4;
    else if (c < p.cx + p.cn) p.Xn[(long)b * p.cx + (c - p.cx)] = o4;
    else { p.rew[b] = o4.x; p.done[b] = o4.y; }
  }
