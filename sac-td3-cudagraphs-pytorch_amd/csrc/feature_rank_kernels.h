// Device code of the feature-rank call (include/sactd3_feature_rank.h): the spectrum of M = H2^T H2 / V, H2 the second hidden layer of
// an online net over V valid ring rows.  Included by dormant.hip behind dormant_kernels.h: k_dormant_compact (unchanged, on this call's
// own slot list), dm_pick and hidden_tile.h are used as they are, under dormant.hip's pragmas (contraction off, no packed fp32 instructions).
//
// k_frank_gram: grid (min(ceil(n / 16), 16), nets, 2), 256 threads, of which G = min(ceil(V / 16), 16) per (net, half) work.  Workgroup
//   (g, net, half) walks the 16-row tiles g, g + G, ... of the checked list.  Per tile: the ring front end, LayerNorm + ReLU and layer 2
//   of hidden_tile.h as k_dormant_scan calls them, rows behind V stored as zeros; then H2^T H2 of the tile for the Gram columns
//   128 half .. + 127 onto accumulators that stay in registers for the whole call: wave w owns the Gram rows 64 w .. + 63 as 4 x 8 tiles of 16 x 16 (128 accumulator registers per lane), each fed by four v_mfma_f32_16x16x4f32 whose k are the
//   tile's four row quads -- lane (r, kq) reads H2[4 kq + m][i0 + r] and H2[4 kq + m][j0 + r] for the m-th of them; with the row stride of
//   260 floats the 64 lanes of such a read touch 64 different LDS banks.  Both halves recompute the forward pass (about two thirds of a
//   tile's MACs): splitting the Gram's columns, not the rows, keeps the accumulators out of memory until the end and the partials at
//   G <= 16.  At the end a lane holds four consecutive rows of one column; the matrix is symmetric, so they are stored as four consecutive
//   columns of one row of part[net][g] (plain 16-byte stores): the partial is the transpose of what was accumulated, the same matrix.
// k_frank_eig: grid (nets), 1024 threads, one workgroup holds the whole problem in LDS.
//   load: A[i][j] = (sum_g part[g][i][j]) / V for i <= j, g ascending, into a packed upper triangle (256 * 257 / 2 floats: a full image
//     would not fit beside the rest); the optional `gram` output here, mirrored; the trace from the diagonal through one 256-wide tree.
//   solve: parallel cyclic two-sided Jacobi, round-robin order: a sweep is 255 rounds of 128 disjoint pairs; in round t pair 0 is
//     (255, t), pair k is ((t + k) mod 255, (t - k) mod 255).  A round is two phases between block barriers.  (a) thread k < 128:
//     theta = (a_qq - a_pp) / (2 a_pq), t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c, tau = s / (1 + c);
//     (s, tau, t) into LDS; a pair with a_pq == 0, |a_pq| <= u sqrt(|a_pp a_qq|) or |a_pq| <= 2^-30 trace (u / 64 of the
//     trace: it moves no eigenvalue by a rounding of lambda_1, and rank-deficient inputs stop sweeping over their noise) gets the identity
//     and is no rotation.  (b) the 128 * 129 / 2 pair blocks (a <= b)
//     are dealt over the threads (a thread's blocks are the same in every round: decoded once): an off-diagonal block reads its four
//     elements, applies R_a^T B R_b, R = [[c, s], [-s, c]] in Rutishauser's form (x - s (y + tau x), y + s (x - tau y)), and writes them back; a diagonal block writes a_pp - t a_pq, a_qq + t a_pq
//     -- each as a two-sum whose remainder goes to lo[256], since the 255 updates a sweep of a diagonal element are the first-order error
//     of its eigenvalue (30 - 100 u of lambda_1 without the remainders, a few u with them) -- and an exact 0.  No two blocks share an element.  The loop ends behind the first sweep without a rotation or behind FR_SWEEPS sweeps
//     (converged = 0, counted); each sweep counts its rotations in an LDS word of its own, so the decision is block-uniform.
//   tail: the diagonal plus lo, clamped at 0, sorted descending by counting (ties by index); sigma_i = sqrt(lambda_i) where lambda_i > floor *
//     lambda_1; the sums (compensated, ascending i) and the summary by one thread in one fixed order.
#pragma once
#include "feature_rank.h"

#define FR_TRI (HT_HID * (HT_HID + 1) / 2)      // floats of the packed upper triangle
#define FR_PAIRS (HT_HID / 2)
#define FR_BLOCKS (FR_PAIRS * (FR_PAIRS + 1) / 2)
#define FR_THREADS 1024
#define FR_PER ((FR_BLOCKS + FR_THREADS - 1) / FR_THREADS)
#define FR_U 5.9604644775390625e-8f             // 2^-24, the unit roundoff of fp32
#define FR_TINY 9.31322574615478515625e-10f     // 2^-30: an off-diagonal element at or below this share of the trace is left alone

__global__ __launch_bounds__(256) void k_frank_gram(FrankArgs q) {
  __shared__ __attribute__((aligned(16))) float Xs[HT_TILE * HT_XS];
  __shared__ __attribute__((aligned(16))) float H1[HT_TILE * HT_AS];
  __shared__ __attribute__((aligned(16))) float H2[HT_TILE * HT_AS];
  __shared__ __attribute__((aligned(16))) float Ln[4 * HT_HID];      // g1, be1, g2, be2
  const DormantScanArgs& p = q.scan;
  const int tid = threadIdx.x, row = tid >> 4, sub = tid & 15;
  const int lane = tid & 63, wave = tid >> 6, r = lane & 15, kq = lane >> 4, half = blockIdx.z;
  if ((int)blockIdx.y >= p.nnets || half > 1) return;
  const NetView N = dm_pick(p.net, blockIdx.y);
  const int V = min(max(p.st.rows[0], 0), p.n);      // k_dormant_compact's, one launch ahead on this stream
  const int g = blockIdx.x, ntiles = (V + HT_TILE - 1) / HT_TILE, G = min(ntiles, FR_MAXG);
  if (g >= G) return;                                // (block-uniform; k_frank_eig reads the partials of [0, G) alone)

  float b1c[4], b2c[4];
  ht_ring_load(N, tid, Ln, b1c, b2c);
  ht_f32x4 gr[4][8];      // Gram rows 64 wave + 16 ti + 4 kq + m, column 128 half + 16 tj + r
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < 8; ++tj) gr[ti][tj] = ht_f32x4{0.f, 0.f, 0.f, 0.f};

  for (int tile = g; tile < ntiles; tile += G) {
    const bool ok = ht_ring_layer1(N, p.ring, p.rec_f, p.len, p.st.slots, V, tile, Xs, H1, b1c, tid);
    __syncthreads();
    ht_ln_relu_lds(H1 + row * HT_AS, Ln, Ln + HT_HID, sub, p.ln);
    __syncthreads();
    ht_layer2(H1, N.P + N.W2, b2c, H2, wave, r, kq);
    __syncthreads();
    ht_ln_relu_lds(H2 + row * HT_AS, Ln + 2 * HT_HID, Ln + 3 * HT_HID, sub, p.ln);
    if (!ok) {      // a row behind V adds nothing to the Gram matrix (the 16 elements this thread has just written)
#pragma unroll
      for (int c = 0; c < 4; ++c) *(float4*)(H2 + row * HT_AS + 4 * sub + 64 * c) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    // 6. gr += H2^T H2 of this tile: the m-th MFMA of a 16 x 16 tile takes the rows 4 kq + m
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const float* __restrict__ h = H2 + (4 * kq + m) * HT_AS + r;
      float a[4], b[8];
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) a[ti] = h[wave * 64 + ti * 16];
#pragma unroll
      for (int tj = 0; tj < 8; ++tj) b[tj] = h[half * 128 + tj * 16];
#pragma unroll
      for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 8; ++tj) gr[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ti], b[tj], gr[ti][tj], 0, 0, 0);
    }
    __syncthreads();      // H2 is written again by the next tile
  }

  float* __restrict__ out = q.st.part + ((size_t)N.id * FR_MAXG + g) * (size_t)(HT_HID * HT_HID);
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < 8; ++tj)
      *(float4*)(out + (size_t)(half * 128 + tj * 16 + r) * HT_HID + wave * 64 + ti * 16 + 4 * kq) =
          make_float4(gr[ti][tj][0], gr[ti][tj][1], gr[ti][tj][2], gr[ti][tj][3]);
}

// where element (i, j), i <= j, lies in the packed upper triangle
__device__ __forceinline__ int fr_at(int i, int j) { return ((i * (2 * HT_HID - 1 - i)) >> 1) + j; }
__device__ __forceinline__ int fr_sym(int x, int y) { return x <= y ? fr_at(x, y) : fr_at(y, x); }
// pair k of round t of the round-robin order
__device__ __forceinline__ void fr_pair(int t, int k, int& p, int& q) {
  const int u = t + k, d = t - k;
  p = k == 0 ? HT_HID - 1 : (u >= HT_HID - 1 ? u - (HT_HID - 1) : u);
  q = d < 0 ? d + (HT_HID - 1) : d;
}

__global__ __launch_bounds__(FR_THREADS) void k_frank_eig(FrankArgs q) {
  __shared__ float A[FR_TRI];
  __shared__ __attribute__((aligned(16))) float4 rot[FR_PAIRS];      // (s, tau, t, -) of the round's pairs; the tail's scratch behind the solver
  __shared__ float lam[HT_HID], sor[HT_HID];
  __shared__ float lo[HT_HID];      // what the updates of diagonal element i rounded away: lambda_i = A_ii + lo_i
  __shared__ int rotated[FR_SWEEPS];
  __shared__ float scal[2];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= q.scan.nnets) return;
  const int id = dm_pick(q.scan.net, blockIdx.x).id;
  const int V = min(max(q.scan.st.rows[0], 0), q.scan.n), R = q.scan.st.rows[1];
  const int tiles = (V + HT_TILE - 1) / HT_TILE, G = tiles < FR_MAXG ? tiles : FR_MAXG;

  // ---- load
  {
    const float* __restrict__ part = q.st.part + (size_t)id * FR_MAXG * (size_t)(HT_HID * HT_HID);
    float* __restrict__ gram = q.gram ? q.gram + (size_t)id * (HT_HID * HT_HID) : nullptr;
    for (int e = tid; e < HT_HID * HT_HID; e += FR_THREADS) {
      const int i = e >> 8, j = e & (HT_HID - 1);
      if (i > j) continue;
      float s = 0.f;
      for (int g = 0; g < G; ++g) s += part[(size_t)g * (HT_HID * HT_HID) + e];
      const float m = V > 0 ? s / (float)V : 0.f;
      A[fr_at(i, j)] = m;
      if (gram) { gram[i * HT_HID + j] = m; gram[j * HT_HID + i] = m; }
    }
    if (tid < FR_SWEEPS) rotated[tid] = 0;
    if (tid < HT_HID) lo[tid] = 0.f;
  }
  __syncthreads();
  if (tid < HT_HID) lam[tid] = A[fr_at(tid, tid)];
  __syncthreads();
  for (int w = HT_HID / 2; w >= 1; w >>= 1) {
    if (tid < w) lam[tid] = lam[tid] + lam[tid + w];
    __syncthreads();
  }
  const float trace = lam[0];
  const float tiny = FR_TINY * fabsf(trace);

  // ---- solve
  int ab[FR_PER];      // this thread's pair blocks, a | b << 8 (constant indices: registers)
#pragma unroll
  for (int it = 0; it < FR_PER; ++it) {
    const int e = tid + FR_THREADS * it, y = e / (FR_PAIRS + 1), x = e - y * (FR_PAIRS + 1);      // rows y and 127 - y of the triangle fill 129 places
    const int a = x < FR_PAIRS - y ? y : FR_PAIRS - 1 - y, b = x < FR_PAIRS - y ? y + x : x - 1;   // (x - (128 - y) + 127 - y)
    ab[it] = e < FR_BLOCKS ? (a | (b << 8)) : -1;
  }
  int sweeps = 0, converged = 1;
  if (V > 0) {      // (block-uniform)
    converged = 0;
    for (int sweep = 0; sweep < FR_SWEEPS && !converged; ++sweep) {
      for (int t = 0; t < HT_HID - 1; ++t) {
        if (tid < FR_PAIRS) {
          int pp, qq;
          fr_pair(t, tid, pp, qq);
          const float app = A[fr_at(pp, pp)], aqq = A[fr_at(qq, qq)], apq = A[fr_sym(pp, qq)];
          float s = 0.f, tau = 0.f, tn = 0.f;
          if (!(apq == 0.f || fabsf(apq) <= tiny || fabsf(apq) <= FR_U * sqrtf(fabsf(app * aqq)))) {
            const float th = (aqq - app) / (2.f * apq);
            // (behind 1e18 theta^2 would overflow: there sqrt(theta^2 + 1) is |theta| to the last bit)
            tn = fabsf(th) < 1e18f ? copysignf(1.f, th) / (fabsf(th) + sqrtf(th * th + 1.f)) : 0.5f / th;
            if (tn != 0.f) {         // (an angle that underflows to 0 is the identity as well)
              const float c = 1.f / sqrtf(tn * tn + 1.f);
              s = tn * c;
              tau = s / (1.f + c);
              rotated[sweep] = 1;    // (every writer stores the same word)
            }
          }
          rot[tid] = make_float4(s, tau, tn, 0.f);
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < FR_PER; ++it) {
          if (ab[it] < 0) continue;
          const int a = ab[it] & 255, b = ab[it] >> 8;
          const float4 ra = rot[a], rb = rot[b];
          if (ra.z == 0.f && rb.z == 0.f) continue;      // two identities: the block stays as it is
          int pa, qa, pb, qb;
          fr_pair(t, a, pa, qa);
          fr_pair(t, b, pb, qb);
          if (a == b) {
            const int ip = fr_at(pa, pa), iq = fr_at(qa, qa), ix = fr_sym(pa, qa);
            const float apq = A[ix], app = A[ip], aqq = A[iq];
            // d + dl = t a_pq exactly; a_pp - d and a_qq + d as two-sums: the diagonal is touched 255 times a sweep, and its roundings
            // are the first-order error of the eigenvalues (nothing here is contracted or reassociated)
            const float d = ra.z * apq, dl = fmaf(ra.z, apq, -d);
            const float np = app - d, bp = np - app, ep = (app - (np - bp)) + (-d - bp);
            const float nq = aqq + d, bq = nq - aqq, eq = (aqq - (nq - bq)) + (d - bq);
            A[ip] = np; lo[pa] += ep - dl;
            A[iq] = nq; lo[qa] += eq + dl;
            A[ix] = 0.f;
          } else {
            const int i00 = fr_sym(pa, pb), i01 = fr_sym(pa, qb), i10 = fr_sym(qa, pb), i11 = fr_sym(qa, qb);
            const float b00 = A[i00], b01 = A[i01], b10 = A[i10], b11 = A[i11];
            // x' = c x - s y as x - s (y + tau x), y' = s x + c y as y + s (x - tau y): c = 1 - s tau, and a small angle rounds a small term
            const float t00 = b00 - ra.x * (b10 + ra.y * b00), t01 = b01 - ra.x * (b11 + ra.y * b01);
            const float t10 = b10 + ra.x * (b00 - ra.y * b10), t11 = b11 + ra.x * (b01 - ra.y * b11);
            A[i00] = t00 - rb.x * (t01 + rb.y * t00);
            A[i01] = t01 + rb.x * (t00 - rb.y * t01);
            A[i10] = t10 - rb.x * (t11 + rb.y * t10);
            A[i11] = t11 + rb.x * (t10 - rb.y * t11);
          }
        }
        __syncthreads();
      }
      ++sweeps;
      converged = rotated[sweep] == 0 ? 1 : 0;      // (written before the sweep's last barrier, never behind it)
    }
  }

  // ---- tail
  __syncthreads();      // (with V == 0 no barrier of the solver stands between the trace's read of lam[0] and the stores below)
  float* __restrict__ sig = lam;              // sigma_i in place of the clamped diagonal, once that is sorted
  float* __restrict__ ent = (float*)rot;      // p_i ln p_i
  if (tid < HT_HID) lam[tid] = fmaxf(A[fr_at(tid, tid)] + lo[tid], 0.f);
  __syncthreads();
  if (tid < HT_HID) {
    const float v = lam[tid];
    int before = 0;
    for (int j = 0; j < HT_HID; ++j) {
      const float w = lam[j];
      before += (w > v || (w == v && j < tid)) ? 1 : 0;
    }
    sor[before & (HT_HID - 1)] = v;      // (a permutation of 0 .. 255 for any values that compare; the mask keeps a NaN's store inside)
  }
  __syncthreads();
  const float lam1 = sor[0];
  if (tid < HT_HID) {
    const float v = sor[tid];
    q.st.lambda[id * HT_HID + tid] = v;
    if (q.spectrum) q.spectrum[id * HT_HID + tid] = v;
    sig[tid] = (lam1 > 0.f && v > q.floor * lam1) ? sqrtf(v) : 0.f;
  }
  __syncthreads();
  if (tid == 0) {
    float s = 0.f, cs = 0.f, l = 0.f, cl = 0.f;
    for (int i = 0; i < HT_HID; ++i) { ht_kahan(s, cs, sig[i]); ht_kahan(l, cl, sor[i]); }
    scal[0] = s; scal[1] = l;
  }
  __syncthreads();
  const float S = scal[0], lsum = scal[1];
  if (tid < HT_HID) {
    const float pr = S > 0.f ? sig[tid] / S : 0.f;
    ent[tid] = pr > 0.f ? pr * logf(pr) : 0.f;
  }
  __syncthreads();
  if (tid == 0) {
    float h = 0.f, ch = 0.f, run = 0.f, cr = 0.f;
    const float need = (1.0f - q.delta) * S;
    int rank = 0, srank = 0;
    for (int i = 0; i < HT_HID; ++i) {
      ht_kahan(h, ch, ent[i]);
      if (sig[i] > 0.f) ++rank;
      if (S > 0.f && srank == 0) {
        ht_kahan(run, cr, sig[i]);
        if (run >= need) srank = i + 1;
      }
    }
    if (S > 0.f && srank == 0) srank = rank;      // (not reached with finite values: the last prefix is S itself)
    float* __restrict__ sm = q.st.summary + id * FR_SUMMARY;
    sm[0] = trace; sm[1] = lsum; sm[2] = (float)rank; sm[3] = (float)srank;
    sm[4] = S > 0.f ? expf(-h) : 0.f;
    sm[5] = lam1 > 0.f ? lsum / lam1 : 0.f;
    sm[6] = (float)sweeps; sm[7] = (float)converged;
    q.st.words[FR_W_RANK + id] = rank;
    q.st.words[FR_W_SRANK + id] = srank;
    q.st.words[FR_W_SWEEPS + id] = sweeps;
    if (!converged) q.st.words[FR_W_UNCONVERGED + id] += 1;
    if (blockIdx.x == 0) {      // one thread of the launch: the rows are the same for every net
      q.st.words[FR_W_VALID] = V;
      q.st.words[FR_W_REFUSED] += R;
    }
  }
}
