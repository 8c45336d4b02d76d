// What engine.hip knows of the feature-rank call (feature_rank_kernels.h, compiled in dormant.hip -- the plasticity-diagnostics unit;
// include/sactd3_feature_rank.h is its C ABI): the argument struct and the host launcher.  The call shares k_dormant_compact, the
// hidden tile (hidden_tile.h) and NetView (net_view.h) with the dormant scan and no device memory: a scan's state and this call's never meet.
#pragma once
#include "dormant.h"
#include "net_view.h"

#define FR_MAXG 16         // workgroups per (net, column half): min(ceil(n / 16), 16) are launched, G = min(ceil(V / 16), 16) of them work
#define FR_MAXN 4096       // rows of one call
#define FR_SWEEPS 16       // Jacobi sweeps at most
#define FR_SUMMARY 8       // floats per net: trace, lambda_sum, rank, srank, erank, stable, sweeps, converged
// device words of the feature (FrankState::words); the triples are per net (actor, Q1, Q2)
enum { FR_W_VALID = 0, FR_W_REFUSED = 1, FR_W_RANK = 2, FR_W_SRANK = 5, FR_W_SWEEPS = 8, FR_W_UNCONVERGED = 11, FR_WORDS = 16 };

// The feature's own device memory, made at its first call.
struct FrankState {
  float* part;       // [DM_NETS][FR_MAXG][256][256] a workgroup's share of H2^T H2, stored transposed (the matrix is symmetric)
  int* slots;        // [FR_MAXN] the checked slots of the last call, in the order of idx
  int* rows;         // {V = valid rows, refused rows} of the last call
  float* lambda;     // [DM_NETS][256] eigenvalues of the Gram matrix, descending
  float* summary;    // [DM_NETS][FR_SUMMARY]
  int* words;        // [FR_WORDS]
};
struct FrankArgs {
  DormantScanArgs scan;      // ring, idx, n, ln, nets as a dormant scan has them; st.slots / st.rows point at FrankState's, the rest of st is NULL
  FrankState st;
  float delta, floor;
  float* spectrum;           // NULL, or the caller's [DM_NETS][256]: rows of the named nets are written
  float* gram;               // NULL, or the caller's [DM_NETS][256][256]: the same
};

static inline int frank_groups(int n) { const int t = (n + HT_TILE - 1) / HT_TILE; return t < FR_MAXG ? t : FR_MAXG; }

// hipErrorInvalidValue, and nothing is launched, where an argument is outside what the kernels' address arithmetic holds; otherwise
// hipGetLastError() behind the launch.  Issues k_dormant_compact, k_frank_gram and k_frank_eig.
hipError_t feature_rank_launch(const FrankArgs& args, hipStream_t stream);
