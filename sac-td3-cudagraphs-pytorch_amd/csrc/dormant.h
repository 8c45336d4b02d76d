// What engine.hip knows of the dormant-neuron scan and the ReDo recycler (dormant.hip, dormant_kernels.h; include/sactd3_dormant.h is
// their C ABI): the argument structs and one host launcher per kernel.  Nothing else crosses between the two translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "net_view.h"

#define DM_NETS 3          // 0: the actor; 1, 2: the critics.  Pair (net, layer) = 2 net + layer, layer 0 / 1 = the two hidden layers
#define DM_PAIRS 6
#define DM_MAXG 128        // workgroups per net: min(ceil(n / 16), 128) are launched, G = min(ceil(V / 16), 128) of them work (V: the valid rows)
#define DM_MAXN 65536      // rows of one scan
// device words of the feature (DormantState::words)
enum { DM_W_COUNT = 0 /* .. 5: dormant neurons per pair, last scan */, DM_W_VALID = 6, DM_W_REFUSED = 7, DM_W_RECYCLED = 8, DM_W_LEFT_ZERO = 9, DM_WORDS = 16 };

// The feature's own device memory, made at its first scan.
struct DormantState {
  float* part;       // [DM_NETS][2][DM_MAXG][256] column sums of a workgroup's tiles
  int* slots;        // [DM_MAXN] the checked slots of the last scan, in the order of idx: what the tiles are cut from
  int* rows;         // {V = valid rows, refused rows} of the last scan
  float* scores;     // [DM_PAIRS][256]
  uint8_t* mask;     // [DM_PAIRS][256] 1: dormant at the last scan's tau
  int* words;        // [DM_WORDS]
};
struct DormantScanArgs {
  const float* ring; int rec_f; int len;        // record r at ring + r * rec_f; slots are checked against [0, len)
  const long long* idx; long idx_ld; int n;     // slot of row r: idx[r * idx_ld]
  int ln;                                       // sactd3_config::layer_norm
  float tau;
  NetView net[DM_NETS]; int nnets;           // the scanned nets, in ascending id
  DormantState st;
  float* out;                                   // NULL, or the caller's [DM_PAIRS][256]: rows of the scanned nets are written
};
struct RedoArgs {
  NetView net[DM_NETS]; int nnets;
  DormantState st;
  unsigned long long seed; unsigned epoch;      // the Philox key and the first counter word
};

static inline int dormant_groups(int n) { const int t = (n + HT_TILE - 1) / HT_TILE; return t < DM_MAXG ? t : DM_MAXG; }

// hipErrorInvalidValue, and nothing is launched, where an argument is outside what the kernels' address arithmetic holds; otherwise
// hipGetLastError() behind the launch.  dormant_scan_launch issues k_dormant_compact, k_dormant_scan and k_dormant_finish.
hipError_t dormant_scan_launch(const DormantScanArgs& args, hipStream_t stream);
hipError_t dormant_redo_launch(const RedoArgs& args, hipStream_t stream);
