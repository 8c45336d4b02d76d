// What engine.hip knows of the nearest-ring-rows call (ring_knn.hip, ring_knn_kernels.h; include/sactd3_ring_knn.h is its C ABI): the
// argument struct, the slice rule and one host launcher.  Nothing else crosses between the translation units.
#pragma once
#include <hip/hip_runtime.h>

#define KNN_QT 64            // queries of one workgroup: four 16-column MFMA tiles
#define KNN_MAXK 16          // neighbours per query at most (engine.hip asserts it against the C ABI's)
#define KNN_MAXD 416         // key width at most, a multiple of 16 (the same)
#define KNN_CHUNK 1024       // queries of one launch
#define KNN_MAXSLICES 256    // ring slices of one launch at most
#define KNN_SLAB ((size_t)KNN_MAXSLICES * KNN_CHUNK * KNN_MAXK)      // elements of each half (sel, slot) of the partial slab
// device words of the feature (k_knn_count)
enum { KNN_W_BADQ = 0 /* non-finite queries so far */, KNN_W_BADROWS /* non-finite ring keys skipped */, KNN_W_SHORT /* results with < k hits */, KNN_WORDS = 4 };
// per-query flags of one launch (k_knn_finish -> k_knn_count)
enum { KNN_F_BADQ = 1, KNN_F_SHORT = 2 };

struct KnnArgs {
  const float* ring; int rec_f;             // the ring and a record's floats (a multiple of 16: a record's key starts 64-byte aligned)
  int D, k;                                 // key width (the record's leading D floats); neighbours
  long first, last;                         // the clipped range [first, last), last - first >= 1
  int slice_rows, nslices;                  // knn_slices(last - first)
  int m;                                    // queries of this launch (<= KNN_CHUNK)
  int count_rows;                           // this launch counts the range's non-finite ring keys (the first of a call)
  const float *offset, *scale;              // [D] or NULL
  // the caller's arrays, already moved to query 0 of this launch
  const float* q; long q_ld;
  const long long* exclude; long exclude_ld;      // or NULL
  long long* index; long index_ld;                // outputs: NULL = not wanted
  float* dist2; long dist2_ld;
  // the feature's own memory
  float* part_sel; int* part_slot;          // [nslices][KNN_CHUNK][KNN_MAXK]: a slice's k best per query, by (sel, slot) ascending
  int* qflags;                              // [KNN_CHUNK] KNN_F_* per query of this launch
  int* bad;                                 // [KNN_MAXSLICES] non-finite ring keys per slice of this launch
  int* words;                               // [KNN_WORDS]
};

// THE slice rule (include/sactd3_ring_knn.h states it): a function of the range length alone
static inline void knn_slices(long len, int* slice_rows, int* nslices) {
  long s0 = (len + 63) / 64;
  s0 = s0 < 1 ? 1 : s0 > KNN_MAXSLICES ? KNN_MAXSLICES : s0;
  const long rows = ((len + s0 - 1) / s0 + 15) / 16 * 16;
  *slice_rows = (int)rows;
  *nslices = (int)((len + rows - 1) / rows);
}

// hipErrorInvalidValue, and nothing is launched, where an argument is outside what the kernels' address arithmetic holds; otherwise
// hipGetLastError() behind the launches: k_knn_scan<DP>, k_knn_finish, then the single-workgroup k_knn_count.
hipError_t ring_knn_launch(const KnnArgs& args, long rb_len, hipStream_t stream);
