// What does the cache policy of a kernel's LAST stores cost at the node boundary behind it?  A linear hipGraph of 28 nodes, each
// `k_hop<MODE>`: block b reads the region that block (b + shift) % nb of the PREVIOUS node wrote (one batch of independent float4
// loads), then writes its own region with MODE stores: 0 plain, 1 write-through (`buffer_store_dwordx4 ... sc1`), 2 non-temporal
// (`global_store_dword ... nt`).  Blocks are dealt round-robin over the 8 XCDs: shift 0 / 8 = consumer on the producer's XCD,
// shift 1 = on the neighbouring one.  Total bytes per node 0.5 / 1 / 2 / 4 MB (128 blocks x 4 KB, then 256 blocks x 4 / 8 / 16 KB).
// Prints us per node; with --json one JSON object.  A second table: the GPU-side fixed cost of a graph replay (replay time of
// 7 / 14 / 28 / 56 empty nodes, least-squares intercept and slope).
//   hipcc --offload-arch=gfx950 -O3 tools/store_policy_probe.hip -o /tmp/store_policy_probe && /tmp/store_policy_probe
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr int MAXL = 4;
template <int MODE>
__global__ __launch_bounds__(256) void k_hop(const float4* src, float4* dst, int shift, int lines, unsigned bytes) {
  const int nb = gridDim.x, b = blockIdx.x, sb = (b + shift) % nb, t = threadIdx.x;
  float4 v[MAXL];
#pragma unroll
  for (int l = 0; l < MAXL; ++l) v[l] = src[((size_t)sb * lines + min(l, lines - 1)) * 256 + t];
  float4 acc = make_float4(1.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int l = 0; l < MAXL; ++l) if (l < lines) { acc.x += v[l].x; acc.y += v[l].y; acc.z += v[l].z; acc.w += v[l].w; }
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(dst, 0, (int)bytes, 0x00020000);   // (stores past `bytes` are dropped)
#pragma unroll
  for (int l = 0; l < MAXL; ++l) if (l < lines) {
    const unsigned idx = ((unsigned)b * lines + l) * 256 + t;
    if (MODE == 1) {
      u32x4 u; u.x = __float_as_uint(acc.x); u.y = __float_as_uint(acc.y); u.z = __float_as_uint(acc.z); u.w = __float_as_uint(acc.w);
      __builtin_amdgcn_raw_buffer_store_b128(u, rsrc, (int)(idx * 16u), 0, 16);           // aux 16 = sc1
    } else if (MODE == 2) {
      float* d = reinterpret_cast<float*>(dst + idx);
      __builtin_nontemporal_store(acc.x, d); __builtin_nontemporal_store(acc.y, d + 1);
      __builtin_nontemporal_store(acc.z, d + 2); __builtin_nontemporal_store(acc.w, d + 3);
    } else dst[idx] = acc;
  }
}
__global__ void k_empty() {}
static double run(hipGraphExec_t ge, hipStream_t s, int reps) {
  for (int i = 0; i < 200; ++i) hipGraphLaunch(ge, s);
  hipStreamSynchronize(s);
  auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < reps; ++i) hipGraphLaunch(ge, s);
  hipStreamSynchronize(s);
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps;
}
template <typename F>
static int chain(hipStream_t s, int N, F launch, double* us) {
  hipGraph_t g;
  CK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  for (int i = 0; i < N; ++i) launch(i);
  CK(hipStreamEndCapture(s, &g));
  hipGraphExec_t ge; CK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
  double best = 1e9;
  for (int r = 0; r < 3; ++r) { const double u = run(ge, s, 1500); if (u < best) best = u; }
  *us = best;
  CK(hipGraphExecDestroy(ge)); CK(hipGraphDestroy(g));
  return 0;
}
int main(int argc, char** argv) {
  const bool json = argc > 1 && !strcmp(argv[1], "--json");
  hipStream_t s; CK(hipStreamCreate(&s));
  const int N = 28;
  const char* mode_name[3] = {"plain", "sc1", "nt"};
  const int shifts[3] = {0, 8, 1};
  const int cfg[4][2] = {{128, 1}, {256, 1}, {256, 2}, {256, 4}};
  if (json) printf("{\"nodes_per_graph\": %d, \"us_per_node\": [", N);
  bool first = true;
  for (const auto& c : cfg) {
    const int nb = c[0], lines = c[1];
    const size_t bytes = (size_t)nb * lines * 256 * sizeof(float4);
    float4 *a, *b;
    CK(hipMalloc(&a, bytes)); CK(hipMalloc(&b, bytes)); CK(hipMemset(a, 0, bytes)); CK(hipMemset(b, 0, bytes));
    for (int mode = 0; mode < 3; ++mode) {
      if (!json) printf("%4.1f MB per node (%3d blocks x %2d KB) %-5s:", bytes / 1048576.0, nb, lines * 4, mode_name[mode]);
      for (int shift : shifts) {
        double us = 0.0;
        auto launch = [&](int i) {
          const float4* src = (i & 1) ? b : a; float4* dst = (i & 1) ? a : b;
          if (mode == 0) hipLaunchKernelGGL(k_hop<0>, dim3(nb), dim3(256), 0, s, src, dst, shift, lines, (unsigned)bytes);
          else if (mode == 1) hipLaunchKernelGGL(k_hop<1>, dim3(nb), dim3(256), 0, s, src, dst, shift, lines, (unsigned)bytes);
          else hipLaunchKernelGGL(k_hop<2>, dim3(nb), dim3(256), 0, s, src, dst, shift, lines, (unsigned)bytes);
        };
        if (chain(s, N, launch, &us)) return 1;
        if (json) { printf("%s{\"mb\": %.1f, \"blocks\": %d, \"store\": \"%s\", \"shift\": %d, \"us\": %.3f}", first ? "" : ", ", bytes / 1048576.0, nb, mode_name[mode], shift, us / N); first = false; }
        else printf("  shift %d: %5.2f us/node", shift, us / N);
      }
      if (!json) printf("\n");
    }
    CK(hipFree(a)); CK(hipFree(b));
  }
  // fixed cost per replay: empty nodes
  const int ns[4] = {7, 14, 28, 56};
  double t[4], sx = 0, sy = 0, sxx = 0, sxy = 0;
  for (int i = 0; i < 4; ++i) {
    if (chain(s, ns[i], [&](int) { hipLaunchKernelGGL(k_empty, dim3(1), dim3(64), 0, s); }, &t[i])) return 1;
    sx += ns[i]; sy += t[i]; sxx += (double)ns[i] * ns[i]; sxy += ns[i] * t[i];
  }
  const double slope = (4 * sxy - sx * sy) / (4 * sxx - sx * sx), icpt = (sy - slope * sx) / 4;
  if (json) printf("], \"empty_replay_us\": {\"7\": %.2f, \"14\": %.2f, \"28\": %.2f, \"56\": %.2f, \"slope_us_per_node\": %.3f, \"intercept_us\": %.2f}}\n", t[0], t[1], t[2], t[3], slope, icpt);
  else printf("empty nodes 7 / 14 / 28 / 56: %.2f / %.2f / %.2f / %.2f us per replay; slope %.3f us per node, intercept %.2f us\n", t[0], t[1], t[2], t[3], slope, icpt);
  return 0;
}
