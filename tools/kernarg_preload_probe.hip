// What does a dependent scalar-load round at the head of a node cost, and does kernel-argument preloading (the packet processor
// places the first kernel-argument dwords in user SGPRs before the wave starts) remove it?  A linear hipGraph of 28 nodes; each
// node's 128 blocks do what the update kernels' blocks do first: decide a role from the kernel arguments (rider or tile), select one
// of 4 descriptors by the block id, copy that descriptor by value, issue one batch of float4 loads through it, and as many stores.
//   form "struct": everything in one by-value struct (the kernels' form): role -> descriptor choice -> descriptor = 3 rounds
//   form "header": the decision words as leading scalar parameters in front of the same struct
// The preload switch is per translation unit, so the probe is built twice; "header" of the build WITHOUT the switch loads its
// scalars in one round (2 rounds in all), "header" of the build WITH it has them in SGPRs at entry (1 round) -- if the firmware
// honours the request; otherwise the compiler's compatibility prologue loads them and the two builds time alike.
// A second table: replay time of 7 / 14 / 28 / 56 empty nodes, without parameters and with 14 scalar ones (preloaded in the
// build with the switch): does the number of user SGPRs move the launch floor?
//   hipcc --offload-arch=gfx950 -O3 tools/kernarg_preload_probe.hip -o /tmp/kpp_off
//   hipcc --offload-arch=gfx950 -O3 -mllvm -amdgpu-kernarg-preload-count=16 -DPROBE_PRELOAD=1 tools/kernarg_preload_probe.hip -o /tmp/kpp_on
// Each prints one JSON object (--json) or a table.
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdio>
#include <cstring>
#ifndef PROBE_PRELOAD
#define PROBE_PRELOAD 0
#endif
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
constexpr int LINES = 1;    // float4 per thread: 0.5 MB read and 0.5 MB written per node -- light enough for a scalar round to show
// A descriptor is 200 bytes, as the update kernels' are: its words lie in four 64-byte lines of the kernel-argument segment, and the
// role words lie behind the four descriptors -- every round of the struct form asks for lines no earlier round has brought in.  (With
// everything in one or two lines the later rounds hit the scalar cache and cost nothing: the first version of this probe.)
struct Desc { const float4* src; int ld; int pad0[15]; float4* dst; int rows; int pad1[15]; int scale; int pad2[11]; int tile0; };
static_assert(sizeof(Desc) == 200, "descriptor size");
struct Args { Desc d[4]; int pad[16]; int nprob; int tiles; int riders; int pad1; float* rider_dst; };

__device__ __forceinline__ void body(const Desc q, int b) {
  const int t = threadIdx.x, local = min(b - q.tile0, q.rows - 1);
  float4 v[LINES];
#pragma unroll
  for (int l = 0; l < LINES; ++l) v[l] = q.src[(size_t)local * q.ld + l * 256 + t];
#pragma unroll
  for (int l = 0; l < LINES; ++l) {
    float4 o = v[l]; o.x = o.x * 0.5f + (float)q.scale;
    q.dst[(size_t)local * q.ld + l * 256 + t] = o;
  }
}
__global__ __launch_bounds__(256) void k_struct(Args p) {
  const int b = blockIdx.x;
  if (b >= p.tiles) { if (b - p.tiles < p.riders && threadIdx.x == 0) p.rider_dst[b - p.tiles] = 1.f; return; }
  int pi = 0;
  if (p.nprob > 1 && b >= p.d[1].tile0) pi = 1;
  if (p.nprob > 2 && b >= p.d[2].tile0) pi = 2;
  if (p.nprob > 3 && b >= p.d[3].tile0) pi = 3;
  body(p.d[pi], b);
}
__global__ __launch_bounds__(256) void k_header(int tiles, int riders, int nprob, int t1, int t2, int t3, Args p) {
  const int b = blockIdx.x;
  if (b >= tiles) { if (b - tiles < riders && threadIdx.x == 0) p.rider_dst[b - tiles] = 1.f; return; }
  int pi = 0;
  if (nprob > 1 && b >= t1) pi = 1;
  if (nprob > 2 && b >= t2) pi = 2;
  if (nprob > 3 && b >= t3) pi = 3;
  body(p.d[pi], b);
}
__global__ void k_empty() {}
__global__ void k_empty14(int a0, int a1, int a2, int a3, int a4, int a5, int a6, int a7, int a8, int a9, int a10, int a11, int a12, int a13) {}

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
  for (int r = 0; r < 5; ++r) { const double u = run(ge, s, 1500); if (u < best) best = u; }
  *us = best;
  CK(hipGraphExecDestroy(ge)); CK(hipGraphDestroy(g));
  return 0;
}
int main(int argc, char** argv) {
  const bool json = argc > 1 && !strcmp(argv[1], "--json");
  hipStream_t s; CK(hipStreamCreate(&s));
  const int N = 28, tiles = 128, riders = 8, per = 32, ld = LINES * 256;
  const size_t bytes = (size_t)tiles * ld * sizeof(float4);
  float4 *a, *b; float* rd;
  CK(hipMalloc(&a, bytes)); CK(hipMalloc(&b, bytes)); CK(hipMalloc(&rd, riders * sizeof(float)));
  CK(hipMemset(a, 0, bytes)); CK(hipMemset(b, 0, bytes));
  auto args = [&](int i) {
    Args p{};
    const float4* src = (i & 1) ? b : a; float4* dst = (i & 1) ? a : b;
    for (int k = 0; k < 4; ++k) { Desc& q = p.d[k]; q.src = src + (size_t)k * per * ld; q.dst = dst + (size_t)k * per * ld; q.ld = ld; q.rows = per; q.tile0 = k * per; q.scale = 0; }
    p.nprob = 4; p.tiles = tiles; p.riders = riders; p.rider_dst = rd;
    return p;
  };
  const dim3 grid(tiles + riders), block(256);
  double us_struct = 0, us_header = 0;
  // interleaved four times, best kept: the two forms see the same state of the machine
  for (int rep = 0; rep < 4; ++rep) {
    double u = 0;
    if (chain(s, N, [&](int i) { hipLaunchKernelGGL(k_struct, grid, block, 0, s, args(i)); }, &u)) return 1;
    if (!rep || u < us_struct) us_struct = u;
    if (chain(s, N, [&](int i) { const Args p = args(i); hipLaunchKernelGGL(k_header, grid, block, 0, s, p.tiles, p.riders, p.nprob, p.d[1].tile0, p.d[2].tile0, p.d[3].tile0, p); }, &u)) return 1;
    if (!rep || u < us_header) us_header = u;
  }
  const int ns[4] = {7, 14, 28, 56};
  double t0[4], t14[4];
  for (int i = 0; i < 4; ++i) {
    if (chain(s, ns[i], [&](int) { hipLaunchKernelGGL(k_empty, dim3(1), dim3(64), 0, s); }, &t0[i])) return 1;
    if (chain(s, ns[i], [&](int) { hipLaunchKernelGGL(k_empty14, dim3(1), dim3(64), 0, s, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13); }, &t14[i])) return 1;
  }
  auto fit = [&](const double* t, double* slope, double* icpt) {
    double sx = 0, sy = 0, sxx = 0, sxy = 0;
    for (int i = 0; i < 4; ++i) { sx += ns[i]; sy += t[i]; sxx += (double)ns[i] * ns[i]; sxy += ns[i] * t[i]; }
    *slope = (4 * sxy - sx * sy) / (4 * sxx - sx * sx); *icpt = (sy - *slope * sx) / 4;
  };
  double s0, i0, s14, i14;
  fit(t0, &s0, &i0); fit(t14, &s14, &i14);
  if (json) {
    printf("{\"built_with_preload\": %s, \"nodes_per_graph\": %d, \"blocks\": %d, \"us_per_node\": {\"struct\": %.3f, \"header\": %.3f}, ",
           PROBE_PRELOAD ? "true" : "false", N, tiles + riders, us_struct / N, us_header / N);
    printf("\"empty_replay_us\": {\"no_params\": {\"7\": %.2f, \"14\": %.2f, \"28\": %.2f, \"56\": %.2f, \"slope_us_per_node\": %.3f, \"intercept_us\": %.2f}, ",
           t0[0], t0[1], t0[2], t0[3], s0, i0);
    printf("\"14_scalars\": {\"7\": %.2f, \"14\": %.2f, \"28\": %.2f, \"56\": %.2f, \"slope_us_per_node\": %.3f, \"intercept_us\": %.2f}}}\n",
           t14[0], t14[1], t14[2], t14[3], s14, i14);
  } else {
    printf("preload switch %s: struct %.3f us/node, header %.3f us/node (%d nodes of %d blocks)\n", PROBE_PRELOAD ? "ON" : "off", us_struct / N, us_header / N, N, tiles + riders);
    printf("empty nodes 7 / 14 / 28 / 56, no parameters: %.2f / %.2f / %.2f / %.2f us per replay; slope %.3f us per node, intercept %.2f us\n", t0[0], t0[1], t0[2], t0[3], s0, i0);
    printf("empty nodes 7 / 14 / 28 / 56, 14 scalars:    %.2f / %.2f / %.2f / %.2f us per replay; slope %.3f us per node, intercept %.2f us\n", t14[0], t14[1], t14[2], t14[3], s14, i14);
  }
  CK(hipFree(a)); CK(hipFree(b)); CK(hipFree(rd));
  return 0;
}
