// Global-norm gradient clipping of a flat fp32 gradient, in place (torch.nn.utils.clip_grad_norm_ with the
// 2-norm and error_if_nonfinite=False):
//
//   norm = sqrt(sum g_i^2);  coef = min(1, max_norm / (norm + 1e-6));  g_i *= coef
//
// all in fp32, stats[0] = norm (before clipping) and stats[1] = coef left on the device.  Nothing branches on
// a non-finite value: an inf or NaN in g makes norm, coef and every g_i what torch makes them.  With coef == 1
// the multiply still runs and leaves every g_i bitwise as it was.
//
// The order of the sum is a function of n alone (kernels/clip_plan.h), so every data-parallel rank, which
// clips the same all-reduced gradient, gets the same coefficient and the replicas stay bitwise identical:
//
//   * g is read as "quads", float4s counted from g itself: quad j is g[4j .. 4j+3] whatever g's address (the
//     16-byte accesses are declared 4-byte aligned, so a view that starts one float into a buffer is read
//     through the same instructions in the same order), and the n % 4 floats behind the last quad are scalars;
//   * a thread adds the squares of its quads in ascending index order, one fmaf per float, acc = g^2 + acc;
//   * the 64 lanes of a wave go through the xor butterfly (32, 16, .. 1: every lane ends with the same bits);
//   * the 16 wave sums go through LDS and are added in wave order by every thread;
//   * (two-launch form) the workgroups' sums are added in workgroup order.
//
// Two forms, no workgroup ever waits for another and no atomic is used:
//
//   n <= kClipOneWgMax: clip_one_wg_kernel, ONE workgroup of 1024 threads.  Thread t loads quads t, t + 1024, ..
//     (at most kClipQuadsPerThread) into registers, the workgroup reduces, and the thread scales and stores
//     the registers it still holds: g crosses the memory system once in each direction and the step gets one
//     launch.  LeNet's 21,840 floats are 5,460 quads: 6 loads of a wave cover 1.5 KB each, all in flight
//     before the first fmaf.
//   n >  kClipOneWgMax: clip_sqnorm_partials_kernel (workgroup b sums quads [b * chunk, (b + 1) * chunk) into
//     partials[b]), then clip_scale_kernel on the same grid: wave 0 of every workgroup re-adds the partials in
//     index order (the same bits in every workgroup), and the workgroup scales its own chunk.  Workgroup 0
//     writes stats.
#include "common.h"
#include "launchers.h"

namespace csed {
namespace {

constexpr int kClipWaves = kClipThreads / kWave;

// 16 bytes of gradient at a 4-byte aligned address
struct __attribute__((packed, aligned(4))) Quad {
  float x, y, z, w;
};

__device__ __forceinline__ float sq_acc(float acc, const Quad& q) {
  acc = fmaf(q.x, q.x, acc);
  acc = fmaf(q.y, q.y, acc);
  acc = fmaf(q.z, q.z, acc);
  return fmaf(q.w, q.w, acc);
}

__device__ __forceinline__ Quad scaled(Quad q, float c) {
  q.x *= c;
  q.y *= c;
  q.z *= c;
  q.w *= c;
  return q;
}

// The workgroup's sum of every thread's acc, the same bits in every thread: butterfly, then the wave sums
// in wave order.
__device__ __forceinline__ float block_sum(float acc, float* wsum) {
  acc = wave_sum(acc);
  if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x / kWave] = acc;
  __syncthreads();
  float s = wsum[0];
#pragma unroll
  for (int w = 1; w < kClipWaves; ++w) s += wsum[w];
  return s;
}

// torch's max_norm / (norm + 1e-6) clamped from above at 1; a NaN stays a NaN (fminf would drop it)
__device__ __forceinline__ float clip_coef(float norm, float max_norm) {
  const float c = max_norm / (norm + 1e-6f);
  return c > 1.0f ? 1.0f : c;
}

__global__ __launch_bounds__(kClipThreads) void clip_one_wg_kernel(float* __restrict__ g, int n, float max_norm,
                                                                   float* __restrict__ stats) {
  __shared__ float wsum[kClipWaves];
  const int t = threadIdx.x, quads = n >> 2, rem = n & 3;
  Quad* gq = reinterpret_cast<Quad*>(g);
  Quad v[kClipQuadsPerThread];
#pragma unroll
  for (int i = 0; i < kClipQuadsPerThread; ++i) {
    const int j = t + i * kClipThreads;
    if (j < quads)
      v[i] = gq[j];
    else
      v[i] = Quad{0.f, 0.f, 0.f, 0.f};
  }
  float e = 0.f;
  if (t < rem) e = g[4 * quads + t];
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < kClipQuadsPerThread; ++i) acc = sq_acc(acc, v[i]);  // (a slot past the end adds +0)
  acc = fmaf(e, e, acc);
  const float norm = sqrtf(block_sum(acc, wsum));
  const float coef = clip_coef(norm, max_norm);
#pragma unroll
  for (int i = 0; i < kClipQuadsPerThread; ++i) {
    const int j = t + i * kClipThreads;
    if (j < quads) gq[j] = scaled(v[i], coef);
  }
  if (t < rem) g[4 * quads + t] = e * coef;
  if (t == 0) {
    stats[0] = norm;
    stats[1] = coef;
  }
}

__global__ __launch_bounds__(kClipThreads) void clip_sqnorm_partials_kernel(const float* __restrict__ g, int64_t n,
                                                                            int64_t chunk,
                                                                            float* __restrict__ partials) {
  __shared__ float wsum[kClipWaves];
  constexpr int64_t T = kClipThreads;
  const int64_t quads = n >> 2, q0 = (int64_t)blockIdx.x * chunk;
  const int64_t q1 = q0 + chunk < quads ? q0 + chunk : quads;
  const Quad* gq = reinterpret_cast<const Quad*>(g);
  float acc = 0.f;
  int64_t j = q0 + threadIdx.x;
  for (; j + 3 * T < q1; j += 4 * T) {  // four loads in flight; the adds keep the ascending order
    const Quad a = gq[j], b = gq[j + T], c = gq[j + 2 * T], d = gq[j + 3 * T];
    acc = sq_acc(sq_acc(sq_acc(sq_acc(acc, a), b), c), d);
  }
  for (; j < q1; j += T) acc = sq_acc(acc, gq[j]);
  if (blockIdx.x == gridDim.x - 1 && (int64_t)threadIdx.x < (n & 3)) {  // the floats behind the last quad
    const float e = g[4 * quads + threadIdx.x];
    acc = fmaf(e, e, acc);
  }
  const float s = block_sum(acc, wsum);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(kClipThreads) void clip_scale_kernel(float* __restrict__ g, int64_t n, int64_t chunk,
                                                                  const float* __restrict__ partials, float max_norm,
                                                                  float* __restrict__ stats) {
  __shared__ float total;
  if (threadIdx.x < kWave) {  // gridDim.x partials, one per workgroup of the first launch
    float s = partials[0];
    for (unsigned b = 1; b < gridDim.x; ++b) s += partials[b];
    if (threadIdx.x == 0) total = s;
  }
  __syncthreads();
  const float norm = sqrtf(total);
  const float coef = clip_coef(norm, max_norm);
  constexpr int64_t T = kClipThreads;
  const int64_t quads = n >> 2, q0 = (int64_t)blockIdx.x * chunk;
  const int64_t q1 = q0 + chunk < quads ? q0 + chunk : quads;
  Quad* gq = reinterpret_cast<Quad*>(g);
  int64_t j = q0 + threadIdx.x;
  for (; j + 3 * T < q1; j += 4 * T) {
    const Quad a = gq[j], b = gq[j + T], c = gq[j + 2 * T], d = gq[j + 3 * T];
    gq[j] = scaled(a, coef);
    gq[j + T] = scaled(b, coef);
    gq[j + 2 * T] = scaled(c, coef);
    gq[j + 3 * T] = scaled(d, coef);
  }
  for (; j < q1; j += T) gq[j] = scaled(gq[j], coef);
  if (blockIdx.x == gridDim.x - 1 && (int64_t)threadIdx.x < (n & 3)) g[4 * quads + threadIdx.x] *= coef;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    stats[0] = norm;
    stats[1] = coef;
  }
}

}  // namespace

hipError_t launch_clip_grad_norm(float* g, int64_t n, float max_norm, float* stats, float* partials,
                                 int64_t partials_n, hipStream_t s) {
  const ClipPlan p = clip_plan(n);
  if (p.error || !g || !stats) return hipErrorInvalidValue;
  if (p.form == 0) {
    hipLaunchKernelGGL(clip_one_wg_kernel, dim3(1), dim3(kClipThreads), 0, s, g, (int)n, max_norm, stats);
    return hipGetLastError();
  }
  if (!partials || partials_n < p.partials) return hipErrorInvalidValue;
  hipLaunchKernelGGL(clip_sqnorm_partials_kernel, dim3(p.grid), dim3(kClipThreads), 0, s, g, n, p.chunk, partials);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(clip_scale_kernel, dim3(p.grid), dim3(kClipThreads), 0, s, g, n, p.chunk, partials, max_norm,
                     stats);
  return hipGetLastError();
}

// Load this translation unit's code object now (hipFuncGetAttributes; the HIP runtime loads it
// lazily, at the TU's first launch): csed::preload_kernels, so a cold epoch does not pay it.
hipError_t preload_clip() {
  hipFuncAttributes attr;
  return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(clip_one_wg_kernel));
}

}  // namespace csed
