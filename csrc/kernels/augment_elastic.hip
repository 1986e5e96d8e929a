// Elastic deformation of MNIST rows (Simard, Steinkraus, Platt 2003) on top of the affine map, once per epoch.
//
//   augment_elastic   uint8 [N, 784] -> uint8 [N, 784], row r of src resampled into row r of dst through
//                     its affine map plus its own smoothed random displacement field
//
// Definition (docs/ARCHITECTURE.md "Elastic augmentation"; tests/_elastic_oracle.py is its float64 twin).
// G is a float32 [32, 32] table: the 28 x 28 Gaussian matrix G[i][k] = exp(-(i-k)^2 / (2 sigma^2)) / Z inside
// zero padding.  Dataset row r draws two raw fields (c = 0: x displacement, c = 1: y displacement)
//   U_c[i][j] = 2 philox_uniform(seed, epoch, 2^40 + 1568 r + 784 c + 28 i + j) - 1        i = y, j = x
// smooths them, D_c = alpha (G U_c G), and output pixel (x, y) samples the source at
//   sx = a (x - c0) + b (y - c0) + c0 + e + D_0[y][x]      sy = cc (x - c0) + d (y - c0) + c0 + f + D_1[y][x]
// with theta = (a, b, e, cc, d, f) drawn as augment.hip draws it (indices 4 r + j < 2^33: the streams never
// meet); from there on it is augment.hip's rule: clamp to [-1, 28], bilinear, zero outside, min(255, floor(v + 0.5)).
//
// Work split.  As in augment.hip: one wave per image, four images per 256-thread workgroup, no workgroup
// barrier; lanes 0..48 load 16 bytes each and store the same 16 output pixels.
//
// Smoothing on the matrix cores, no LDS round trip.  G U G of a 32 x 32 padded field is two fp32 products of
// 2 x 2 tiles of 16 x 16, each tile a chain of v_mfma_f32_16x16x4_f32 over K.  With lane = 16 q + c:
//   an MFMA takes A[i = c][k = q] and B[k = q][n = c] from lane (q, c) and leaves D[4 q + v][c] in its
//   accumulator element v.
// The sum over K is the same under any order of K that A and B share, so each product picks the order that
// its operands already have:
//   V = U G.   Step s = 0..6 takes k = 4 s + q.  Lane (q, c) draws, by Philox, exactly the elements
//              U[16 ti + c][4 s + q] its A fragments hold (rows 28..31 are zeros, not draws; the step s = 7 is
//              columns 28..31, all zeros: neither drawn nor multiplied).  B is G[4 s + q][16 tn + c]: 16
//              registers, loaded once.  28 MFMAs per field.
//   S = G V.   V's accumulators hold V[16 t + 4 q + v][16 tn + c] in lane (q, c): as a B operand, step (t, v)
//              has k = 16 t + 4 q + v.  A is G in the same order, G[16 ti + c][16 t + 4 q + v]: four float4
//              loads of G's rows, 16 more registers.  32 MFMAs per field, no transpose, no shuffle.
// Every padded row or column of G is an exact zero in the table, every padded row of U an exact zero operand,
// so V's and S's padding is exact zeros and nothing outside 28 x 28 reaches a displacement.
//
// LDS.  Each wave owns its bordered fp32 image (augment.hip: 31 x 31 cells at pitch 39, see there for the
// pitch and for the clamps that make every tap an unconditional read) and, behind it, the two smoothed
// fields as [2][784] floats.  S leaves the accumulators in tile order -- lane (q, c) holds pixel rows
// 16 ti + 4 q + v of column 16 tn + c -- and the resampling wants 16 consecutive pixels per lane: that
// exchange is the only trip through LDS (a write of 16 consecutive floats per q, the q's 112 floats = 48
// banks apart: conflict-free; four 16-byte reads per field back).  With disp_in the field comes from
// global memory straight into those registers.  Ordering inside the wave: the wavefront fences around
// wave_barrier(), as in augment.hip.
#include "common.h"
#include "launchers.h"

namespace csed {
namespace {

constexpr int EL_SIDE = 28;
constexpr int EL_ROW = 784;
constexpr int EL_CELLS = 31;             // bordered side: cells -1 .. 29
constexpr int EL_PITCH = 39;             // floats per bordered row (augment.hip)
constexpr int EL_IMG = 1212;             // floats per image region: 31 * 39 = 1209, rounded up to 16 bytes
constexpr int EL_REGION = EL_IMG + 2 * EL_ROW;  // floats per wave: image, then the two fields
constexpr int EL_WAVES = 4;
constexpr int EL_LANES = EL_ROW / 16;    // 49 lanes carry pixels
constexpr int EL_BORDER = 3 * EL_CELLS + 3 * EL_SIDE;
constexpr int EL_G = 32;                 // padded side of G, U, V, S
constexpr float EL_C = 13.5f;
constexpr uint64_t EL_STREAM = 1ull << 40;  // first Philox index of the raw fields
static_assert(EL_IMG >= EL_CELLS * EL_PITCH && EL_IMG % 4 == 0 && EL_REGION % 4 == 0, "16-byte aligned fields");

__device__ __forceinline__ float uniform_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// The smoothed field c of dataset row r, alpha (G U_c G), written to fld[784] (LDS) by the whole wave.
// gB[tn][s] = G[4 s + q][16 tn + c], gA[ti][t] = G[16 ti + c][16 t + 4 q .. + 3].
__device__ __forceinline__ void smooth_field(float* fld, const float (&gB)[2][8], const f32x4 (&gA)[2][2],
                                             uint64_t seed, uint64_t epoch, uint64_t base, int q, int c,
                                             float alpha) {
  // ---- V = U G: the A fragments are drawn here, lane (q, c) element U[16 ti + c][4 s + q]
  f32x4 V[2][2];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti) {
    const int i = 16 * ti + c;
    f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 7; ++s) {
      const float u = philox_uniform(seed, epoch, base + (uint64_t)(EL_SIDE * i + 4 * s + q));
      const float a = i < EL_SIDE ? 2.0f * u - 1.0f : 0.0f;  // (2 u - 1 is exact: u is a multiple of 2^-24)
      v0 = mfma4(a, gB[0][s], v0);
      v1 = mfma4(a, gB[1][s], v1);
    }
    V[ti][0] = v0, V[ti][1] = v1;
  }
  // ---- S = G V: V's accumulators are the B fragments, k = 16 t + 4 q + v
#pragma unroll
  for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      f32x4 S = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int v = 0; v < 4; ++v) S = mfma4(gA[ti][t][v], V[t][tn][v], S);
      }
      const int x = 16 * tn + c;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int y = 16 * ti + 4 * q + v;
        if (x < EL_SIDE && y < EL_SIDE) fld[y * EL_SIDE + x] = alpha * S[v];
      }
    }
  }
}

__global__ __launch_bounds__(EL_WAVES * kWave) void augment_elastic_kernel(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const int64_t* __restrict__ idx,
    const float* __restrict__ theta_in, float* __restrict__ theta_out, const float* __restrict__ disp_in,
    float* __restrict__ disp_out, const float* __restrict__ gauss, int64_t N, int M, uint64_t seed,
    uint64_t epoch, float max_shift, float max_rot_rad, float max_scale, float alpha) {
  __shared__ __attribute__((aligned(16))) float lds[EL_WAVES * EL_REGION];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m = blockIdx.x * EL_WAVES + wave;  // wave-uniform: position in idx / theta / disp
  if (m >= M) return;
  const int64_t r = idx ? idx[m] : (int64_t)m;
  if (r < 0 || r >= N) return;  // an index outside the set: the row is skipped, nothing is written
  float* img = lds + wave * EL_REGION;
  float* fld = img + EL_IMG;

  // ---- the row's pixels: one uint4 per lane, issued before everything else
  uint4 px = make_uint4(0, 0, 0, 0);
  if (lane < EL_LANES) px = *reinterpret_cast<const uint4*>(src + r * EL_ROW + 16 * lane);

  // ---- the affine map, once per wave: augment.hip's draw, expression for expression
  float a, b, e, cc, d, f;
  if (theta_in) {
    const float* t = theta_in + 6 * (int64_t)m;
    a = t[0], b = t[1], e = t[2], cc = t[3], d = t[4], f = t[5];
  } else {
    const float u = philox_uniform(seed, epoch, 4ull * (uint64_t)r + (uint64_t)(lane & 3));
    const float t = 2.0f * u - 1.0f;
    const float dx = uniform_f(__shfl(t, 0, kWave)) * max_shift;
    const float dy = uniform_f(__shfl(t, 1, kWave)) * max_shift;
    const float phi = uniform_f(__shfl(t, 2, kWave)) * max_rot_rad;
    const float s = 1.0f + uniform_f(__shfl(t, 3, kWave)) * max_scale;
    float sn, cs;
    sincosf(phi, &sn, &cs);
    a = d = cs / s;
    b = sn / s;
    cc = -b;
    e = -dx;
    f = -dy;
  }
  a = uniform_f(a), b = uniform_f(b), e = uniform_f(e), cc = uniform_f(cc), d = uniform_f(d), f = uniform_f(f);
  if (theta_out && lane == 0) {
    float* t = theta_out + 6 * (int64_t)m;
    t[0] = a, t[1] = b, t[2] = e, t[3] = cc, t[4] = d, t[5] = f;
  }

  // ---- stage: zero border (all 64 lanes), then the image as fp32
  for (int i = lane; i < EL_BORDER; i += kWave) {
    int row, col;
    if (i < 3 * EL_CELLS) {  // full rows -1, 28, 29 (cells 0, 29, 30)
      const int k = i / EL_CELLS;
      row = k == 0 ? 0 : EL_SIDE + k;
      col = i - k * EL_CELLS;
    } else {  // columns -1, 28, 29 of the image's rows
      const int j = i - 3 * EL_CELLS, k = j % 3;
      row = 1 + j / 3;
      col = k == 0 ? 0 : EL_SIDE + k;
    }
    img[row * EL_PITCH + col] = 0.0f;
  }
  if (lane < EL_LANES) {
    const uint32_t w[4] = {px.x, px.y, px.z, px.w};
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const int p = 16 * lane + 4 * qd, y = p / EL_SIDE, x = p - y * EL_SIDE;
      float* o = img + (y + 1) * EL_PITCH + (x + 1);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (float)((w[qd] >> (8 * j)) & 0xffu);
    }
  }

  // ---- the two displacement fields, drawn and smoothed by all 64 lanes (the branch is wave-uniform)
  const bool drawn = !disp_in && alpha != 0.0f;  // (alpha = 0: the field is zero, the affine kernel's bytes)
  if (drawn) {
    const int q = lane >> 4, c = lane & 15;
    float gB[2][8];
    f32x4 gA[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int s = 0; s < 8; ++s) gB[t][s] = gauss[(4 * s + q) * EL_G + 16 * t + c];
#pragma unroll
      for (int k = 0; k < 2; ++k) gA[t][k] = *reinterpret_cast<const f32x4*>(gauss + (16 * t + c) * EL_G + 16 * k + 4 * q);
    }
    const uint64_t base = EL_STREAM + 1568ull * (uint64_t)r;
    smooth_field(fld, gB, gA, seed, epoch, base, q, c, alpha);
    smooth_field(fld + EL_ROW, gB, gA, seed, epoch, base + EL_ROW, q, c, alpha);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane >= EL_LANES) return;

  // ---- this lane's 16 displacements per axis: from LDS, from disp_in, or zero
  f32x4 D[2][4];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const int o = k * EL_ROW + 16 * lane + 4 * qd;
      if (disp_in) D[k][qd] = *reinterpret_cast<const f32x4*>(disp_in + 2 * EL_ROW * (int64_t)m + o);
      else if (drawn) D[k][qd] = *reinterpret_cast<const f32x4*>(fld + o);
      else D[k][qd] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (disp_out) *reinterpret_cast<f32x4*>(disp_out + 2 * EL_ROW * (int64_t)m + o) = D[k][qd];
    }
  }

  // ---- gather: augment.hip's, with the displacement added to the coordinate before the clamp
  uint32_t out[4];
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {
    const int p = 16 * lane + 4 * qd, y = p / EL_SIDE, x = p - y * EL_SIDE;
    const float yc = (float)y - EL_C;
    const float bx = fmaf(b, yc, EL_C + e), by = fmaf(d, yc, EL_C + f);
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float xc = (float)(x + j) - EL_C;
      const float sx = fmaxf(fminf(fmaf(a, xc, bx) + D[0][qd][j], (float)EL_SIDE), -1.0f);
      const float sy = fmaxf(fminf(fmaf(cc, xc, by) + D[1][qd][j], (float)EL_SIDE), -1.0f);
      const float x0 = floorf(sx), y0 = floorf(sy);
      const float fx = sx - x0, fy = sy - y0;
      const int cx = min(max((int)x0, -1), EL_SIDE) + 1, cy = min(max((int)y0, -1), EL_SIDE) + 1;  // cells 0 .. 29
      const float* t = img + cy * EL_PITCH + cx;
      const float v00 = t[0], v01 = t[1], v10 = t[EL_PITCH], v11 = t[EL_PITCH + 1];
      const float top = fmaf(fx, v01 - v00, v00), bot = fmaf(fx, v11 - v10, v10);
      const float v = fmaf(fy, bot - top, top);
      const uint32_t byte = min((uint32_t)floorf(v + 0.5f), 255u);
      word |= byte << (8 * j);
    }
    out[qd] = word;
  }
  *reinterpret_cast<uint4*>(dst + r * EL_ROW + 16 * lane) = make_uint4(out[0], out[1], out[2], out[3]);
}

}  // namespace

hipError_t launch_augment_elastic(const uint8_t* src, uint8_t* dst, const int64_t* idx, const float* theta_in,
                                  float* theta_out, const float* disp_in, float* disp_out, const float* gauss,
                                  int64_t N, int64_t M, uint64_t seed, uint64_t epoch, float max_shift,
                                  float max_rot_deg, float max_scale, float alpha, hipStream_t s) {
  if (M <= 0) return hipSuccess;
  const float max_rot_rad = max_rot_deg * 0.017453292519943295f;
  hipLaunchKernelGGL(augment_elastic_kernel, dim3((unsigned)((M + EL_WAVES - 1) / EL_WAVES)),
                     dim3(EL_WAVES * kWave), 0, s, src, dst, idx, theta_in, theta_out, disp_in, disp_out, gauss, N,
                     (int)M, seed, epoch, max_shift, max_rot_rad, max_scale, alpha);
  return hipGetLastError();
}

}  // namespace csed
