// Random affine augmentation of MNIST rows (shift / rotate / scale), once per epoch.
//
//   augment_affine   uint8 [N, 784] -> uint8 [N, 784], row r of src warped into row r of dst
//
// The engines gather raw uint8 rows of the device-resident train set inside their step kernels, so
// augmentation is a copy of that set made by this kernel before the epoch; the step kernels then read
// the copy.  It has no counterpart in the reference (ref src/train.py:25-41 uses ToTensor + Normalize only).
//
// Definition (docs/ARCHITECTURE.md "Affine augmentation"; tests/_augment_oracle.py is its float64 twin).
// With c = 13.5 and theta = (a, b, e, cc, d, f), output pixel (x, y) samples the source at
//   sx = a (x - c) + b (y - c) + c + e        sy = cc (x - c) + d (y - c) + c + f
// bilinearly over the four neighbouring pixel centres, taps outside [0, 27]^2 contributing 0; the byte
// is min(255, floor(v + 0.5)).  A drawn map of dataset row r takes u_j = philox_uniform(seed, epoch, 4 r + j):
//   dx = (2 u0 - 1) max_shift   dy = (2 u1 - 1) max_shift   phi = (2 u2 - 1) max_rot_deg pi / 180
//   s = 1 + (2 u3 - 1) max_scale      a = d = cos(phi) / s,  b = -cc = sin(phi) / s,  e = -dx,  f = -dy
// keyed by the dataset row, not by the position in idx, the grid or the rank.
//
// Work split.  One wave per image, four images per 256-thread workgroup.  A row is 49 x 16 bytes: lanes
// 0..48 load one uint4 each, and later produce the same 16 consecutive output pixels and store them with
// one 16-byte store; lanes 49..63 only help with the border.  28 = 7 x 4, so every aligned group of four
// pixels lies inside one image row: a lane's 16 pixels are four such groups.
//
// LDS.  Each wave owns IMG floats: the image as fp32 inside a zero border, one cell before and two after
// in both directions (31 x 31 cells at row pitch PITCH).  Source coordinates are clamped to [-1, 28]
// before the floor, so floor is in [-1, 28] and the four taps (x0, x0 + 1) x (y0, y0 + 1) are cells
// 0..30: every tap is an unconditional LDS read, the ones outside the image read the border's zeros (at
// the clamp itself the fraction is 0 and both cells are border or carry weight 0).  fminf / fmaxf return
// the other operand for a NaN, so a NaN theta reads cell 0 instead of a wild address; the integer cell is
// clamped once more for the same reason.
//
// PITCH = 39 floats.  The 49 lanes of one read are 16 pixels apart: seven lanes cover four image rows, so
// lane 7 m + j reads row 4 m + const at the same column as lane j.  A pitch that is a multiple of 16
// dwords folds those seven rows onto one bank (pitch 32: 7-way at the identity map); an odd pitch spreads
// them.  Counted on a 64-bank model over all 64 reads of a lane (16 pixels x 4 taps): pitch 39 is 2-way
// at the identity and the 90-degree turn, at most 3-way at 7 and 15 degrees with shift and scale (mean
// 2.0 - 2.5); 31, 33, 35 and 37 reach 4- or 5-way at one of those angles.
//
// A wave touches only its own region, so the kernel has no workgroup barrier.  What orders a wave's LDS
// writes before its reads: LDS instructions of one wave execute in issue order, so the only thing to
// prevent is the compiler moving a read above a write of another lane -- the wavefront-scope fences
// around wave_barrier() below.
#include "common.h"
#include "launchers.h"

namespace csed {
namespace {

constexpr int AUG_SIDE = 28;            // image side
constexpr int AUG_ROW = 784;            // bytes per row of src / dst
constexpr int AUG_CELLS = 31;           // bordered side: cells -1 .. 29
constexpr int AUG_PITCH = 39;           // floats per bordered row (see above)
constexpr int AUG_IMG = AUG_CELLS * AUG_PITCH;  // floats per wave
constexpr int AUG_WAVES = 4;            // images per workgroup
constexpr int AUG_LANES = AUG_ROW / 16; // 49 lanes carry pixels
constexpr int AUG_BORDER = 3 * AUG_CELLS + 3 * AUG_SIDE;  // border cells: rows -1, 28, 29 and columns -1, 28, 29
constexpr float AUG_C = 13.5f;

__device__ __forceinline__ float uniform_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

__global__ __launch_bounds__(AUG_WAVES * kWave) void augment_affine_kernel(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const int64_t* __restrict__ idx,
    const float* __restrict__ theta_in, float* __restrict__ theta_out, int64_t N, int M, uint64_t seed,
    uint64_t epoch, float max_shift, float max_rot_rad, float max_scale) {
  __shared__ float lds[AUG_WAVES * AUG_IMG];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m = blockIdx.x * AUG_WAVES + wave;  // wave-uniform: position in idx / theta
  if (m >= M) return;
  const int64_t r = idx ? idx[m] : (int64_t)m;
  if (r < 0 || r >= N) return;  // an index outside the set: the row is skipped, nothing is written
  float* img = lds + wave * AUG_IMG;

  // ---- the row's pixels: one uint4 per lane, issued before the map's arithmetic
  uint4 px = make_uint4(0, 0, 0, 0);
  if (lane < AUG_LANES) px = *reinterpret_cast<const uint4*>(src + r * AUG_ROW + 16 * lane);

  // ---- the map, once per wave
  float a, b, e, cc, d, f;
  if (theta_in) {
    const float* t = theta_in + 6 * (int64_t)m;
    a = t[0], b = t[1], e = t[2], cc = t[3], d = t[4], f = t[5];
  } else {
    // lane j < 4 draws u_j (the other lanes repeat them): one Philox evaluation for the four draws
    const float u = philox_uniform(seed, epoch, 4ull * (uint64_t)r + (uint64_t)(lane & 3));
    const float t = 2.0f * u - 1.0f;  // exact: u is a multiple of 2^-24 in [0, 1)
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
  for (int i = lane; i < AUG_BORDER; i += kWave) {
    int row, col;
    if (i < 3 * AUG_CELLS) {  // full rows -1, 28, 29 (cells 0, 29, 30)
      const int k = i / AUG_CELLS;
      row = k == 0 ? 0 : AUG_SIDE + k;
      col = i - k * AUG_CELLS;
    } else {  // columns -1, 28, 29 of the image's rows
      const int j = i - 3 * AUG_CELLS, k = j % 3;
      row = 1 + j / 3;
      col = k == 0 ? 0 : AUG_SIDE + k;
    }
    img[row * AUG_PITCH + col] = 0.0f;
  }
  if (lane < AUG_LANES) {
    const uint32_t w[4] = {px.x, px.y, px.z, px.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p = 16 * lane + 4 * q, y = p / AUG_SIDE, x = p - y * AUG_SIDE;
      float* o = img + (y + 1) * AUG_PITCH + (x + 1);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (float)((w[q] >> (8 * j)) & 0xffu);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane >= AUG_LANES) return;

  // ---- gather: 16 output pixels per lane, the coordinate recomputed per pixel from the definition
  uint32_t out[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int p = 16 * lane + 4 * q, y = p / AUG_SIDE, x = p - y * AUG_SIDE;
    const float yc = (float)y - AUG_C;
    const float bx = fmaf(b, yc, AUG_C + e), by = fmaf(d, yc, AUG_C + f);
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float xc = (float)(x + j) - AUG_C;
      const float sx = fmaxf(fminf(fmaf(a, xc, bx), (float)AUG_SIDE), -1.0f);
      const float sy = fmaxf(fminf(fmaf(cc, xc, by), (float)AUG_SIDE), -1.0f);
      const float x0 = floorf(sx), y0 = floorf(sy);
      const float fx = sx - x0, fy = sy - y0;
      const int cx = min(max((int)x0, -1), AUG_SIDE) + 1, cy = min(max((int)y0, -1), AUG_SIDE) + 1;  // cells 0 .. 29
      const float* t = img + cy * AUG_PITCH + cx;
      const float v00 = t[0], v01 = t[1], v10 = t[AUG_PITCH], v11 = t[AUG_PITCH + 1];
      const float top = fmaf(fx, v01 - v00, v00), bot = fmaf(fx, v11 - v10, v10);  // (differences of bytes: exact)
      const float v = fmaf(fy, bot - top, top);
      const uint32_t byte = min((uint32_t)floorf(v + 0.5f), 255u);
      word |= byte << (8 * j);
    }
    out[q] = word;
  }
  *reinterpret_cast<uint4*>(dst + r * AUG_ROW + 16 * lane) = make_uint4(out[0], out[1], out[2], out[3]);
}

}  // namespace

hipError_t launch_augment_affine(const uint8_t* src, uint8_t* dst, const int64_t* idx, const float* theta_in,
                                 float* theta_out, int64_t N, int64_t M, uint64_t seed, uint64_t epoch,
                                 float max_shift, float max_rot_deg, float max_scale, hipStream_t s) {
  if (M <= 0) return hipSuccess;
  const float max_rot_rad = max_rot_deg * 0.017453292519943295f;
  hipLaunchKernelGGL(augment_affine_kernel, dim3((unsigned)((M + AUG_WAVES - 1) / AUG_WAVES)),
                     dim3(AUG_WAVES * kWave), 0, s, src, dst, idx, theta_in, theta_out, N, (int)M, seed, epoch,
                     max_shift, max_rot_rad, max_scale);
  return hipGetLastError();
}

}  // namespace csed
