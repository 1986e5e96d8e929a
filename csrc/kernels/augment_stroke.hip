// Stroke-thickness and random-erasing augmentation of MNIST rows, once per epoch.
//
//   augment_stroke   uint8 [N, 784] -> uint8 [N, 784], row r of src thickened / thinned and masked into row r of dst
//
// Like the affine kernel (augment.hip) it rewrites the epoch's copy of the train set; unlike it, it is not a
// resampling through a coordinate map but a grey-level morphology with a disc and a rectangle mask, all in
// integers.  It has no counterpart in the reference.
//
// Definition (docs/ARCHITECTURE.md "Stroke augmentation"; tests/_stroke_oracle.py is its NumPy twin, bit for bit).
// Parameters (q, e, top, left, h, w), int32.  B_k = {dx^2 + dy^2 <= k^2}, k = 0..3: row dy of the disc is the
// span |dx| <= w_k(|dy|), w_1 = (1, 0), w_2 = (2, 1, 0), w_3 = (3, 2, 2, 0).  q is clamped to [-768, 768];
// a = |q|, k = a >> 8, p = a & 255, k1 = min(k + 1, 3); M_j = max over B_j of I for q >= 0, min for q < 0, taps
// outside the image reading 0 either way; the byte is (M_k (256 - p) + M_k1 p + 128) >> 8.  If e != 0 the
// pixels top <= y < top + h, left <= x < left + w become 0 afterwards.  Drawn parameters of dataset row r take
// u_j = philox_uniform(seed, epoch, 2^41 + 8 r + j), U_j = 2^24 u_j:
//   t = (2 u_0 - 1) T (fp32, one rounding)   q = sign(t) floor(256 |t|)   e = u_1 < erase_p
//   h = lo + ((U_2 n) >> 24)   w = lo + ((U_3 n) >> 24)   n = hi - lo + 1
//   top = (U_4 (29 - h)) >> 24   left = (U_5 (29 - w)) >> 24
// keyed by the dataset row, not by the position in idx, the grid or the rank.
//
// Work split.  augment.hip's: one wave per image, four images per 256-thread workgroup, lanes 0..48 own 16
// consecutive pixels each (one 16-byte load, one 16-byte store), which are four aligned groups of four pixels,
// every group inside one image row (28 = 7 x 4).  The whole row is in registers before anything is stored, so
// dst may be src.
//
// The maxima.  A disc is a union of horizontal spans, so the work is split into a horizontal and a vertical
// pass.  Horizontal, in registers: a group's three-pixel neighbourhood to the left and right is the group before
// and after it -- another register of the same lane, or the neighbouring lane's last / first register (one
// shuffle each way), or the fill value where the group touches the image's edge.  From those twelve bytes come
// the running maxima H_0..H_3 over half-widths 0..3 of each pixel, packed into one 32-bit word (byte j = H_j).
// Vertical, through LDS: M_k(x, y) is the maximum over |dy| <= k of byte w_k(|dy|) of word (x, y + dy).  M_k and
// M_k1 come from the same 2 k1 + 1 <= 7 words per pixel, and because a lane's pixels are four aligned groups of
// four, from 4 (2 k1 + 1) 16-byte LDS reads per lane.  k, k1 and the byte selectors are wave-uniform (scalar loop
// bounds and shift counts; the span table is one 64-bit constant).  p == 0 needs no M_k1 (k1 := k), and q == 0
// skips LDS altogether.
//
// Erosion is the same code on the complemented image (fill = 0xff: what lies outside the image is 255 after the
// complement, i.e. reads 0 for the minimum), the two maxima complemented back before the blend -- the blend's
// rounding is not symmetric under the complement.
//
// LDS.  Each wave owns STK_IMG words: the 784 H words in pixel order between two borders of 84 fill words (three
// image rows above and below; no side border is needed, a vertical tap keeps its column), so word (x, y + dy)
// of pixel n is linear word 84 + n + 28 dy and every tap is an unconditional read.  Linear word v lives at
// cell v + 4 (v >> 4): four pad words after every sixteen.  An aligned group of four words stays contiguous and
// 16-byte aligned, and the 49 lanes of one access, 16 words apart, become 20 cells apart: on the 64-bank model
// a 16-byte access is served 16 lanes at a time, and 20 l mod 64, l = 0..15, are the sixteen distinct multiples
// of 4 -- every bank once, for the H stores and for the reads at any dy (28 dy only shifts all lanes alike).
// The unpadded layout (stride 16) puts lanes l, l + 4, l + 8, l + 12 on the same banks: 4-way.
//
// Robustness.  |q| <= 768 after the clamp, so k1 <= 3 and the reads stay within linear words 0 .. 951; the
// rectangle is clipped with integer min / max (its far edge in 64 bits) and only ever clears bytes of the lane's
// own registers.  No parameter enters an address.
//
// A wave touches only its own region: no workgroup barrier, and the wavefront-scope fences around
// wave_barrier() that augment.hip explains.
#include "common.h"
#include "launchers.h"

namespace csed {
namespace {

constexpr int STK_SIDE = 28;             // image side
constexpr int STK_ROW = 784;             // bytes per row of src / dst, H words per image
constexpr int STK_WAVES = 4;             // images per workgroup
constexpr int STK_LANES = STK_ROW / 16;  // 49 lanes carry pixels
constexpr int STK_PAD = 3 * STK_SIDE;    // border words before and after the image
constexpr int STK_WORDS = STK_ROW + 2 * STK_PAD;  // linear words per wave
constexpr int STK_QMAX = 768;            // |q| <= 3 px in 1/256 px
constexpr uint64_t STK_STREAM = 1ull << 41;  // first Philox index of the stroke draws
// w_k(|dy|) as nibble |dy| of the 16-bit field k
constexpr uint64_t STK_SPANS = 0x0223001200010000ull;

__host__ __device__ constexpr int stk_cell(int v) { return v + ((v >> 4) << 2); }
constexpr int STK_IMG = stk_cell(STK_WORDS - 1) + 1;  // 1188 cells per wave
static_assert(STK_IMG % 4 == 0 && STK_PAD % 4 == 0, "16-byte LDS accesses need aligned regions");

__device__ __forceinline__ int uniform_i(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ int span_shift(int k, int ady) { return 8 * (int)((STK_SPANS >> (16 * k + 4 * ady)) & 15u); }

__global__ __launch_bounds__(STK_WAVES * kWave) void augment_stroke_kernel(
    const uint8_t* src, uint8_t* dst, const int64_t* __restrict__ idx, const int* __restrict__ params_in,
    int* __restrict__ params_out, int64_t N, int M, uint64_t seed, uint64_t epoch, float max_thickness,
    float erase_p, int erase_lo, int erase_hi) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[STK_WAVES * STK_IMG];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m = blockIdx.x * STK_WAVES + wave;  // wave-uniform: position in idx / params
  if (m >= M) return;
  const int64_t r = idx ? idx[m] : (int64_t)m;
  if (r < 0 || r >= N) return;  // an index outside the set: the row is skipped, nothing is written
  uint32_t* img = lds + wave * STK_IMG;

  // ---- the row's pixels: one uint4 per lane, issued before the parameters' arithmetic
  uint4 px = make_uint4(0, 0, 0, 0);
  if (lane < STK_LANES) px = *reinterpret_cast<const uint4*>(src + r * STK_ROW + 16 * lane);

  // ---- the parameters, once per wave
  int q, e, top, left, h, w;
  if (params_in) {
    const int* t = params_in + 6 * (int64_t)m;
    q = t[0], e = t[1], top = t[2], left = t[3], h = t[4], w = t[5];
  } else {
    // lane j < 8 draws u_j (the other lanes repeat them): one Philox pass of the wave for the six draws
    const float u = philox_uniform(seed, epoch, STK_STREAM + 8ull * (uint64_t)r + (uint64_t)(lane & 7));
    const int U = (int)(u * 16777216.0f);  // exact: u is a multiple of 2^-24 in [0, 1)
    const float t = (2.0f * __shfl(u, 0, kWave) - 1.0f) * max_thickness;  // (2 u - 1 is exact: one rounding)
    q = (int)floorf(fabsf(t) * 256.0f);
    q = t < 0.0f ? -q : q;
    e = __shfl(u, 1, kWave) < erase_p;
    const int n = erase_hi - erase_lo + 1;  // <= 28: U n < 2^29
    h = erase_lo + ((__shfl(U, 2, kWave) * n) >> 24);
    w = erase_lo + ((__shfl(U, 3, kWave) * n) >> 24);
    top = (__shfl(U, 4, kWave) * (STK_SIDE + 1 - h)) >> 24;
    left = (__shfl(U, 5, kWave) * (STK_SIDE + 1 - w)) >> 24;
  }
  q = uniform_i(min(max(q, -STK_QMAX), STK_QMAX));
  e = uniform_i(e), top = uniform_i(top), left = uniform_i(left), h = uniform_i(h), w = uniform_i(w);
  if (params_out && lane == 0) {
    int* t = params_out + 6 * (int64_t)m;
    t[0] = q, t[1] = e, t[2] = top, t[3] = left, t[4] = h, t[5] = w;
  }
  const int a = q < 0 ? -q : q, k = a >> 8, p = a & 255;
  const int k1 = p ? min(k + 1, 3) : k;  // (p == 0: M_k1 carries weight 0)
  const uint32_t fill = q < 0 ? 0xffffffffu : 0u;

  uint32_t out[4] = {px.x, px.y, px.z, px.w};
  if (k1 > 0) {
    // ---- horizontal pass in registers: the packed running maxima H_0..H_3 of the (complemented) row
    const uint32_t c[4] = {px.x ^ fill, px.y ^ fill, px.z ^ fill, px.w ^ fill};
    const uint32_t before = __shfl_up(c[3], 1, kWave), after = __shfl_down(c[0], 1, kWave);
    if (lane < 2 * STK_PAD / 4) {  // the two borders: 42 lanes, one 16-byte store each
      const int v = lane < STK_PAD / 4 ? 4 * lane : STK_PAD + STK_ROW + 4 * (lane - STK_PAD / 4);
      *reinterpret_cast<uint4*>(img + stk_cell(v)) = make_uint4(fill, fill, fill, fill);
    }
    if (lane < STK_LANES) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int x0 = (16 * lane + 4 * g) % STK_SIDE;  // the group's first column: 0, 4, .. 24
        const uint32_t L = x0 == 0 ? fill : g ? c[g - 1] : before;
        const uint32_t R = x0 == STK_SIDE - 4 ? fill : g < 3 ? c[g + 1] : after;
        uint32_t b[10];  // columns x0 - 3 .. x0 + 6
#pragma unroll
        for (int j = 0; j < 3; ++j) b[j] = (L >> (8 * (j + 1))) & 0xffu, b[7 + j] = (R >> (8 * j)) & 0xffu;
#pragma unroll
        for (int j = 0; j < 4; ++j) b[3 + j] = (c[g] >> (8 * j)) & 0xffu;
        uint32_t hw[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t h0 = b[3 + j];
          const uint32_t h1 = max(h0, max(b[2 + j], b[4 + j]));
          const uint32_t h2 = max(h1, max(b[1 + j], b[5 + j]));
          const uint32_t h3 = max(h2, max(b[j], b[6 + j]));
          hw[j] = h0 | (h1 << 8) | (h2 << 16) | (h3 << 24);
        }
        *reinterpret_cast<uint4*>(img + stk_cell(STK_PAD + 16 * lane + 4 * g)) = make_uint4(hw[0], hw[1], hw[2], hw[3]);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // ---- vertical pass: M_k and M_k1 of the lane's 16 pixels from 2 k1 + 1 rows of H words
    if (lane < STK_LANES) {
      uint32_t mk[16], mk1[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) mk[i] = mk1[i] = 0;
      for (int dy = -k1; dy <= k1; ++dy) {  // scalar bounds, 1 <= k1 <= 3
        const int ady = dy < 0 ? -dy : dy;
        const bool in_k = ady <= k;
        const int s1 = span_shift(k1, ady), s0 = in_k ? span_shift(k, ady) : 0;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const uint4 v = *reinterpret_cast<const uint4*>(img + stk_cell(STK_PAD + 16 * lane + 4 * g + STK_SIDE * dy));
          const uint32_t t[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            mk1[4 * g + j] = max(mk1[4 * g + j], (t[j] >> s1) & 0xffu);
            if (in_k) mk[4 * g + j] = max(mk[4 * g + j], (t[j] >> s0) & 0xffu);
          }
        }
      }
      const uint32_t fb = fill & 0xffu;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        uint32_t word = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t v = ((mk[4 * g + j] ^ fb) * (uint32_t)(256 - p) + (mk1[4 * g + j] ^ fb) * (uint32_t)p + 128u) >> 8;
          word |= v << (8 * j);
        }
        out[g] = word;
      }
    }
  }
  if (lane >= STK_LANES) return;

  // ---- erase: the clipped rectangle as a mask on the lane's 16 bytes
  if (e) {
    const int y0 = max(top, 0), y1 = (int)min((int64_t)top + (int64_t)h, (int64_t)STK_SIDE);
    const int x0 = max(left, 0), x1 = (int)min((int64_t)left + (int64_t)w, (int64_t)STK_SIDE);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int n = 16 * lane + 4 * g, y = n / STK_SIDE, x = n - y * STK_SIDE;
      uint32_t keep = 0xffffffffu;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (y >= y0 && y < y1 && x + j >= x0 && x + j < x1) keep &= ~(0xffu << (8 * j));
      out[g] &= keep;
    }
  }
  *reinterpret_cast<uint4*>(dst + r * STK_ROW + 16 * lane) = make_uint4(out[0], out[1], out[2], out[3]);
}

}  // namespace

hipError_t launch_augment_stroke(const uint8_t* src, uint8_t* dst, const int64_t* idx, const int* params_in,
                                 int* params_out, int64_t N, int64_t M, uint64_t seed, uint64_t epoch,
                                 float max_thickness, float erase_p, int erase_lo, int erase_hi, hipStream_t s) {
  if (M <= 0) return hipSuccess;
  hipLaunchKernelGGL(augment_stroke_kernel, dim3((unsigned)((M + STK_WAVES - 1) / STK_WAVES)),
                     dim3(STK_WAVES * kWave), 0, s, src, dst, idx, params_in, params_out, N, (int)M, seed, epoch,
                     max_thickness, erase_p, erase_lo, erase_hi);
  return hipGetLastError();
}

}  // namespace csed
