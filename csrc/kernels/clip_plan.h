// Which form and grid a global-norm gradient clip of n floats gets (kernels/clip.hip): decided here and
// nowhere else.  The launcher dispatches on clip_plan(), the op (bindings.cpp) reports its message and sizes
// its checks from it, and Python asks through csed::clip_plan (optim/clip.py).  Plain scalar logic: no HIP
// call, no environment, no allocation.
#pragma once
#include <stdint.h>

namespace csed {

constexpr int kClipThreads = 1024;  // threads of every clip workgroup (16 waves)
// float4s one thread of the one-workgroup form keeps in registers between the reduction and the scale
// (32 VGPRs of gradient: the whole workgroup still fits one CU at full width)
constexpr int kClipQuadsPerThread = 8;
// largest n of the one-workgroup form: 32,768 floats (LeNet's 21,840 come to 6 float4s per thread)
constexpr int64_t kClipOneWgMax = (int64_t)kClipThreads * kClipQuadsPerThread * 4;
constexpr int kClipMaxGrid = 1024;          // most workgroups (= partial sums) of the two-launch form
constexpr int kClipQuadsPerThreadLarge = 4; // two-launch form: float4s per thread before the grid stops growing

static_assert(kClipOneWgMax >= 21840, "the one-workgroup form covers LeNet's flat gradient");

struct ClipPlan {
  int form;            // 0: clip_one_wg_kernel (one launch), 1: clip_sqnorm_partials + clip_scale
  int grid;            // workgroups of each launch
  int partials;        // floats of the partial-sum buffer the form needs (0: none)
  int64_t chunk;       // form 1: float4s per workgroup (workgroup b owns quads [b * chunk, (b + 1) * chunk))
  const char* error;   // null, or why there is no launch
};

// The plan is a function of n alone, so the order of the sum is too.
inline ClipPlan clip_plan(int64_t n) {
  ClipPlan p = {0, 1, 0, 0, nullptr};
  if (n < 1) {
    p.error = "clip_grad_norm_: the gradient needs at least one element";
    return p;
  }
  if (n <= kClipOneWgMax) return p;
  const int64_t quads = n / 4, per_wg = (int64_t)kClipThreads * kClipQuadsPerThreadLarge;
  const int64_t want = (quads + per_wg - 1) / per_wg;
  p.form = 1;
  p.grid = (int)(want < kClipMaxGrid ? want : kClipMaxGrid);
  p.partials = p.grid;
  p.chunk = (quads + p.grid - 1) / p.grid;
  return p;
}

}  // namespace csed
