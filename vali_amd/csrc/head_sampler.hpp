// The bilinear sampler of a network head's planes at frame pixels (step 3 of "instance masks" in include/vali_hip.h),
// shared by vali_mask_paint (mask.hip) and vali_semantic_paint (semantic.hip): one copy, so the two cannot drift.
// tests/mask_model.py (taps) restates it in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#pragma clang fp contract(off)

namespace vali {
namespace {

// step 3 of the definition along one axis
struct Axis {
  float src, scale, dst, k;
  int P;
};
__device__ __forceinline__ Axis make_axis(int src, int src_n, int dst, int dst_n, int P, int net) {
  Axis a;
  a.src = (float)src, a.scale = __fdiv_rn((float)dst_n, (float)src_n), a.dst = (float)dst;
  a.k = __fdiv_rn((float)P, (float)net);
  a.P = P;
  return a;
}
struct Tap {
  int i0, i1;
  float t;
};
__device__ __forceinline__ Tap axis_tap(const Axis& a, int px) {
  const float g = __fadd_rn(__fmul_rn(__fsub_rn(__fadd_rn((float)px, 0.5f), a.src), a.scale), a.dst);
  const float f = __fsub_rn(__fmul_rn(g, a.k), 0.5f);
  float x0 = floorf(f);
  Tap t;
  t.t = __fsub_rn(f, x0);
  x0 = fminf(fmaxf(x0, -1.0f), (float)a.P);
  const int i = (int)x0;
  t.i0 = min(max(i, 0), a.P - 1), t.i1 = min(max(i + 1, 0), a.P - 1);
  return t;
}

} // namespace
} // namespace vali
