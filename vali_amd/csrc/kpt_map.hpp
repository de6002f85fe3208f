// A keypoint of a pose head in frame pixels, and whether it is visible (steps 2 and 3 of "pose skeletons" in
// include/vali_hip.h), shared by vali_pose_paint (pose.hip) and vali_warp_fit (warp.hip): one copy, so a keypoint the
// drawer shows is a keypoint the fit may use.  tests/pose_model.py (map_axis, row_points) restates it in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#pragma clang fp contract(off)

namespace vali {
namespace {

// step 3: a visible keypoint has -65536 <= fx < 131072
constexpr float kLoF = -65536.0f, kHiF = 131072.0f;

// step 2 along one axis: one rounding per operation
__device__ __forceinline__ float map_axis(float v, int dst, int src_n, int dst_n, int src) {
  const float scale = __fdiv_rn((float)src_n, (float)dst_n);
  return __fadd_rn(__fmul_rn(__fsub_rn(v, (float)dst), scale), (float)src);
}

// step 3 (a NaN fails every comparison; fabsf(v) < inf: v is finite)
__device__ __forceinline__ bool kpt_visible(float conf, float thr, float kx, float ky, float fx, float fy) {
  return conf > thr && fabsf(kx) < INFINITY && fabsf(ky) < INFINITY && fx >= kLoF && fx < kHiF && fy >= kLoF && fy < kHiF;
}

} // namespace
} // namespace vali
