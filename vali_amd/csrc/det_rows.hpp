// What the painters that read vali_detect_select's dets rows on the device share (vali_mask_paint in mask.hip,
// vali_pose_paint in pose.hip): a row's eight values and step 1 of both definitions in include/vali_hip.h -- which rows
// are drawn, and the box clipped to the frame.  One copy, so a row the masker skips is a row the pose drawer skips.
#pragma once
#include "tile_paint.hpp"

namespace vali {
namespace {

__device__ __forceinline__ void load_row(const int32_t* dets, int i, int (&r)[8]) {
  const uint4 a = load16_u((const uint8_t*)(dets + (size_t)i * 8)), b = load16_u((const uint8_t*)(dets + (size_t)i * 8) + 16);
  r[0] = (int)a.x, r[1] = (int)a.y, r[2] = (int)a.z, r[3] = (int)a.w;
  r[4] = (int)b.x, r[5] = (int)b.y, r[6] = (int)b.z, r[7] = (int)b.w;
}

// step 1 of the definition; the box clipped to the W x H frame
struct Row {
  int x0, y0, x1, y1;
  int cls, k;
};
__device__ __forceinline__ bool resolve_row(const int (&r)[8], int f, int W, int H, int K, const vali_roi& rc, Row& o) {
  if (r[0] != f || r[3] < 1 || r[4] < 1 || r[7] < 0 || r[7] >= K)
    return false;
  if (rc.src_w < 1 || rc.src_h < 1 || rc.dst_w < 1 || rc.dst_h < 1)
    return false;
  // 64 bits: x + w overflows int32
  const long long x0 = r[1], y0 = r[2], x1 = x0 + r[3], y1 = y0 + r[4];
  if (x0 >= W || y0 >= H || x1 <= 0 || y1 <= 0)
    return false;
  o.x0 = clampi(x0, 0, W), o.y0 = clampi(y0, 0, H), o.x1 = clampi(x1, 0, W), o.y1 = clampi(y1, 0, H);
  o.cls = r[5], o.k = r[7];
  return true;
}
// the same box for a row that is known to pass
__device__ __forceinline__ void clip_box(const int (&r)[8], int W, int H, Row& o) {
  const long long x0 = r[1], y0 = r[2], x1 = x0 + r[3], y1 = y0 + r[4];
  o.x0 = clampi(x0, 0, W), o.y0 = clampi(y0, 0, H), o.x1 = clampi(x1, 0, W), o.y1 = clampi(y1, 0, H);
  o.cls = r[5], o.k = r[7];
}

} // namespace
} // namespace vali
