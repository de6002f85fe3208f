// The annotator rows of one detection, as vali_detect_select (detect.hip) and vali_track_update (track.hip) write them
// into `marks` (include/vali_hip.h): the outline at row `at`, the label's background at M + at and its text at 2 M + at.
// One copy, so a tracked box is drawn exactly as the detection it came from; the two differ only in what picks the colour
// and the label (the class there, the track's id here).
#pragma once
#include <stdint.h>

#include "../../include/vali_hip.h"

namespace vali {
namespace {

struct MarkStyle {
  int32_t* marks;
  const int32_t *colours, *label_rects;
  int n_colours, n_labels, thickness, label_alpha, text_colour;
};

__device__ __forceinline__ void put_row(int32_t* p, int v0, int v1, int v2, int v3, int v4, int v5, int v6, int v7) {
  p[0] = v0, p[1] = v1, p[2] = v2, p[3] = v3, p[4] = v4, p[5] = v5, p[6] = v6, p[7] = v7;
}

// `colour`: an index below n_colours; `label`: an index below n_labels, or -1 for a detection without a label.  Neither
// is looked at when !used: the rows are then all zero.
__device__ __forceinline__ void put_marks(const MarkStyle& s, int M, int at, bool used, int f, int x, int y, int w, int h,
                                          int colour, int label) {
  const int c = used ? s.colours[colour] : 0;
  if (used)
    put_row(s.marks + (size_t)at * 8, f, x, y, w, h, VALI_MARK_BOX, s.thickness, c);
  else
    put_row(s.marks + (size_t)at * 8, 0, 0, 0, 0, 0, 0, 0, 0);
  if (s.label_rects) {
    int32_t* bg = s.marks + ((size_t)M + at) * 8;
    int32_t* tx = s.marks + ((size_t)2 * M + at) * 8;
    if (used && label >= 0) {
      const int32_t* lr = s.label_rects + (size_t)label * 4;
      const int u = lr[0], v = lr[1], lw = lr[2], lh = lr[3];
      const int ly = (int)((uint32_t)y - (uint32_t)lh);
      put_row(bg, f, x, ly, lw, lh, VALI_MARK_FILL, 0, (int)(((uint32_t)c & 0x00FFFFFFu) | ((uint32_t)s.label_alpha << 24)));
      put_row(tx, f, x, ly, lw, lh, VALI_MARK_STAMP, (int)((uint32_t)u | ((uint32_t)v << 16)), s.text_colour);
    } else {
      put_row(bg, 0, 0, 0, 0, 0, 0, 0, 0);
      put_row(tx, 0, 0, 0, 0, 0, 0, 0, 0);
    }
  }
}

} // namespace
} // namespace vali
