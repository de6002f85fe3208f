// Pose skeletons (vali_pose_paint): the keypoints of a pose head's detections -- gathered by the detection's k, mapped
// back through the letterbox to frame pixels -- written out as points and drawn as limbs (capsules) and joints (discs)
// IN PLACE onto a batch of NV12, YUV420, YUV444, RGB, BGR or RGB_PLANAR frames, from detections that live in DEVICE
// memory (vali_detect_select's dets).
//
// Definition: include/vali_hip.h ("pose skeletons"); tests/pose_model.py restates it in numpy.
//
// Two launches, whatever the data:
//   k_pose_points<DT>  one wave per dets row, lane p = keypoint p (P <= 64).  Writes the row's points (all zero for a
//                      skipped row) and, reduced over the wave, the bounding box of the visible keypoints grown by half
//                      the larger of thickness and diameter and clipped to the frame: the row's box in the workspace (an
//                      empty one for a row that draws nothing).
//   k_pose_paint<FMT>  k_mask_paint's structure: a workgroup owns one 64 x 64 luma tile of one frame, culls its frame's
//                      max_det rows by their boxes into an LDS hit list (in row order) and, with no hit, leaves without
//                      touching a pixel.  The hits are taken 256 / (L + P) at a time: a lane forms one shape of one hit
//                      (limb j, then joint j - L) from the row's points -- its integers, its colour and whether its own
//                      box meets the tile -- and the shapes that do are compacted in drawing order.  Every lane then
//                      applies them to its 16-byte pieces in registers with cover_piece, the coverage computed per
//                      pixel in exact integers, and stores a piece only if a shape changed it.  The pieces are loaded
//                      once a pass has a shape on the tile.
// vali_pose_paint_points draws points the caller holds: k_pose_boxes in the place of k_pose_points, then the same
// k_pose_paint.
// The formats and the frame rules, the tile's pieces, the hit list and the coverage blend are tile_paint.hpp's, the rows
// det_rows.hpp's; here are the points, the shapes and their coverage.
#include <math.h>

#include "det_rows.hpp"
#include "kpt_map.hpp"
#include "tensor_in.hpp"

#pragma clang fp contract(off)

namespace vali {
namespace {

constexpr int kMaxN = 1024, kMaxK = 1 << 20, kMaxD = 1024, kMaxP = 64, kMaxL = 128, kMaxT = 64;
static_assert(kMaxL + kMaxP <= kBlock, "a lane for every shape of a hit");

struct PoseArgs {
  const vali_surface* d_frames;
  const int32_t* dets;
  const vali_roi* rects;
  const int32_t* limbs;  // L pairs
  const int32_t* limb_colours;
  const int32_t* joint_colours;
  const void* kpts;
  int4* points;  // n * D * P rows X, Y, conf bits, flag
  int4* boxes;   // n * D row boxes x0, y0, x1, y1
  long long sn, sk, sp, sc;  // element strides of kpts
  int dt, kdim;
  int n, D, K, P, L;
  int n_limb_colours, n_joint_colours;
  int thickness, diameter, alpha;
  float thr;
  float m[3][4];  // rgb2yuv rows (YUV formats)
};

// ---- launch 1: the points and the box of a row (the mapping and the visibility rule: kpt_map.hpp) -----------------------
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1)
    v = min(v, __shfl_xor(v, d));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1)
    v = max(v, __shfl_xor(v, d));
  return v;
}

template <int DT>
__global__ void __launch_bounds__(kBlock) k_pose_points(const PoseArgs a) {
  typedef TensorElem<DT> E;
  typedef typename E::Bits Bits;
  const int lane = threadIdx.x & (kWave - 1);
  const int row = (int)blockIdx.x * kWavesPerBlock + (int)threadIdx.x / kWave;
  if (row >= a.n * a.D)
    return;
  const int f = row / a.D;
  int r[8];
  load_row(a.dets, row, r);
  const int W = a.d_frames[f].width, H = a.d_frames[f].height;
  const vali_roi rc = a.rects[f];
  int4* out = a.points + (size_t)row * (size_t)a.P;
  Row o;
  if (!resolve_row(r, f, W, H, a.K, rc, o)) {
    if (lane < a.P)
      out[lane] = make_int4(0, 0, 0, 0);
    if (lane == 0)
      a.boxes[row] = make_int4(0, 0, 0, 0);
    return;
  }
  int X = 0, Y = 0, flag = 0;
  float conf = 1.0f;
  if (lane < a.P) {
    const Bits* p = (const Bits*)a.kpts + (long long)f * a.sn + (long long)o.k * a.sk + (long long)lane * a.sp;
    const float kx = E::f((u32)p[0]), ky = E::f((u32)p[a.sc]);
    if (a.kdim == 3)
      conf = E::f((u32)p[2 * a.sc]);
    const float fx = map_axis(kx, rc.dst_x, rc.src_w, rc.dst_w, rc.src_x);
    const float fy = map_axis(ky, rc.dst_y, rc.src_h, rc.dst_h, rc.src_y);
    const bool vis = kpt_visible(conf, a.thr, kx, ky, fx, fy);
    if (vis) {
      X = (int)floorf(fx), Y = (int)floorf(fy);
      flag = (X >= 0 && X < W && Y >= 0 && Y < H) ? 3 : 1;
    }
    out[lane] = make_int4(X, Y, __float_as_int(conf), flag);
  }
  // the box of everything the row can draw: every shape lies within floor(max(t, d) / 2) of a visible keypoint
  const int big = 1 << 30;
  const int x0 = wave_min(flag ? X : big), y0 = wave_min(flag ? Y : big);
  const int x1 = wave_max(flag ? X : -big), y1 = wave_max(flag ? Y : -big);
  if (lane == 0) {
    const int g = (max(a.thickness, a.diameter) + 1) / 2;
    int4 b = make_int4(0, 0, 0, 0);
    if (x0 <= x1) {
      b = make_int4(clampi((long long)x0 - g, 0, W), clampi((long long)y0 - g, 0, H), clampi((long long)x1 + g + 1, 0, W),
                    clampi((long long)y1 + g + 1, 0, H));
      if (b.x >= b.z || b.y >= b.w)
        b = make_int4(0, 0, 0, 0);
    }
    a.boxes[row] = b;
  }
}

// ---- launch 2: the tiles ------------------------------------------------------------------------------------------------
// One shape as the pieces see it: the segment A, A + e (e = 0: a disc), the largest |c| and |q|^2 step 4 lets in, and its
// box.  Everything is the same in every lane.
struct Shape {
  int ax, ay, ex, ey;
  long long L2;
  int cmax;  // the largest |c| with 4 c^2 <= t^2 L2
  int r2;    // the largest |q|^2 with 4 |q|^2 <= t^2
  int rx0, ry0, rx1, ry1;
};

// the largest r with r * r <= v, 0 <= v < 2^62
__device__ __forceinline__ long long isqrt64(long long v) {
  long long r = (long long)sqrt((double)v);
  while (r * r > v)
    --r;
  while ((r + 1) * (r + 1) <= v)
    ++r;
  return r;
}

// |q|^2 <= r2 for r2 <= 1024, whatever the size of q: a component beyond 64 alone is outside
__device__ __forceinline__ bool in_disc(int dx, u32 ady2, int r2) {
  const u32 adx = (u32)min(abs(dx), 64);
  return adx * adx + ady2 <= (u32)r2;
}

// The coverage (255 in the shape, 0 outside) of the N (16, or 6 for a packed RGB piece) frame pixels X .. X + N - 1 of
// frame row py, a byte each: step 4 of the definition.  s and c are linear in the pixel: they are formed once in 64 bits
// for the run's first pixel.  The whole capsule has |c| <= cmax (its caps too: |q| <= t / 2 there), and c is monotone
// along the row, so a run whose two ends are beyond cmax on the same side holds no pixel of the shape.
template <int N>
__device__ __forceinline__ void shape_cov(const Shape& h, int X, int py, u32 (&cv)[N == 16 ? 4 : 2]) {
  constexpr int NW = N == 16 ? 4 : 2;
#pragma unroll
  for (int w = 0; w < NW; ++w)
    cv[w] = 0u;
  const int lo = max(h.rx0 - X, 0), hi = min(h.rx1 - X, N);
  if (py < h.ry0 || py >= h.ry1 || lo >= hi)
    return;
  const int qx = X - h.ax, qy = py - h.ay;
  const long long s0 = (long long)qx * h.ex + (long long)qy * h.ey;
  const long long c0 = (long long)qx * h.ey - (long long)qy * h.ex;
  const long long cl = c0 + (long long)lo * h.ey, ch = c0 + (long long)(hi - 1) * h.ey;
  if ((cl > h.cmax && ch > h.cmax) || (cl < -(long long)h.cmax && ch < -(long long)h.cmax))
    return;
  // Along the run s, s - L2 and c move by at most 15 |e| < 2^22, so 32 bits do for the pixels: a start beyond +-2^23
  // keeps its sign over the run, and a c beyond +-2^26 stays beyond cmax < 2^24.
  const int sa = clampi(s0, -(1 << 23), 1 << 23), ua = clampi(s0 - h.L2, -(1 << 23), 1 << 23);
  const int ca = clampi(c0, -(1 << 26), 1 << 26);
  const u32 cm = (u32)h.cmax;
  // s and s - L2 are monotone along the run: with both ends between the caps, every pixel of it is
  const bool between = h.L2 != 0 && min(sa + lo * h.ex, sa + (hi - 1) * h.ex) > 0 &&
                       max(ua + lo * h.ex, ua + (hi - 1) * h.ex) < 0;
  const u32 aqy = (u32)min(abs(qy), 64), aby = (u32)min(abs(qy - h.ey), 64);
  const u32 aqy2 = aqy * aqy, aby2 = aby * aby;
  const bool point = h.L2 == 0;
  // Selects, not branches, and a word of four pixels finished before the next is begun (the fence below): scheduled across
  // all sixteen pixels, the two rows a 4:2:0 chroma piece asks for held 50 more registers (NV12: 139 VGPRs, 3 waves).
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    u32 word = 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int k = 4 * w + b;
      if (k < N) {
        bool in = (u32)(ca + k * h.ey) + cm <= 2u * cm;
        if (!between) {
          const bool cap_a = point || sa + k * h.ex <= 0, cap_b = ua + k * h.ex >= 0;
          const bool disc = in_disc(cap_a ? qx + k : qx + k - h.ex, cap_a ? aqy2 : aby2, h.r2);
          in = (cap_a || cap_b) ? disc : in;
        }
        word |= in ? 0xffu << (8 * b) : 0u;
      }
    }
    // the bytes of pixels lo .. hi - 1
    const int l = min(max(lo - 4 * w, 0), 4), r = min(max(hi - 4 * w, 0), 4);
    cv[w] = word & (u32)(((1ull << (8 * r)) - 1ull) & ~((1ull << (8 * l)) - 1ull));
    __builtin_amdgcn_sched_barrier(0);
  }
}

// a shape as cover_piece's coverage source (tile_paint.hpp)
struct ShapeCov : Shape {
  template <int N>
  __device__ __forceinline__ void get(int X, int py, u32 (&cv)[N == 16 ? 4 : 2]) const {
    shape_cov<N>(*this, X, py, cv);
  }
};

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// compact_put (tile_paint.hpp) from 0 with the wave's number as a scalar: called inside the drawing loop, compact_put's
// lane comparisons w < wave were kept across the loop as pairs of scalar registers, and scalars spilled
__device__ __forceinline__ int compact_lanes(bool flag, int value, uint16_t* out, int* wtot) {
  const int lane = threadIdx.x & (kWave - 1), wave = uni((int)threadIdx.x / kWave);
  const unsigned long long b = __ballot(flag);
  const int before = __popcll(b & ((1ull << lane) - 1ull));
  wtot[wave] = __popcll(b);  // (every lane of the wave, the same value: a lane == 0 would be one more pair)
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kWavesPerBlock; ++w) {
    const int c = wtot[w];
    off += w < wave ? c : 0;
    tot += c;
  }
  if (flag)
    out[off + before] = (uint16_t)value;
  __syncthreads();
  return tot;
}

template <int FMT>
__global__ void __launch_bounds__(kBlock) k_pose_paint(const PoseArgs a) {
  __shared__ uint16_t hits[kMaxD];
  __shared__ uint16_t shp[kBlock];
  __shared__ int wtot[kWavesPerBlock];
  // the shapes of a pass, of two passes in turn: a wave may form the next pass's while another still draws this one's
  __shared__ int4 seg[2][kBlock];  // ax, ay, ex, ey
  // L2's low word; its high bits (8), the largest |q|^2 of a cap (12) and the shape's reach (6); cmax; the colour's three
  // channels and its alpha
  __shared__ int4 lim[2][kBlock];
  constexpr int NS = nslots(FMT);

  const int f = blockIdx.y;
  const vali_surface* d = a.d_frames + f;
  const int W = d->width, H = d->height;
  const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
  if ((int)blockIdx.x >= tiles_x * tiles_y)
    return;  // the grid is sized for the batch's largest frame
  const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
  const int tx0 = tx * kTile, ty0 = ty * kTile;
  const int tx1 = min(tx0 + kTile, W), ty1 = min(ty0 + kTile, H);
  const int tid = threadIdx.x;

  // A pass takes `per` hits: lane slot * nshapes + j forms shape j (limbs in table order, then joints) of the pass's
  // hit `slot`, so lane order is drawing order.  What a lane needs of the tables does not change from pass to pass, and
  // is asked for here, so that it arrives while the rows are culled.
  const int nshapes = a.L + a.P;
  const int per = kBlock / nshapes;
  const int slot = tid / nshapes, j = tid - slot * nshapes;
  const bool limb = j < a.L;
  const int t = limb ? a.thickness : a.diameter;
  const int hr = t / 2;  // how far the shape reaches from its segment
  // the tile grown by that reach: a segment whose box misses it has no pixel on the tile
  const int mx0 = tx0 - hr, mx1 = tx1 + hr, my0 = ty0 - hr, my1 = ty1 + hr;
  int ia = j - a.L, ib = ia;
  u32 colour = 0u;
  if (slot < per) {
    if (limb) {
      ia = a.limbs[2 * j], ib = a.limbs[2 * j + 1];
      colour = (u32)a.limb_colours[j % a.n_limb_colours];
    } else {
      colour = (u32)a.joint_colours[ia % a.n_joint_colours];
    }
  }

  // the frame's rows whose box (launch 1) meets this tile, in row order
  int nh = 0;
  for (int base = 0; base < a.D; base += kBlock) {
    const int i = base + tid;
    bool flag = false;
    if (i < a.D) {
      const int4 b = a.boxes[f * a.D + i];
      flag = b.x < b.z && b.x < tx1 && b.z > tx0 && b.y < ty1 && b.w > ty0;
    }
    nh = compact_put(flag, i, hits, nh, wtot);
  }
  if (nh == 0)
    return;

  u32 pk = 0u;  // the colour's three channels as the format stores them, and its alpha
  bool valid = false;
  const int4 *pa = a.points, *pb = a.points;  // the lane's two keypoints in row 0 of the frame
  if (slot < per) {
    // (a pair outside 0 .. P - 1 draws nothing: the table is device memory, so the host cannot refuse it)
    valid = (unsigned)ia < (unsigned)a.P && (unsigned)ib < (unsigned)a.P;
    if (valid) {
      pa = a.points + (size_t)(f * a.D) * (size_t)a.P + ia;
      pb = a.points + (size_t)(f * a.D) * (size_t)a.P + ib;
    }
    const u32 alpha = a.alpha >= 0 ? (u32)a.alpha : colour >> 24;
    const u32 cr = (colour >> 16) & 0xffu, cg = (colour >> 8) & 0xffu, cb = colour & 0xffu;
    u32 c0, c1, c2;
    if constexpr (a_isyuv(FMT)) {
      const float fr = (float)cr, fg = (float)cg, fb = (float)cb;
      c0 = quantize_u8(dot_rgb(a.m[0], fr, fg, fb)), c1 = quantize_u8(dot_rgb(a.m[1], fr, fg, fb));
      c2 = quantize_u8(dot_rgb(a.m[2], fr, fg, fb));
    } else if constexpr (FMT == A_BGR) {
      c0 = cb, c1 = cg, c2 = cr;
    } else {
      c0 = cr, c1 = cg, c2 = cb;
    }
    pk = c0 | c1 << 8 | c2 << 16 | alpha << 24;
  }

  // one pass: the lanes form their shapes of the hits base .. base + per - 1 into seg[buf] / lim[buf]; returns how many
  // meet the tile, their lanes in shp[] in drawing order
  const auto form = [&](int base, int buf) -> int {
    bool meets = false;
    if (valid && base + slot < nh) {
      const size_t row = (size_t)(int)hits[base + slot] * (size_t)a.P;
      const int4 A = pa[row], B = pb[row];
      if (A.w != 0 && B.w != 0) {
        meets = min(A.x, B.x) < mx1 && max(A.x, B.x) >= mx0 && min(A.y, B.y) < my1 && max(A.y, B.y) >= my0;
        if (meets) {
          const int ex = B.x - A.x, ey = B.y - A.y;
          const long long L2 = (long long)ex * ex + (long long)ey * ey;
          // 4 c^2 <= t^2 L2  <=>  |c| <= isqrt(t^2 L2 / 4) < 2^24: t^2 L2 < 2^49
          const int cmax = (int)isqrt64(((long long)(t * t) * L2) >> 2);
          seg[buf][tid] = make_int4(A.x, A.y, ex, ey);
          lim[buf][tid] = make_int4((int)(u32)L2, (int)(L2 >> 32) | (t * t / 4) << 8 | hr << 20, cmax, (int)pk);
        }
      }
    }
    return compact_lanes(meets, tid, shp, wtot);
  };

  // the first pass with a shape on the tile; without one the tile is not read
  int base = 0, buf = 0, ns = 0;
  for (; base < nh; base += per, buf ^= 1) {
    ns = form(base, buf);
    if (ns != 0)
      break;
  }
  if (ns == 0)
    return;

  // (the pieces are loaded here, not at the first shape inside the loop below: there, every lane condition of
  // load_piece was hoisted in front of the loop as a pair of scalar registers, and 56 to 101 scalars spilled)
  Piece pc[NS];
  u32 cur[NS][4], orig[NS][4];
#define VALI_SLOT(S) load_piece<FMT, S>(d, tid, tx0, ty0, W, H, pc[S], cur[S], orig[S]);
  VALI_SLOTS(VALI_SLOT)
#undef VALI_SLOT

  for (;;) {
    for (int si = 0; si < ns; ++si) {
      const int e = (int)shp[si];
      const int4 sg = seg[buf][e], lm = lim[buf][e];
      ShapeCov h;
      h.ax = sg.x, h.ay = sg.y, h.ex = sg.z, h.ey = sg.w;
      const u32 ly = (u32)lm.y;
      h.L2 = (long long)(((unsigned long long)(ly & 0xffu) << 32) | (unsigned long long)(u32)lm.x);
      h.cmax = lm.z;
      h.r2 = (int)((ly >> 8) & 0xfffu);
      const int reach = (int)(ly >> 20);
      // (not clipped to the frame: the bytes of a piece beyond the frame's edge are never stored)
      h.rx0 = min(h.ax, h.ax + h.ex) - reach, h.rx1 = max(h.ax, h.ax + h.ex) + reach + 1;
      h.ry0 = min(h.ay, h.ay + h.ey) - reach, h.ry1 = max(h.ay, h.ay + h.ey) + reach + 1;
      const u32 cpk = (u32)lm.w;
      const u32 col[3] = {cpk & 0xffu, (cpk >> 8) & 0xffu, (cpk >> 16) & 0xffu};
      const u32 alpha = cpk >> 24;
#define VALI_SLOT(S) cover_piece<FMT, S>(h, pc[S], col, alpha, cur[S]);
      VALI_SLOTS(VALI_SLOT)
#undef VALI_SLOT
    }
    base += per, buf ^= 1;
    if (base >= nh)
      break;
    ns = form(base, buf);
  }

  // only what a shape changed goes back
#define VALI_SLOT(S) store_piece(pc[S], cur[S], orig[S]);
  VALI_SLOTS(VALI_SLOT)
#undef VALI_SLOT
}
#undef VALI_SLOTS

// ---- vali_pose_paint_points' launch 1: the caller's points, sanitised into the workspace, and the box of a row ----------
// One wave per row, lane p = point p, as k_pose_points: a point is visible when flag & 1 and -65536 <= X, Y < 131072, for
// every int32 value; the copy k_pose_paint reads keeps X, Y and the third value of a visible point and flag 0 / 1 / 3 (3:
// inside the frame, formed here), and is all zero for any other.  (Its own arguments: PoseArgs, and with it what
// vali_pose_paint compiles to, stays as it is.)
struct BoxArgs {
  const vali_surface* d_frames;
  const int4* src;  // n * D * P rows, the caller's
  int4* points;     // the workspace's copy
  int4* boxes;
  int n, D, P;
  int thickness, diameter;
};

__global__ void __launch_bounds__(kBlock) k_pose_boxes(const BoxArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int row = (int)blockIdx.x * kWavesPerBlock + (int)threadIdx.x / kWave;
  if (row >= a.n * a.D)
    return;
  const int f = row / a.D;
  const int W = a.d_frames[f].width, H = a.d_frames[f].height;
  int X = 0, Y = 0, flag = 0;
  if (lane < a.P) {
    const int4 p = a.src[(size_t)row * (size_t)a.P + lane];
    const int lo = -65536, hi = 131072;
    int4 o = make_int4(0, 0, 0, 0);
    if ((p.w & 1) && p.x >= lo && p.x < hi && p.y >= lo && p.y < hi) {
      X = p.x, Y = p.y;
      flag = (X >= 0 && X < W && Y >= 0 && Y < H) ? 3 : 1;
      o = make_int4(X, Y, p.z, flag);
    }
    a.points[(size_t)row * (size_t)a.P + lane] = o;
  }
  const int big = 1 << 30;
  const int x0 = wave_min(flag ? X : big), y0 = wave_min(flag ? Y : big);
  const int x1 = wave_max(flag ? X : -big), y1 = wave_max(flag ? Y : -big);
  if (lane == 0) {
    const int g = (max(a.thickness, a.diameter) + 1) / 2;
    int4 b = make_int4(0, 0, 0, 0);
    if (x0 <= x1) {
      b = make_int4(clampi((long long)x0 - g, 0, W), clampi((long long)y0 - g, 0, H), clampi((long long)x1 + g + 1, 0, W),
                    clampi((long long)y1 + g + 1, 0, H));
      if (b.x >= b.z || b.y >= b.w)
        b = make_int4(0, 0, 0, 0);
    }
    a.boxes[row] = b;
  }
}

bool dims_ok(int n, int D, int p) {
  return n >= 1 && n <= kMaxN && D >= 1 && D <= kMaxD && (long long)n * D <= 65535 && p >= 1 && p <= kMaxP;
}

void launch_paint(int fmt, const dim3& grid, hipStream_t s, const PoseArgs& a) {
  with_tile_format(fmt, [&](auto f) { hipLaunchKernelGGL(k_pose_paint<f>, grid, dim3(kBlock), 0, s, a); });
}

} // namespace
} // namespace vali

using namespace vali;

extern "C" {

size_t vali_pose_workspace_size(int n, int max_det, int p) {
  if (!dims_ok(n, max_det, p))
    return 0;
  return (size_t)n * (size_t)max_det * (size_t)(1 + p) * 16u;
}

int vali_pose_paint(const vali_surface* frames, const vali_surface* d_frames, int n, int format, const vali_pose_in* in,
                    const int32_t* d_dets, const vali_roi* d_rects, const vali_pose_style* style, int32_t* d_points,
                    const vali_cvt_params* params, void* d_ws, size_t ws_bytes, vali_stream_t stream) {
  VALI_REQUIRE(frames && d_frames && in && d_dets && d_rects && style && d_ws, "null argument");
  VALI_REQUIRE(n >= 1 && n <= kMaxN, "n outside 1..1024");
  VALI_REQUIRE(in->k >= 1 && in->k <= kMaxK, "k outside 1..2^20");
  VALI_REQUIRE(in->p >= 1 && in->p <= kMaxP, "p outside 1..64");
  VALI_REQUIRE(in->kdim == 2 || in->kdim == 3, "kdim is neither 2 nor 3");
  VALI_REQUIRE(in->max_det >= 1 && in->max_det <= kMaxD, "max_det outside 1..1024");
  VALI_REQUIRE((long long)n * in->max_det <= 65535, "n * max_det exceeds 65535");
  VALI_REQUIRE(in->n_limbs >= 0 && in->n_limbs <= kMaxL, "n_limbs outside 0..128");
  VALI_REQUIRE(in->d_limbs || in->n_limbs == 0, "limbs has a null pointer");
  const int64_t strides[4] = {in->stride_n, in->stride_k, in->stride_p, in->stride_c};
  int rc = check_head_tensor(__func__, "kpts", in->kpts, in->dtype, strides, 4);
  if (rc != VALI_OK)
    return rc;
  VALI_REQUIRE(style->d_limb_colours && style->d_joint_colours, "limb_colours or joint_colours has a null pointer");
  VALI_REQUIRE(style->n_limb_colours >= 1 && style->n_joint_colours >= 1, "n_limb_colours or n_joint_colours below 1");
  VALI_REQUIRE(style->kpt_thr == style->kpt_thr, "kpt_thr is a NaN");
  VALI_REQUIRE(style->thickness >= 1 && style->thickness <= kMaxT, "thickness outside 1..64");
  VALI_REQUIRE(style->diameter >= 1 && style->diameter <= kMaxT, "diameter outside 1..64");
  VALI_REQUIRE(style->alpha >= -1 && style->alpha <= 255, "alpha outside -1..255");
  VALI_REQUIRE((((uintptr_t)d_dets | (uintptr_t)d_rects | (uintptr_t)style->d_limb_colours |
                 (uintptr_t)style->d_joint_colours | (uintptr_t)in->d_limbs) & 3u) == 0,
               "dets, rects, limbs or colours are not 4-byte aligned");
  VALI_REQUIRE(((uintptr_t)d_points & 15u) == 0, "points is not 16-byte aligned");
  int tiles = 0;
  rc = check_frames(__func__, n, frames, format, &tiles);
  if (rc != VALI_OK)
    return rc;
  const int fmt = tile_format(format);
  VALI_REQUIRE(params || !a_isyuv(fmt), "a YUV format needs params (rgb2yuv)");
  VALI_REQUIRE(((uintptr_t)d_ws & 15u) == 0, "the workspace is not 16-byte aligned");
  VALI_REQUIRE(ws_bytes >= vali_pose_workspace_size(n, in->max_det, in->p),
               "the workspace is smaller than vali_pose_workspace_size");

  PoseArgs a = {};
  a.d_frames = d_frames, a.dets = d_dets, a.rects = d_rects, a.limbs = in->d_limbs;
  a.limb_colours = style->d_limb_colours, a.joint_colours = style->d_joint_colours;
  a.kpts = in->kpts;
  const size_t rows = (size_t)n * (size_t)in->max_det;
  a.boxes = (int4*)d_ws;
  a.points = d_points ? (int4*)d_points : (int4*)d_ws + rows;
  a.sn = in->stride_n, a.sk = in->stride_k, a.sp = in->stride_p, a.sc = in->stride_c;
  a.dt = in->dtype, a.kdim = in->kdim;
  a.n = n, a.D = in->max_det, a.K = in->k, a.P = in->p, a.L = in->n_limbs;
  a.n_limb_colours = style->n_limb_colours, a.n_joint_colours = style->n_joint_colours;
  a.thickness = style->thickness, a.diameter = style->diameter, a.alpha = style->alpha;
  a.thr = style->kpt_thr;
  if (a_isyuv(fmt))
    for (int k = 0; k < 3; ++k)
      for (int j = 0; j < 4; ++j)
        a.m[k][j] = params->rgb2yuv[k][j];

  hipStream_t s = as_stream(stream);
  VALI_ENTRY(s);
  const dim3 pgrid((unsigned)((rows + kWavesPerBlock - 1) / kWavesPerBlock));
  with_float_dtype(a.dt, [&](auto dt) { hipLaunchKernelGGL(k_pose_points<dt>, pgrid, dim3(kBlock), 0, s, a); });
  VALI_LAUNCH_CHECK();
  launch_paint(fmt, dim3(tiles, n), s, a);
  VALI_LAUNCH_CHECK();
  return VALI_OK;
}

int vali_pose_paint_points(const vali_surface* frames, const vali_surface* d_frames, int n, int format,
                           const int32_t* d_points, int p, int max_det, const int32_t* d_limbs, int n_limbs,
                           const vali_pose_style* style, const vali_cvt_params* params, void* d_ws, size_t ws_bytes,
                           vali_stream_t stream) {
  VALI_REQUIRE(frames && d_frames && d_points && style && d_ws, "null argument");
  VALI_REQUIRE(n >= 1 && n <= kMaxN, "n outside 1..1024");
  VALI_REQUIRE(p >= 1 && p <= kMaxP, "p outside 1..64");
  VALI_REQUIRE(max_det >= 1 && max_det <= kMaxD, "max_det outside 1..1024");
  VALI_REQUIRE((long long)n * max_det <= 65535, "n * max_det exceeds 65535");
  VALI_REQUIRE(n_limbs >= 0 && n_limbs <= kMaxL, "n_limbs outside 0..128");
  VALI_REQUIRE(d_limbs || n_limbs == 0, "limbs has a null pointer");
  VALI_REQUIRE(style->d_limb_colours && style->d_joint_colours, "limb_colours or joint_colours has a null pointer");
  VALI_REQUIRE(style->n_limb_colours >= 1 && style->n_joint_colours >= 1, "n_limb_colours or n_joint_colours below 1");
  VALI_REQUIRE(style->thickness >= 1 && style->thickness <= kMaxT, "thickness outside 1..64");
  VALI_REQUIRE(style->diameter >= 1 && style->diameter <= kMaxT, "diameter outside 1..64");
  VALI_REQUIRE(style->alpha >= -1 && style->alpha <= 255, "alpha outside -1..255");
  VALI_REQUIRE((((uintptr_t)style->d_limb_colours | (uintptr_t)style->d_joint_colours | (uintptr_t)d_limbs) & 3u) == 0,
               "limbs or colours are not 4-byte aligned");
  VALI_REQUIRE(((uintptr_t)d_points & 15u) == 0, "points is not 16-byte aligned");
  int tiles = 0;
  int rc = check_frames(__func__, n, frames, format, &tiles);
  if (rc != VALI_OK)
    return rc;
  const int fmt = tile_format(format);
  VALI_REQUIRE(params || !a_isyuv(fmt), "a YUV format needs params (rgb2yuv)");
  VALI_REQUIRE(((uintptr_t)d_ws & 15u) == 0, "the workspace is not 16-byte aligned");
  VALI_REQUIRE(ws_bytes >= vali_pose_workspace_size(n, max_det, p), "the workspace is smaller than vali_pose_workspace_size");

  const size_t rows = (size_t)n * (size_t)max_det;
  PoseArgs a = {};
  a.d_frames = d_frames, a.limbs = d_limbs;
  a.limb_colours = style->d_limb_colours, a.joint_colours = style->d_joint_colours;
  a.boxes = (int4*)d_ws;
  a.points = (int4*)d_ws + rows;
  a.n = n, a.D = max_det, a.P = p, a.L = n_limbs;
  a.n_limb_colours = style->n_limb_colours, a.n_joint_colours = style->n_joint_colours;
  a.thickness = style->thickness, a.diameter = style->diameter, a.alpha = style->alpha;
  if (a_isyuv(fmt))
    for (int k = 0; k < 3; ++k)
      for (int j = 0; j < 4; ++j)
        a.m[k][j] = params->rgb2yuv[k][j];
  BoxArgs b = {};
  b.d_frames = d_frames, b.src = (const int4*)d_points, b.points = a.points, b.boxes = a.boxes;
  b.n = n, b.D = max_det, b.P = p;
  b.thickness = style->thickness, b.diameter = style->diameter;

  hipStream_t s = as_stream(stream);
  VALI_ENTRY(s);
  hipLaunchKernelGGL(k_pose_boxes, dim3((unsigned)((rows + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock), 0, s, b);
  VALI_LAUNCH_CHECK();
  launch_paint(fmt, dim3(tiles, n), s, a);
  VALI_LAUNCH_CHECK();
  return VALI_OK;
}

} // extern "C"
