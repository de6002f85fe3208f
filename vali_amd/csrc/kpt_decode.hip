// Keypoint decode (vali_kpt_decode): the heatmaps (M, P, Hh, Wh) or SimCC vectors (M, P, Wx), (M, P, Wy) of a second-stage
// (top-down) pose or landmark network -> one point per map in FRAME pixels, through the matrices or roi records the crops
// were cut with, as the rows vali_pose_paint_points draws.  ONE launch, nothing allocated, nothing synchronises.
//
// Definition: include/vali_hip.h ("keypoint decode"); tests/kpt_decode_model.py restates it in numpy.
//
//   k_kpt_decode<DT, G>    a group of G lanes (a wave, or the workgroup of four) owns the map of one (slot, keypoint) and
//                          reads it ONCE.  A row is cut into the 16-byte pieces of the address grid: a piece that lies
//                          inside the row is one 16-byte load, the piece a row begins or ends in is read element by
//                          element, so a base or a pitch off the grid costs two narrow pieces a row and no byte outside a
//                          row is touched.  The pieces of all rows are dealt to the lanes in turn, six in flight per
//                          lane.  A lane carries (value, index) under e > best || (e == best && idx < best_idx) from
//                          (-inf, none): a NaN fails both comparisons, -0.0 equals 0.0, and a -inf beats "none" through
//                          its index.  The rule is a total order, so lanes combine by shuffles and waves through four
//                          pairs of LDS words in any order.  One lane then re-reads the peak's four neighbours and does
//                          steps 3 to 6.
//   k_kpt_decode_simcc<DT> a wave per (slot, keypoint): the same scan over the x vector, then over the y vector.
// Wave or workgroup per map: kWaveMapElems below.  A skipped slot's groups store zeros and leave without reading a map.
#include <math.h>

#include "common.hpp"
#include "dev_util.hpp"
#include "kpt_map.hpp"
#include "tensor_in.hpp"

#pragma clang fp contract(off)

namespace vali {
namespace {

constexpr int kMaxN = 1024, kMaxM = 65535, kMaxP = 64, kMaxSide = 4096, kMaxElems = 1 << 20, kMaxD = 1024;
constexpr int kMaxCanvas = 65535;
// A wave owns a map of up to this many elements; a larger one gets the workgroup.  At 8192 float16 elements a lane of
// the wave walks 16 pieces, three rounds of six loads in flight: beyond that the one wave's rounds, each a memory
// latency long, are the map's whole time, and four waves quarter it for one barrier.  Below it a workgroup per map
// would spend that barrier on maps of one round a lane (64 x 48 float16: 384 pieces, six a lane).
constexpr int kWaveMapElems = 8192;
constexpr int kNone = 0x7fffffff;
// pieces in flight per lane: eight took 70 VGPRs and the eighth wave of a SIMD (profiles/kpt_decode.md)
constexpr int kUnroll = 6;

struct DecArgs {
  const vali_surface* d_frames;
  const int32_t* rows;  // M rows of 8: matrices (D == 0) or roi records
  const void* heat;
  const void* vx;
  const void* vy;
  int4* points;
  float* kpts;  // or null
  long long sm, sp, sy;  // heat, in elements
  long long xm, xp, ym, yp;  // the vectors
  int n, M, P, Hh, Wh;  // SimCC: Wh = Wx, Hh = Wy
  int npx, npy;  // 16-byte pieces a row of Wh (of Hh, SimCC) elements can meet
  int D;  // rois: max_det; 0: matrices
  int cw, ch;
  int refine, align;
  float thr;
};

__device__ __forceinline__ void take(float e, int idx, float& best, int& bi) {
  if (e > best || (e == best && idx < bi))
    best = e, bi = idx;
}

// The peak of `rows` rows of W elements, `pitch` elements apart, over the G lanes of a group, this one being lane t: each
// lane's own best.  np pieces a row: one more than the row's bytes fill when a row may begin off the 16-byte grid.
template <int DT, int G>
__device__ __forceinline__ void scan(const typename TensorElem<DT>::Bits* base, int rows, int W, long long pitch, int np,
                                     int t, float& best, int& bi) {
  typedef TensorElem<DT> E;
  typedef typename E::Bits Bits;
  constexpr int ES = sizeof(Bits), EPV = 16 / ES, SH = ES == 4 ? 2 : 1;
  const int qg = G / np, rg = G - qg * np;  // the next piece of a lane is G pieces on
  int y = t / np, k = t - y * np;
  while (y < rows) {
    u32 w[kUnroll][4];
    int x0s[kUnroll], ys[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      ys[u] = y, x0s[u] = W;  // nothing of it is inside the row
      w[u][0] = w[u][1] = w[u][2] = w[u][3] = 0u;
      if (y < rows) {
        const Bits* r = base + (long long)y * pitch;
        const uint8_t* q = (const uint8_t*)((uintptr_t)r & ~(uintptr_t)15) + 16 * k;
        const int x0 = (int)(q - (const uint8_t*)r) >> SH;  // from -(EPV - 1)
        if (x0 < W) {
          x0s[u] = x0;
          if (x0 >= 0 && x0 + EPV <= W) {
            const v4u32 v = gload<v4u32>(q);
            w[u][0] = v.x, w[u][1] = v.y, w[u][2] = v.z, w[u][3] = v.w;
          } else {
#pragma unroll
            for (int e = 0; e < EPV; ++e) {
              const int x = x0 + e;
              if (x >= 0 && x < W)
                w[u][e * ES / 4] |= (u32)gload<Bits>(r + x) << (8 * (e * ES % 4));
            }
          }
        }
      }
      k += rg, y += qg;
      if (k >= np)
        k -= np, ++y;
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int at = ys[u] * W;
#pragma unroll
      for (int e = 0; e < EPV; ++e) {
        const int x = x0s[u] + e;
        if (x >= 0 && x < W)
          take(E::f(elem_bits<ES>(w[u], e)), at + x, best, bi);
      }
    }
  }
}

__device__ __forceinline__ void wave_peak(float& best, int& bi) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const float ov = __shfl_xor(best, d);
    const int oi = __shfl_xor(bi, d);
    take(ov, oi, best, bi);
  }
}

// step 1 for slot m: false for a skipped slot; the frame it belongs to
__device__ __forceinline__ bool slot_row(const DecArgs& a, int m, int (&r)[8], int& frame) {
  const uint4 lo = load16_u(a.rows + (size_t)m * 8), hi = load16_u(a.rows + (size_t)m * 8 + 4);
  r[0] = (int)lo.x, r[1] = (int)lo.y, r[2] = (int)lo.z, r[3] = (int)lo.w;
  r[4] = (int)hi.x, r[5] = (int)hi.y, r[6] = (int)hi.z, r[7] = (int)hi.w;
  if (a.D == 0) {
    frame = r[0];
    return frame >= 0 && frame < a.n;
  }
  frame = m / a.D;
  return r[2] >= 1 && r[3] >= 1 && r[6] >= 1 && r[7] >= 1;  // src_w, src_h, dst_w, dst_h
}

__device__ __forceinline__ void put_row(const DecArgs& a, int map, int4 pt, float fx, float fy, float conf) {
  a.points[map] = pt;
  if (a.kpts) {
    float* o = a.kpts + 3 * (size_t)map;
    o[0] = fx, o[1] = fy, o[2] = conf;
  }
}

// steps 4 to 6 for the peak (xp + ox, yp + oy) of a map of wn x hn cells
__device__ __forceinline__ void finish(const DecArgs& a, int map, const int (&r)[8], int frame, int xp, int yp, float ox,
                                       float oy, int wn, int hn, float conf) {
  const float sx = __fdiv_rn((float)a.cw, (float)wn), sy = __fdiv_rn((float)a.ch, (float)hn);
  float cu, cv;
  if (a.align == VALI_KPT_ALIGN_CENTRE) {
    cu = __fmul_rn(__fadd_rn(__fadd_rn((float)xp, 0.5f), ox), sx);
    cv = __fmul_rn(__fadd_rn(__fadd_rn((float)yp, 0.5f), oy), sy);
  } else {
    cu = __fadd_rn(__fmul_rn(__fadd_rn((float)xp, ox), sx), 0.5f);
    cv = __fadd_rn(__fmul_rn(__fadd_rn((float)yp, oy), sy), 0.5f);
  }
  float fx, fy;
  if (a.D == 0) {
    const float ma = __int_as_float(r[1]), mb = __int_as_float(r[2]), mc = __int_as_float(r[3]);
    const float md = __int_as_float(r[4]), me = __int_as_float(r[5]), mf = __int_as_float(r[6]);
    fx = __fadd_rn(__fadd_rn(__fmul_rn(ma, cu), __fmul_rn(mb, cv)), mc);
    fy = __fadd_rn(__fadd_rn(__fmul_rn(md, cu), __fmul_rn(me, cv)), mf);
  } else {  // src_x, src_y, src_w, src_h, dst_x, dst_y, dst_w, dst_h
    fx = map_axis(cu, r[4], r[2], r[6], r[0]);
    fy = map_axis(cv, r[5], r[3], r[7], r[1]);
  }
  int X = 0, Y = 0, flag = 0;
  if (kpt_visible(conf, a.thr, cu, cv, fx, fy)) {
    const int W = a.d_frames[frame].width, H = a.d_frames[frame].height;
    X = (int)floorf(fx), Y = (int)floorf(fy);
    flag = (X >= 0 && X < W && Y >= 0 && Y < H) ? 3 : 1;
  }
  put_row(a, map, make_int4(X, Y, __float_as_int(conf), flag), fx, fy, conf);
}

__device__ __forceinline__ void no_peak(const DecArgs& a, int map) {
  const float nan = __int_as_float(0x7fc00000);
  put_row(a, map, make_int4(0, 0, 0x7fc00000, 0), 0.0f, 0.0f, nan);
}

template <int DT, int G>
__global__ void __launch_bounds__(kBlock) k_kpt_decode(const DecArgs a) {
  typedef TensorElem<DT> E;
  typedef typename E::Bits Bits;
  static_assert(G == kWave || G == kBlock, "a wave or the workgroup");
  const int map = G == kWave ? (int)blockIdx.x * kWavesPerBlock + (int)threadIdx.x / kWave : (int)blockIdx.x;
  const int t = G == kWave ? (int)(threadIdx.x & (kWave - 1)) : (int)threadIdx.x;
  if (map >= a.M * a.P)
    return;  // (a whole wave: only G == kWave has a partial last workgroup)
  const int m = map / a.P, j = map - m * a.P;
  int r[8], frame;
  if (!slot_row(a, m, r, frame)) {  // the same in every lane of the group
    if (t == 0)
      put_row(a, map, make_int4(0, 0, 0, 0), 0.0f, 0.0f, 0.0f);
    return;
  }
  const Bits* base = (const Bits*)a.heat + (long long)m * a.sm + (long long)j * a.sp;
  float best = -INFINITY;
  int bi = kNone;
  scan<DT, G>(base, a.Hh, a.Wh, a.sy, a.npx, t, best, bi);
  wave_peak(best, bi);
  if constexpr (G == kBlock) {
    __shared__ float lv[kWavesPerBlock];
    __shared__ int li[kWavesPerBlock];
    if ((t & (kWave - 1)) == 0)
      lv[t / kWave] = best, li[t / kWave] = bi;
    __syncthreads();
    if (t == 0) {
#pragma unroll
      for (int w = 1; w < kWavesPerBlock; ++w)
        take(lv[w], li[w], best, bi);
    }
  }
  if (t != 0)
    return;
  if (bi == kNone) {
    no_peak(a, map);
    return;
  }
  const int yp = bi / a.Wh, xp = bi - yp * a.Wh;
  float ox = 0.0f, oy = 0.0f;
  if (a.refine == VALI_KPT_REFINE_QUARTER) {
    const Bits* row = base + (long long)yp * a.sy;
    if (xp > 0 && xp < a.Wh - 1) {
      const float d = __fsub_rn(E::f((u32)gload<Bits>(row + xp + 1)), E::f((u32)gload<Bits>(row + xp - 1)));
      ox = d > 0.0f ? 0.25f : d < 0.0f ? -0.25f : 0.0f;
    }
    if (yp > 0 && yp < a.Hh - 1) {
      const float d = __fsub_rn(E::f((u32)gload<Bits>(row + a.sy + xp)), E::f((u32)gload<Bits>(row - a.sy + xp)));
      oy = d > 0.0f ? 0.25f : d < 0.0f ? -0.25f : 0.0f;
    }
  }
  finish(a, map, r, frame, xp, yp, ox, oy, a.Wh, a.Hh, best);
}

template <int DT>
__global__ void __launch_bounds__(kBlock) k_kpt_decode_simcc(const DecArgs a) {
  typedef typename TensorElem<DT>::Bits Bits;
  const int map = (int)blockIdx.x * kWavesPerBlock + (int)threadIdx.x / kWave;
  const int t = (int)(threadIdx.x & (kWave - 1));
  if (map >= a.M * a.P)
    return;
  const int m = map / a.P, j = map - m * a.P;
  int r[8], frame;
  if (!slot_row(a, m, r, frame)) {
    if (t == 0)
      put_row(a, map, make_int4(0, 0, 0, 0), 0.0f, 0.0f, 0.0f);
    return;
  }
  float bx = -INFINITY, by = -INFINITY;
  int ix = kNone, iy = kNone;
  scan<DT, kWave>((const Bits*)a.vx + (long long)m * a.xm + (long long)j * a.xp, 1, a.Wh, 0, a.npx, t, bx, ix);
  scan<DT, kWave>((const Bits*)a.vy + (long long)m * a.ym + (long long)j * a.yp, 1, a.Hh, 0, a.npy, t, by, iy);
  wave_peak(bx, ix);
  wave_peak(by, iy);
  if (t != 0)
    return;
  if (ix == kNone || iy == kNone) {
    no_peak(a, map);
    return;
  }
  finish(a, map, r, frame, ix, iy, 0.0f, 0.0f, a.Wh, a.Hh, by < bx ? by : bx);
}

// the pieces a row of w elements of es bytes can meet: one more when a row may begin off the 16-byte grid
int pieces(int w, int es, bool on_grid) { return (w * es + 15) / 16 + (on_grid ? 0 : 1); }

template <int DT>
void launch_dt(const DecArgs& a, bool simcc, hipStream_t s) {
  const unsigned maps = (unsigned)a.M * (unsigned)a.P;
  const unsigned waves = (maps + kWavesPerBlock - 1) / kWavesPerBlock;
  if (simcc)
    hipLaunchKernelGGL(k_kpt_decode_simcc<DT>, dim3(waves), dim3(kBlock), 0, s, a);
  else if (a.Hh * a.Wh <= kWaveMapElems)
    hipLaunchKernelGGL((k_kpt_decode<DT, kWave>), dim3(waves), dim3(kBlock), 0, s, a);
  else
    hipLaunchKernelGGL((k_kpt_decode<DT, kBlock>), dim3(maps), dim3(kBlock), 0, s, a);
}

} // namespace
} // namespace vali

using namespace vali;

extern "C" {

int vali_kpt_decode(const vali_surface* d_frames, int n, const vali_kpt_decode_in* in, const int32_t* d_matrices,
                    const vali_roi* d_rois, int32_t* d_points, float* d_kpts, vali_stream_t stream) {
  VALI_REQUIRE(d_frames && in && d_points, "null argument");
  VALI_REQUIRE((d_matrices != nullptr) != (d_rois != nullptr), "exactly one of matrices and rois");
  VALI_REQUIRE(n >= 1 && n <= kMaxN, "n outside 1..1024");
  const bool simcc = in->heat == nullptr;
  VALI_REQUIRE(!simcc || (in->simcc_x && in->simcc_y), "neither heat nor both of simcc_x and simcc_y");
  VALI_REQUIRE(simcc || (!in->simcc_x && !in->simcc_y), "heat and SimCC vectors at once");
  // one dtype for the heatmaps or the two SimCC vectors: tensor_in.hpp's predicates under this entry point's own words
  if (!float_dtype(in->dtype))
    return fail(VALI_ERR_INVALID_ARG, "%s: dtype %d is not float32, float16 or bfloat16", __func__, in->dtype);
  VALI_REQUIRE(in->m >= 1 && in->m <= kMaxM, "m outside 1..65535");
  VALI_REQUIRE(in->p >= 1 && in->p <= kMaxP, "p outside 1..64");
  VALI_REQUIRE(in->hh >= 1 && in->hh <= kMaxSide && in->wh >= 1 && in->wh <= kMaxSide, "hh or wh outside 1..4096");
  VALI_REQUIRE(simcc || (long long)in->hh * in->wh <= kMaxElems, "hh * wh exceeds 2^20");
  VALI_REQUIRE(in->canvas_w >= 1 && in->canvas_w <= kMaxCanvas && in->canvas_h >= 1 && in->canvas_h <= kMaxCanvas,
               "canvas size outside 1..65535");
  VALI_REQUIRE(in->refine == VALI_KPT_REFINE_NONE || in->refine == VALI_KPT_REFINE_QUARTER, "unknown refine");
  VALI_REQUIRE(!simcc || in->refine == VALI_KPT_REFINE_NONE, "SimCC vectors take no refinement");
  VALI_REQUIRE(in->align == VALI_KPT_ALIGN_CENTRE || in->align == VALI_KPT_ALIGN_INDEX, "unknown align");
  VALI_REQUIRE(in->kpt_thr == in->kpt_thr, "kpt_thr is a NaN");
  if (d_rois) {
    VALI_REQUIRE(in->max_det >= 1 && in->max_det <= kMaxD, "max_det outside 1..1024");
    VALI_REQUIRE((long long)n * in->max_det == in->m, "m is not n * max_det");
  }
  const int es = float_dtype_size(in->dtype);
  const uintptr_t emask = (uintptr_t)(es - 1);
  const int64_t hs[3] = {in->stride_m, in->stride_p, in->stride_y};
  const int64_t vs[4] = {in->x_stride_m, in->x_stride_p, in->y_stride_m, in->y_stride_p};
  if (simcc) {
    VALI_REQUIRE((((uintptr_t)in->simcc_x | (uintptr_t)in->simcc_y) & emask) == 0,
                 "simcc_x or simcc_y is not aligned to its element size");
    VALI_REQUIRE(strides_ok(vs, 4), "a SimCC stride outside 0..2^40");
  } else {
    VALI_REQUIRE(((uintptr_t)in->heat & emask) == 0, "heat is not aligned to its element size");
    VALI_REQUIRE(strides_ok(hs, 3), "a heat stride outside 0..2^40");
  }
  VALI_REQUIRE((((uintptr_t)d_frames | (uintptr_t)d_matrices | (uintptr_t)d_rois | (uintptr_t)d_kpts) & 3u) == 0,
               "frames, matrices, rois or kpts are not 4-byte aligned");
  VALI_REQUIRE(((uintptr_t)d_points & 15u) == 0, "points is not 16-byte aligned");

  DecArgs a = {};
  a.d_frames = d_frames;
  a.rows = d_matrices ? d_matrices : (const int32_t*)d_rois;
  a.heat = in->heat, a.vx = in->simcc_x, a.vy = in->simcc_y;
  a.points = (int4*)d_points, a.kpts = d_kpts;
  a.n = n, a.M = in->m, a.P = in->p, a.Hh = in->hh, a.Wh = in->wh;
  a.D = d_rois ? in->max_det : 0;
  a.cw = in->canvas_w, a.ch = in->canvas_h;
  a.refine = in->refine, a.align = in->align;
  a.thr = in->kpt_thr;
  if (simcc) {
    a.xm = vs[0], a.xp = vs[1], a.ym = vs[2], a.yp = vs[3];
    a.npx = pieces(a.Wh, es, (((uintptr_t)a.vx | (uintptr_t)((vs[0] | vs[1]) * es)) & 15u) == 0);
    a.npy = pieces(a.Hh, es, (((uintptr_t)a.vy | (uintptr_t)((vs[2] | vs[3]) * es)) & 15u) == 0);
  } else {
    a.sm = hs[0], a.sp = hs[1], a.sy = hs[2];
    a.npx = pieces(a.Wh, es, (((uintptr_t)a.heat | (uintptr_t)((hs[0] | hs[1] | hs[2]) * es)) & 15u) == 0);
  }

  hipStream_t s = as_stream(stream);
  VALI_ENTRY(s);
  with_float_dtype(in->dtype, [&](auto dt) { launch_dt<dt>(a, simcc, s); });
  VALI_LAUNCH_CHECK();
  return VALI_OK;
}

} // extern "C"
