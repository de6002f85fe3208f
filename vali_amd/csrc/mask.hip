// Instance masks (vali_mask_paint): the masks of a segmentation head's detections -- coefficients x prototypes, upsampled
// bilinearly to the frame, thresholded at 0 -- blended IN PLACE onto a batch of NV12, YUV420, YUV444, RGB, BGR or
// RGB_PLANAR frames, from detections that live in DEVICE memory (vali_detect_select's dets).
//
// Definition: include/vali_hip.h ("instance masks"); tests/mask_model.py restates it in numpy.
//
// Two launches, whatever the data:
//   k_mask_logits   grid (prototype tiles of 64 x 16, n * max_det rows).  A skipped row leaves after reading its dets row;
//                   the others read their M coefficients once into LDS and store, as float32 into the row's hp x wp slot
//                   of the workspace, the logits of the prototype range launch 2 can sample for the row's clipped box.
//                   The range comes from the sample position of the box's first and last pixel: the position is
//                   monotone in the pixel, and the clamps are the sampler's own.  Lanes run along x.
//   k_mask_paint<FMT>
//                   k_annotate's structure: a workgroup owns one 64 x 64 luma tile of one frame, culls its frame's
//                   max_det rows against the tile into an LDS hit list (in row order) and, with no hit, leaves without
//                   touching a pixel.  The sampler's per-column (ix0, ix1, tx) and per-row (iy0, iy1, ty) depend on the
//                   frame's record only: 64 + 64 of them go to LDS once per tile.  A lane keeps its 16-byte pieces in
//                   registers, applies all hits in order -- the logits come through the L2 -- and stores a piece only if a
//                   mask changed it.  The blend is STAMP's (cover_piece) with the coverage made on the fly.
// The formats and the frame rules, the tile's pieces, the hit list and the coverage blend are tile_paint.hpp's, shared
// with annotate.hip, the rows det_rows.hpp's, shared with pose.hip, the sampler (step 3) head_sampler.hpp's, shared with
// semantic.hip; here is the coverage of a hit.
#include <math.h>

#include "det_rows.hpp"
#include "head_sampler.hpp"
#include "tensor_in.hpp"

#pragma clang fp contract(off)

namespace vali {
namespace {

constexpr int kLogW = 64, kLogH = 16;  // prototype pixels a tile (launch 1)
constexpr int kMaxN = 1024, kMaxM = 64, kMaxP = 1024, kMaxK = 1 << 20, kMaxD = 1024;

struct MaskArgs {
  const vali_surface* d_frames;
  const int32_t* dets;
  const vali_roi* rects;
  const int32_t* colours;
  const void* protos;
  const void* coeffs;
  float* ws;
  long long pn, pm, py;  // element strides of protos
  long long cn, ck, cm;  // ... and of coeffs
  int pdt, cdt;
  int n, D, M, Hp, Wp, K, net_w, net_h;
  int n_colours, alpha;
  float m[3][4];  // rgb2yuv rows (YUV formats)
};

// ---- launch 1: the logits a row's box can sample ------------------------------------------------------------------------
template <int DT>
__global__ void __launch_bounds__(kBlock) k_mask_logits(const MaskArgs a) {
  typedef typename std::conditional<DT == VALI_DTYPE_F32, u32, uint16_t>::type Bits;  // an element's bits
  __shared__ float cf[kMaxM];
  const int row = blockIdx.y, f = row / a.D;
  int r[8];
  load_row(a.dets, row, r);
  const int W = a.d_frames[f].width, H = a.d_frames[f].height;
  const vali_roi rc = a.rects[f];
  Row o;
  if (!resolve_row(r, f, W, H, a.K, rc, o))
    return;
  const Axis ax = make_axis(rc.src_x, rc.src_w, rc.dst_x, rc.dst_w, a.Wp, a.net_w);
  const Axis ay = make_axis(rc.src_y, rc.src_h, rc.dst_y, rc.dst_h, a.Hp, a.net_h);
  // all of 0 .. Wp - 1 resp. 0 .. Hp - 1, and c0 <= c1, r0 <= r1: the position is monotone in the pixel
  const int c0 = axis_tap(ax, o.x0).i0, c1 = axis_tap(ax, o.x1 - 1).i1;
  const int r0 = axis_tap(ay, o.y0).i0, r1 = axis_tap(ay, o.y1 - 1).i1;
  const int tiles_x = (a.Wp + kLogW - 1) / kLogW;
  const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
  const int X0 = tx * kLogW, Y0 = ty * kLogH;
  if (X0 > c1 || X0 + kLogW <= c0 || Y0 > r1 || Y0 + kLogH <= r0)
    return;
  const int tid = threadIdx.x;
  if (tid < a.M)
    cf[tid] = tensor_elem_f(a.coeffs, a.cdt, (long long)f * a.cn + (long long)o.k * a.ck + (long long)tid * a.cm);
  __syncthreads();
  const int xp = X0 + (tid & (kWave - 1));
  if (xp < c0 || xp > c1)
    return;
  const Bits* base = (const Bits*)a.protos + (long long)f * a.pn + xp;
  float* out = a.ws + (size_t)row * (size_t)a.Hp * (size_t)a.Wp + xp;
  for (int j = tid / kWave; j < kLogH; j += kWavesPerBlock) {
    const int yp = Y0 + j;
    if (yp < r0 || yp > r1)
      continue;
    const Bits* p = base + (long long)yp * a.py;
    float acc = 0.0f;
    for (int m = 0; m < a.M; ++m) {
      const u32 b = (u32)p[(long long)m * a.pm];
      const float v = DT == VALI_DTYPE_F32   ? __uint_as_float(b)
                      : DT == VALI_DTYPE_F16 ? (float)__builtin_bit_cast(_Float16, (uint16_t)b)
                                             : __uint_as_float(b << 16);
      acc = __fadd_rn(acc, __fmul_rn(cf[m], v));
    }
    out[(size_t)yp * (size_t)a.Wp] = acc;
  }
}

// ---- launch 2: the tiles ------------------------------------------------------------------------------------------------
// one hit, as the pieces see it: the logits of its slot, its clipped box, and the tile's sampler taps in LDS
struct Hit {
  const float* L;
  int Wp;
  int rx0, ry0, rx1, ry1;
  int tx0, ty0;
  const int4* colp;  // i0, i1, the bits of t, 0 of luma column tx0 + j
  const int4* rowp;  // ... of luma row ty0 + j
};

// The coverage (255 in the mask, 0 outside) of the N (16, or 6 for a packed RGB piece) frame pixels X .. X + N - 1 of frame
// row py, a byte each: steps 4 and 5 of the definition.  Only pixels inside the clipped box are sampled, so every logit
// read is one launch 1 wrote; the taps index inside the row's slot whatever the pixel.
template <int N>
__device__ __forceinline__ void mask_cov(const Hit& h, int X, int py, u32 (&cv)[N == 16 ? 4 : 2]) {
  constexpr int NW = N == 16 ? 4 : 2;
#pragma unroll
  for (int k = 0; k < NW; ++k)
    cv[k] = 0u;
  const int lo = max(h.rx0 - X, 0), hi = min(h.rx1 - X, N);
  if (py < h.ry0 || py >= h.ry1 || lo >= hi)
    return;
  const int4 rp = h.rowp[(py - h.ty0) & (kTile - 1)];
  const float* r0 = h.L + (size_t)rp.x * (size_t)h.Wp;
  const float* r1 = h.L + (size_t)rp.y * (size_t)h.Wp;
  const float ty = __int_as_float(rp.z);
#pragma unroll
  for (int k = 0; k < N; ++k) {
    if (k >= lo && k < hi) {
      const int4 cp = h.colp[(X - h.tx0 + k) & (kTile - 1)];
      const float tx = __int_as_float(cp.z);
      const float a = r0[cp.x], b = r0[cp.y], c = r1[cp.x], d = r1[cp.y];
      const float top = __fadd_rn(a, __fmul_rn(tx, __fsub_rn(b, a)));
      const float bot = __fadd_rn(c, __fmul_rn(tx, __fsub_rn(d, c)));
      const float v = __fadd_rn(top, __fmul_rn(ty, __fsub_rn(bot, top)));
      if (v > 0.0f)  // a NaN is never in
        cv[k / 4] |= 0xffu << (8 * (k % 4));
    }
  }
}

// a hit as cover_piece's coverage source (tile_paint.hpp)
struct HitCov : Hit {
  template <int N>
  __device__ __forceinline__ void get(int X, int py, u32 (&cv)[N == 16 ? 4 : 2]) const {
    mask_cov<N>(*this, X, py, cv);
  }
};

template <int FMT>
__global__ void __launch_bounds__(kBlock) k_mask_paint(const MaskArgs a) {
  __shared__ uint16_t hits[kMaxD];
  __shared__ int wtot[kWavesPerBlock];
  __shared__ int4 colp[kTile], rowp[kTile];
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
  const vali_roi rc = a.rects[f];

  // the frame's rows whose box meets this tile, in row order
  int nh = 0;
  for (int base = 0; base < a.D; base += kBlock) {
    const int i = base + tid;
    bool flag = false;
    if (i < a.D) {
      int r[8];
      load_row(a.dets, f * a.D + i, r);
      Row o;
      flag = resolve_row(r, f, W, H, a.K, rc, o) && o.x0 < tx1 && o.x1 > tx0 && o.y0 < ty1 && o.y1 > ty0;
    }
    nh = compact_put(flag, i, hits, nh, wtot);
  }
  if (nh == 0)
    return;

  // the sampler's taps of the tile's 64 columns and 64 rows: they depend on the frame's record only
  if (tid < kTile) {
    const Tap t = axis_tap(make_axis(rc.src_x, rc.src_w, rc.dst_x, rc.dst_w, a.Wp, a.net_w), tx0 + tid);
    colp[tid] = make_int4(t.i0, t.i1, __float_as_int(t.t), 0);
  } else if (tid < 2 * kTile) {
    const Tap t = axis_tap(make_axis(rc.src_y, rc.src_h, rc.dst_y, rc.dst_h, a.Hp, a.net_h), ty0 + tid - kTile);
    rowp[tid - kTile] = make_int4(t.i0, t.i1, __float_as_int(t.t), 0);
  }
  __syncthreads();

  // the lane's pieces
  Piece pc[NS];
  u32 cur[NS][4], orig[NS][4];
#define VALI_SLOT(S) load_piece<FMT, S>(d, tid, tx0, ty0, W, H, pc[S], cur[S], orig[S]);
  VALI_SLOTS(VALI_SLOT)
#undef VALI_SLOT

  for (int hi = 0; hi < nh; ++hi) {
    const int idx = __builtin_amdgcn_readfirstlane((int)hits[hi]);
    const int row = f * a.D + idx;
    int r[8];
    load_row(a.dets, row, r);
    // (the cull let the row through: only its clipped box is formed again)
    Row o;
    clip_box(r, W, H, o);
    int ci = o.cls % a.n_colours;
    ci += ci < 0 ? a.n_colours : 0;
    const u32 colour = (u32)a.colours[ci];
    const u32 alpha = a.alpha >= 0 ? (u32)a.alpha : colour >> 24;
    // (spelled out as in k_annotate: see there)
    const u32 cr = (colour >> 16) & 0xffu, cg = (colour >> 8) & 0xffu, cb = colour & 0xffu;
    u32 col[3];
    if constexpr (a_isyuv(FMT)) {
      const float fr = (float)cr, fg = (float)cg, fb = (float)cb;
#pragma unroll
      for (int k = 0; k < 3; ++k)
        col[k] = quantize_u8(dot_rgb(a.m[k], fr, fg, fb));
    } else if constexpr (FMT == A_BGR) {
      col[0] = cb, col[1] = cg, col[2] = cr;
    } else {
      col[0] = cr, col[1] = cg, col[2] = cb;
    }
    HitCov h;
    h.L = a.ws + (size_t)row * (size_t)a.Hp * (size_t)a.Wp;
    h.Wp = a.Wp;
    h.rx0 = o.x0, h.ry0 = o.y0, h.rx1 = o.x1, h.ry1 = o.y1;
    h.tx0 = tx0, h.ty0 = ty0;
    h.colp = colp, h.rowp = rowp;
#define VALI_SLOT(S) cover_piece<FMT, S>(h, pc[S], col, alpha, cur[S]);
    VALI_SLOTS(VALI_SLOT)
#undef VALI_SLOT
  }

  // only what a mask changed goes back
#define VALI_SLOT(S) store_piece(pc[S], cur[S], orig[S]);
  VALI_SLOTS(VALI_SLOT)
#undef VALI_SLOT
}
#undef VALI_SLOTS

bool dims_ok(int n, int D, int hp, int wp) {
  return n >= 1 && n <= kMaxN && D >= 1 && D <= kMaxD && (long long)n * D <= 65535 && hp >= 1 && hp <= kMaxP && wp >= 1 &&
         wp <= kMaxP;
}

} // namespace
} // namespace vali

using namespace vali;

extern "C" {

size_t vali_mask_workspace_size(int n, int max_det, int hp, int wp) {
  if (!dims_ok(n, max_det, hp, wp))
    return 0;
  return (size_t)n * (size_t)max_det * (size_t)hp * (size_t)wp * 4u;
}

int vali_mask_paint(const vali_surface* frames, const vali_surface* d_frames, int n, int format, const vali_mask_in* in,
                    const int32_t* d_dets, const vali_roi* d_rects, const int32_t* d_colours, int n_colours, int alpha,
                    const vali_cvt_params* params, void* d_ws, size_t ws_bytes, vali_stream_t stream) {
  VALI_REQUIRE(frames && d_frames && in && d_dets && d_rects && d_colours && d_ws, "null argument");
  VALI_REQUIRE(n >= 1 && n <= kMaxN, "n outside 1..1024");
  VALI_REQUIRE(in->m >= 1 && in->m <= kMaxM, "m outside 1..64");
  VALI_REQUIRE(in->hp >= 1 && in->hp <= kMaxP && in->wp >= 1 && in->wp <= kMaxP, "hp or wp outside 1..1024");
  VALI_REQUIRE(in->k >= 1 && in->k <= kMaxK, "k outside 1..2^20");
  VALI_REQUIRE(in->max_det >= 1 && in->max_det <= kMaxD, "max_det outside 1..1024");
  VALI_REQUIRE((long long)n * in->max_det <= 65535, "n * max_det exceeds 65535");
  VALI_REQUIRE(in->net_w >= 1 && in->net_w <= 65535 && in->net_h >= 1 && in->net_h <= 65535,
               "net_w or net_h outside 1..65535");
  const int64_t ps[3] = {in->protos.stride_n, in->protos.stride_m, in->protos.stride_y};
  const int64_t cs[3] = {in->coeffs.stride_n, in->coeffs.stride_k, in->coeffs.stride_c};
  int rc = check_head_tensor(__func__, "protos", in->protos.data, in->protos.dtype, ps, 3);
  if (rc != VALI_OK)
    return rc;
  rc = check_head_tensor(__func__, "coeffs", in->coeffs.data, in->coeffs.dtype, cs, 3);
  if (rc != VALI_OK)
    return rc;
  VALI_REQUIRE(n_colours >= 1, "n_colours below 1");
  VALI_REQUIRE(alpha >= -1 && alpha <= 255, "alpha outside -1..255");
  VALI_REQUIRE((((uintptr_t)d_dets | (uintptr_t)d_rects | (uintptr_t)d_colours) & 3u) == 0,
               "dets, rects or colours are not 4-byte aligned");
  int tiles = 0;
  rc = check_frames(__func__, n, frames, format, &tiles);
  if (rc != VALI_OK)
    return rc;
  const int fmt = tile_format(format);
  VALI_REQUIRE(params || !a_isyuv(fmt), "a YUV format needs params (rgb2yuv)");
  VALI_REQUIRE(((uintptr_t)d_ws & 15u) == 0, "the workspace is not 16-byte aligned");
  VALI_REQUIRE(ws_bytes >= vali_mask_workspace_size(n, in->max_det, in->hp, in->wp),
               "the workspace is smaller than vali_mask_workspace_size");

  MaskArgs a = {};
  a.d_frames = d_frames, a.dets = d_dets, a.rects = d_rects, a.colours = d_colours;
  a.protos = in->protos.data, a.coeffs = in->coeffs.data, a.ws = (float*)d_ws;
  a.pn = in->protos.stride_n, a.pm = in->protos.stride_m, a.py = in->protos.stride_y;
  a.cn = in->coeffs.stride_n, a.ck = in->coeffs.stride_k, a.cm = in->coeffs.stride_c;
  a.pdt = in->protos.dtype, a.cdt = in->coeffs.dtype;
  a.n = n, a.D = in->max_det, a.M = in->m, a.Hp = in->hp, a.Wp = in->wp, a.K = in->k;
  a.net_w = in->net_w, a.net_h = in->net_h;
  a.n_colours = n_colours, a.alpha = alpha;
  if (a_isyuv(fmt))
    for (int k = 0; k < 3; ++k)
      for (int j = 0; j < 4; ++j)
        a.m[k][j] = params->rgb2yuv[k][j];

  hipStream_t s = as_stream(stream);
  VALI_ENTRY(s);
  const dim3 lgrid(((a.Wp + kLogW - 1) / kLogW) * ((a.Hp + kLogH - 1) / kLogH), n * a.D);
  with_float_dtype(a.pdt, [&](auto dt) { hipLaunchKernelGGL(k_mask_logits<dt>, lgrid, dim3(kBlock), 0, s, a); });
  VALI_LAUNCH_CHECK();
  const dim3 grid(tiles, n);
  with_tile_format(fmt, [&](auto f) { hipLaunchKernelGGL(k_mask_paint<f>, grid, dim3(kBlock), 0, s, a); });
  VALI_LAUNCH_CHECK();
  return VALI_OK;
}

} // extern "C"
