// Semantic segmentation maps (vali_semantic_paint): the (n, c, hs, ws) class logits of a segmentation head, upsampled
// bilinearly to the frame and arg-maxed per pixel, written as a class map per frame and / or tinted IN PLACE onto a
// batch of NV12, YUV420, YUV444, RGB, BGR or RGB_PLANAR frames.
//
// Definition: include/vali_hip.h ("semantic maps"); tests/semantic_model.py restates it in numpy.
//
// One launch, whatever the data: k_semantic_paint<FMT, DT>, grid (tiles of the largest frame, n).  A workgroup owns one
// 64 x 64 luma tile of one frame.  A tile no region pixel meets writes its 255s (with labels) and leaves before it reads a
// frame byte.  Otherwise
//   taps      the sampler's (i0, i1, t) of the tile's 64 columns and 64 rows go to LDS once: they depend on the frame's
//             record only.  Pixels outside the region take the taps of the nearest region pixel, so that a footprint in
//             the logits, first column's i0 .. last column's i1 by first row's i0 .. last row's i1, is the region's.
//   classify  in two passes of 32 tile rows: a lane owns 8 consecutive luma pixels of one row a pass and carries best[8]
//             and label[8] over the classes (16 pixels a lane do not fit the registers of four waves a SIMD).
//             STAGED (the pass's footprint of one class fits kStage floats: frames that are upsampled, the normal
//             case): the footprint of as many classes as fit is converted once into LDS as float32, at an odd row pitch,
//             and the four taps of a pixel are DS reads.  DIRECT (logits finer than about 1.4 cells a frame pixel): the
//             taps are global loads.  Same arithmetic, same results; the choice is per pass, from the taps.
//   labels    the tile's 4096 labels (255 outside the region) go to LDS, and from there to the label surface as 16-byte
//             pieces clipped at the right edge; the classes present are collected in a 256-bit set on the way.
//   paint     tile_paint.hpp's pieces: every present class in ascending order is one cover_piece whose coverage source
//             answers label == c ? 255 : 0 from the LDS tile -- the STAMP blend of the definition by construction.
#include <math.h>

#include "head_sampler.hpp"
#include "tensor_in.hpp"
#include "tile_paint.hpp"

#pragma clang fp contract(off)

namespace vali {
namespace {

constexpr int kMaxN = 1024, kMaxC = 255, kMaxS = 4096;
constexpr int kStage = 8192;  // float32 cells of staged logits a workgroup (32 KiB)

struct SemArgs {
  const vali_surface* d_frames;
  const vali_surface* d_labels;  // or null
  const vali_roi* rects;
  const int32_t* colours;  // or null: labels only
  const void* logits;
  long long sn, sc, sy;  // element strides
  int n, C, Hs, Ws, net_w, net_h;
  int n_colours, alpha;
  float m[3][4];  // rgb2yuv rows (YUV formats)
};

// The two logits rows a lane's pixels sample, in LDS (staged) ...  fresh(): the row bases of a class are made opaque to
// the compiler, which otherwise keeps one address per tap and row (64 of them) alive across the class loop, advances each
// by the class stride, and runs out of registers; with it an address is one add before its load.
struct LdsRows {
  const float* stage;
  int o0, o1;
  __device__ __forceinline__ void fresh() { asm volatile("" : "+v"(o0), "+v"(o1)); }
  __device__ __forceinline__ float top(u32 i) const { return stage[o0 + i]; }
  __device__ __forceinline__ float bot(u32 i) const { return stage[o1 + i]; }
};
// ... and in the tensor (direct)
template <int DT>
struct TensorRows {
  typedef TensorElem<DT> E;
  const typename E::Bits* r0;
  const typename E::Bits* r1;
  __device__ __forceinline__ void fresh() { asm volatile("" : "+v"(r0), "+v"(r1)); }
  __device__ __forceinline__ float top(u32 i) const { return E::f(gload<typename E::Bits>(r0 + i)); }
  __device__ __forceinline__ float bot(u32 i) const { return E::f(gload<typename E::Bits>(r1 + i)); }
};

// steps 3 and 4 of the definition for one class on the lane's kPx pixels: xo[k] holds the two column taps of pixel k as
// offsets into the rows (i0 | i1 << 16)
constexpr int kPx = 8;                    // luma pixels a lane classifies in one pass
constexpr int kPassRows = kBlock / (kTile / kPx);  // tile rows a pass: 32
template <class Rows>
__device__ __forceinline__ void classify(Rows rw, const u32 (&xo)[kPx], const float (&tx)[kPx], float ty, int label,
                                         float (&best)[kPx], int (&lbl)[kPx]) {
  rw.fresh();
#pragma unroll
  for (int k = 0; k < kPx; ++k) {
    const u32 i0 = xo[k] & 0xffffu, i1 = xo[k] >> 16;
    const float a = rw.top(i0), b = rw.top(i1), c = rw.bot(i0), d = rw.bot(i1);
    const float top = __fadd_rn(a, __fmul_rn(tx[k], __fsub_rn(b, a)));
    const float bot = __fadd_rn(c, __fmul_rn(tx[k], __fsub_rn(d, c)));
    const float v = __fadd_rn(top, __fmul_rn(ty, __fsub_rn(bot, top)));
    const bool win = v > best[k];  // a NaN never wins
    best[k] = win ? v : best[k];
    lbl[k] = win ? label : lbl[k];
  }
}

// 0xff in every byte of w that equals the byte replicated in c4
__device__ __forceinline__ u32 eq_bytes(u32 w, u32 c4) {
  const u32 x = w ^ c4;
  const u32 z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
  return (z >> 7) * 0xffu;
}

// one class of the tile's labels as cover_piece's coverage source (tile_paint.hpp): 255 where the label is the class
struct LabelCov {
  const uint8_t* lab;  // the tile's 64 x 64 labels in LDS
  int rx0, ry0, rx1, ry1;
  int tx0, ty0;
  u32 cls;
  template <int N>
  __device__ __forceinline__ void get(int X, int py, u32 (&cv)[N == 16 ? 4 : 2]) const {
    const uint8_t* p = lab + (py - ty0) * kTile + (X - tx0);
    if constexpr (N == 16) {
      // (X - tx0 is a multiple of 16 for every 16-pixel piece: an aligned 16-byte DS read)
      const uint4 q = *(const uint4*)p;
      const u32 c4 = cls * 0x01010101u;
      cv[0] = eq_bytes(q.x, c4), cv[1] = eq_bytes(q.y, c4), cv[2] = eq_bytes(q.z, c4), cv[3] = eq_bytes(q.w, c4);
    } else {
      cv[0] = cv[1] = 0u;
#pragma unroll
      for (int k = 0; k < N; ++k)
        if ((u32)p[k] == cls)
          cv[k / 4] |= 0xffu << (8 * (k % 4));
    }
  }
};

// lane tid's 16-byte piece of the label tile (piece tid of its 256: row tid / 4) in the label surface: the bytes of it
// inside the image area, 0 without label surfaces
__device__ __forceinline__ int label_piece(const vali_surface* d_labels, int f, int tid, int tx0, int ty0, int W, int H,
                                           uint8_t*& lp) {
  lp = nullptr;
  if (!d_labels)
    return 0;
  const vali_surface* l = d_labels + f;
  const int py = ty0 + (tid >> 2), X = tx0 + 16 * (tid & 3);
  lp = (uint8_t*)l->plane[0] + (size_t)py * (size_t)l->pitch[0] + X;
  return py < H ? max(min(W - X, 16), 0) : 0;
}

// (four waves a SIMD, which is what the LDS of four workgroups a CU allows)
template <int FMT, int DT>
__global__ void __launch_bounds__(kBlock, 4) k_semantic_paint(const SemArgs a) {
  typedef TensorElem<DT> E;
  typedef typename E::Bits Bits;
  __shared__ int4 colp[kTile], rowp[kTile];
  __shared__ __attribute__((aligned(16))) float stage[kStage];
  __shared__ __attribute__((aligned(16))) uint8_t lab[kTile * kTile];
  __shared__ u32 present[8];
  constexpr int NS = nslots(FMT);

  const int f = blockIdx.y;
  const vali_surface* d = a.d_frames + f;
  const int W = d->width, H = d->height;
  const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
  if ((int)blockIdx.x >= tiles_x * tiles_y)
    return;  // the grid is sized for the batch's largest frame
  const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
  const int tx0 = txi * kTile, ty0 = tyi * kTile;
  const int tid = threadIdx.x;
  const vali_roi rc = a.rects[f];

  // steps 1 and 2: the region, and what of it this tile holds (64 bits: src_x + src_w overflows int32)
  const bool skipped = rc.src_w < 1 || rc.src_h < 1 || rc.dst_w < 1 || rc.dst_h < 1;
  const int rx0 = clampi(rc.src_x, 0, W), rx1 = clampi((long long)rc.src_x + rc.src_w, 0, W);
  const int ry0 = clampi(rc.src_y, 0, H), ry1 = clampi((long long)rc.src_y + rc.src_h, 0, H);
  const int cx0 = max(rx0, tx0), cx1 = min(rx1, tx0 + kTile), cy0 = max(ry0, ty0), cy1 = min(ry1, ty0 + kTile);
  const bool empty = skipped || cx0 >= cx1 || cy0 >= cy1;

  if (empty) {
    uint8_t* lp;
    const int ln = label_piece(a.d_labels, f, tid, tx0, ty0, W, H, lp);
    if (ln > 0)
      store16_n(lp, make_uint4(~0u, ~0u, ~0u, ~0u), ln);
    return;
  }

  // the sampler's taps of the tile's 64 columns and 64 rows; outside the region those of its nearest pixel
  if (tid < kTile) {
    const int px = min(max(tx0 + tid, cx0), cx1 - 1);
    const Tap t = axis_tap(make_axis(rc.src_x, rc.src_w, rc.dst_x, rc.dst_w, a.Ws, a.net_w), px);
    colp[tid] = make_int4(t.i0, t.i1, __float_as_int(t.t), 0);
  } else if (tid < 2 * kTile) {
    const int qy = min(max(ty0 + tid - kTile, cy0), cy1 - 1);
    const Tap t = axis_tap(make_axis(rc.src_y, rc.src_h, rc.dst_y, rc.dst_h, a.Hs, a.net_h), qy);
    rowp[tid - kTile] = make_int4(t.i0, t.i1, __float_as_int(t.t), 0);
  } else if (tid < 2 * kTile + 8) {
    present[tid - 2 * kTile] = 0u;
  }
  __syncthreads();

  // Two passes of 32 tile rows: a lane classifies kPx consecutive luma pixels of one row a pass, carrying best[] and
  // lbl[] over the classes (16 pixels a lane in one pass do not fit the registers of four waves a SIMD).
  const int one = a.C == 1 ? 1 : 0;  // step 4: C = 1 is the sign, as classes 0 and 1
  const Bits* base = (const Bits*)a.logits + (long long)f * a.sn;
  const int grp = tid & (kTile / kPx - 1);
#pragma unroll 1
  for (int pr0 = 0; pr0 < kTile; pr0 += kPassRows) {
    const int row = pr0 + tid / (kTile / kPx);
    const int py = ty0 + row, X = tx0 + kPx * grp;
    uint2* lout = (uint2*)(lab + row * kTile + kPx * grp);
    if (max(cy0, ty0 + pr0) >= min(cy1, ty0 + pr0 + kPassRows)) {  // no region pixel in these rows
      *lout = make_uint2(~0u, ~0u);
      continue;
    }
    // the footprint of the pass in the logits (the sample position is monotone in the pixel): fw x fh cells from (c0, r0)
    const int c0 = colp[0].x, fw = colp[kTile - 1].y - c0 + 1;
    const int r0 = rowp[pr0].x, fh = rowp[pr0 + kPassRows - 1].y - r0 + 1;
    const int pitch = fw | 1, cells = fh * pitch;  // an odd pitch: rows start on different banks
    const bool staged = cells <= kStage;
    const int cb = staged ? c0 : 0, rb = staged ? r0 : 0;

    u32 xo[kPx];
    float tx[kPx], best[kPx];
    int lbl[kPx];
#pragma unroll
    for (int k = 0; k < kPx; ++k) {
      const int4 cp = colp[kPx * grp + k];
      xo[k] = (u32)(cp.x - cb) | (u32)(cp.y - cb) << 16;
      tx[k] = __int_as_float(cp.z);
      best[k] = one ? 0.0f : -INFINITY, lbl[k] = 0;
    }
    const int4 rp = rowp[row];
    const int y0 = rp.x - rb, y1 = rp.y - rb;
    const float ty = __int_as_float(rp.z);

    if (staged) {
      const int area = fh * fw, chunk = min(a.C, kStage / cells);
      for (int cbase = 0; cbase < a.C; cbase += chunk) {
        const int nc = min(chunk, a.C - cbase);
        if (cbase | pr0)
          __syncthreads();  // the last chunk has been read
        const Bits* src = base + (long long)cbase * a.sc + (long long)r0 * a.sy + c0;
        for (int idx = tid; idx < nc * area; idx += kBlock) {
          const int cc = idx / area, rem = idx - cc * area;
          const int r = rem / fw, col = rem - r * fw;
          stage[cc * cells + r * pitch + col] = E::f(gload<Bits>(src + (long long)cc * a.sc + (long long)r * a.sy + col));
        }
        __syncthreads();
        for (int cc = 0; cc < nc; ++cc) {
          LdsRows rw;
          rw.stage = stage;
          rw.o0 = cc * cells + y0 * pitch, rw.o1 = cc * cells + y1 * pitch;
          classify(rw, xo, tx, ty, cbase + cc + one, best, lbl);
        }
      }
    } else {
      for (int c = 0; c < a.C; ++c) {
        TensorRows<DT> rw;
        rw.r0 = base + (long long)c * a.sc + (long long)y0 * a.sy;
        rw.r1 = base + (long long)c * a.sc + (long long)y1 * a.sy;
        classify(rw, xo, tx, ty, c + one, best, lbl);
      }
    }

    // step 2: 255 outside the region
    u32 lw[2] = {0u, 0u};
    const bool row_in = py >= ry0 && py < ry1;
#pragma unroll
    for (int k = 0; k < kPx; ++k) {
      const bool in = row_in && X + k >= rx0 && X + k < rx1;
      lw[k / 4] |= (u32)(in ? lbl[k] : 255) << (8 * (k % 4));
    }
    *lout = make_uint2(lw[0], lw[1]);
  }
  __syncthreads();

  // step 6: the labels leave as 16-byte pieces; the classes present are collected on the way
  {
    // (formed here, not before the passes: nothing of it is kept in registers through the class loops)
    uint8_t* lp;
    const int ln = label_piece(a.d_labels, f, tid, tx0, ty0, W, H, lp);
    const uint4 q = *(const uint4*)(lab + tid * 16);
    if (ln > 0)
      store16_n(lp, q, ln);
    if (!a.colours)
      return;
    const u32 w[4] = {q.x, q.y, q.z, q.w};
    u32 prev = 255u;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const u32 l = (w[k / 4] >> (8 * (k % 4))) & 0xffu;
      if (l != 255u && l != prev)
        atomicOr(&present[l >> 5], 1u << (l & 31u));
      prev = l;
    }
  }
  __syncthreads();

  // step 5: the lane's pieces, one STAMP blend per class present, ascending
  Piece pc[NS];
  u32 cur[NS][4], orig[NS][4];
#define VALI_SLOT(S) load_piece<FMT, S>(d, tid, tx0, ty0, W, H, pc[S], cur[S], orig[S]);
  VALI_SLOTS(VALI_SLOT)
#undef VALI_SLOT

  for (int w = 0; w < 8; ++w) {
    u32 bits = (u32)__builtin_amdgcn_readfirstlane((int)present[w]);
    while (bits) {
      const int cls = 32 * w + __builtin_ctz(bits);
      bits &= bits - 1u;
      const u32 colour = (u32)a.colours[cls % a.n_colours];
      const u32 alpha = a.alpha >= 0 ? (u32)a.alpha : colour >> 24;
      if (alpha == 0u)
        continue;  // a_eff = 0: every sample stays as it is
      // (spelled out as in k_annotate: see there)
      const u32 cr = (colour >> 16) & 0xffu, cg = (colour >> 8) & 0xffu, cbl = colour & 0xffu;
      u32 col[3];
      if constexpr (a_isyuv(FMT)) {
        const float fr = (float)cr, fg = (float)cg, fb = (float)cbl;
#pragma unroll
        for (int k = 0; k < 3; ++k)
          col[k] = quantize_u8(dot_rgb(a.m[k], fr, fg, fb));
      } else if constexpr (FMT == A_BGR) {
        col[0] = cbl, col[1] = cg, col[2] = cr;
      } else {
        col[0] = cr, col[1] = cg, col[2] = cbl;
      }
      LabelCov h;
      h.lab = lab;
      h.rx0 = cx0, h.ry0 = cy0, h.rx1 = cx1, h.ry1 = cy1;
      h.tx0 = tx0, h.ty0 = ty0;
      h.cls = (u32)cls;
#define VALI_SLOT(S) cover_piece<FMT, S>(h, pc[S], col, alpha, cur[S]);
      VALI_SLOTS(VALI_SLOT)
#undef VALI_SLOT
    }
  }

  // only what a class changed goes back
#define VALI_SLOT(S) store_piece(pc[S], cur[S], orig[S]);
  VALI_SLOTS(VALI_SLOT)
#undef VALI_SLOT
}
#undef VALI_SLOTS

template <int FMT>
void launch_semantic(const dim3& grid, hipStream_t s, const SemArgs& a, int dtype) {
  with_float_dtype(dtype, [&](auto dt) { hipLaunchKernelGGL((k_semantic_paint<FMT, dt>), grid, dim3(kBlock), 0, s, a); });
}

} // namespace
} // namespace vali

using namespace vali;

extern "C" {

int vali_semantic_paint(const vali_surface* frames, const vali_surface* d_frames, int n, int format,
                        const vali_semantic_in* in, const vali_roi* d_rects, const vali_surface* labels,
                        const vali_surface* d_labels, const int32_t* d_colours, int n_colours, int alpha,
                        const vali_cvt_params* params, vali_stream_t stream) {
  VALI_REQUIRE(frames && d_frames && in && d_rects, "null argument");
  VALI_REQUIRE((labels != nullptr) == (d_labels != nullptr), "labels and d_labels: both or neither");
  VALI_REQUIRE(d_labels || d_colours, "neither labels nor colours: nothing to do");
  VALI_REQUIRE(n >= 1 && n <= kMaxN, "n outside 1..1024");
  VALI_REQUIRE(in->c >= 1 && in->c <= kMaxC, "c outside 1..255");
  VALI_REQUIRE(in->hs >= 1 && in->hs <= kMaxS && in->ws >= 1 && in->ws <= kMaxS, "hs or ws outside 1..4096");
  VALI_REQUIRE(in->net_w >= 1 && in->net_w <= 65535 && in->net_h >= 1 && in->net_h <= 65535,
               "net_w or net_h outside 1..65535");
  const vali_mask_tensor& t = in->logits;
  const int64_t strides[3] = {t.stride_n, t.stride_m, t.stride_y};
  int rc = check_head_tensor(__func__, "logits", t.data, t.dtype, strides, 3);
  if (rc != VALI_OK)
    return rc;
  VALI_REQUIRE(!d_colours || n_colours >= 1, "n_colours below 1");
  VALI_REQUIRE(alpha >= -1 && alpha <= 255, "alpha outside -1..255");
  VALI_REQUIRE((((uintptr_t)d_rects | (uintptr_t)d_colours) & 3u) == 0, "rects or colours are not 4-byte aligned");
  int tiles = 0;
  rc = check_frames(__func__, n, frames, format, &tiles);
  if (rc != VALI_OK)
    return rc;
  const int fmt = tile_format(format);
  VALI_REQUIRE(params || !d_colours || !a_isyuv(fmt), "a YUV format needs params (rgb2yuv)");
  for (int i = 0; labels && i < n; ++i) {
    const vali_surface& l = labels[i];
    if (l.format != VALI_FMT_Y)
      return fail(VALI_ERR_INVALID_ARG, "%s: label surface %d has format %d, not Y", __func__, i, l.format);
    if (l.width != frames[i].width || l.height != frames[i].height)
      return fail(VALI_ERR_INVALID_ARG, "%s: label surface %d is %dx%d, its frame %dx%d", __func__, i, l.width, l.height,
                  frames[i].width, frames[i].height);
    if (!l.plane[0])
      return fail(VALI_ERR_INVALID_ARG, "%s: label surface %d: plane 0 is null", __func__, i);
    if (l.pitch[0] < l.width)
      return fail(VALI_ERR_INVALID_ARG, "%s: label surface %d: pitch %d is shorter than a row", __func__, i, l.pitch[0]);
  }

  SemArgs a = {};
  a.d_frames = d_frames, a.d_labels = d_labels, a.rects = d_rects, a.colours = d_colours;
  a.logits = t.data, a.sn = t.stride_n, a.sc = t.stride_m, a.sy = t.stride_y;
  a.n = n, a.C = in->c, a.Hs = in->hs, a.Ws = in->ws, a.net_w = in->net_w, a.net_h = in->net_h;
  a.n_colours = d_colours ? n_colours : 1, a.alpha = alpha;
  if (d_colours && a_isyuv(fmt))
    for (int k = 0; k < 3; ++k)
      for (int j = 0; j < 4; ++j)
        a.m[k][j] = params->rgb2yuv[k][j];

  hipStream_t s = as_stream(stream);
  VALI_ENTRY(s);
  const dim3 grid(tiles, n);
  with_tile_format(fmt, [&](auto f) { launch_semantic<f>(grid, s, a, t.dtype); });
  VALI_LAUNCH_CHECK();
  return VALI_OK;
}

} // extern "C"
