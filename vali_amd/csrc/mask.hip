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
//                   mask changed it.  The blend is STAMP's (annotate.hip: stamp_piece) with the coverage made on the fly.
// The small helpers of annotate.hip (pieces, the blend, t / 255, the colour conversion) are restated here: that file's
// kernels stay as they are.
#include <math.h>

#include "common.hpp"
#include "dev_util.hpp"

#pragma clang fp contract(off)

namespace vali {
namespace {

constexpr int kTile = 64;  // luma pixels a side (launch 2)
constexpr int kLogW = 64, kLogH = 16;  // prototype pixels a tile (launch 1)
constexpr int kMaxN = 1024, kMaxM = 64, kMaxP = 1024, kMaxK = 1 << 20, kMaxD = 1024;

enum MaskFmt : int { A_NV12 = 0, A_YUV420 = 1, A_YUV444 = 2, A_RGB = 3, A_BGR = 4, A_RGBP = 5 };

constexpr bool a_is420(int f) { return f == A_NV12 || f == A_YUV420; }
constexpr bool a_isyuv(int f) { return f == A_NV12 || f == A_YUV420 || f == A_YUV444; }

// A lane's share of the tile (annotate.hip): piece (lane + first) of plane `plane`, whose bytes interleave `nc` channels
// starting with colour channel c0 at 1 >> sh samples per pixel
struct Slot {
  int plane, nc, sh, c0, first;
};
constexpr int nslots(int f) { return f == A_NV12 ? 2 : 3; }
constexpr Slot slot_of(int f, int s) {
  return (f == A_RGB || f == A_BGR) ? Slot{0, 3, 0, 0, s * kBlock}
         : f == A_NV12              ? (s == 0 ? Slot{0, 1, 0, 0, 0} : Slot{1, 2, 1, 1, 0})
         : f == A_YUV420            ? Slot{s, 1, s ? 1 : 0, s, 0}
                                    : Slot{s, 1, 0, s, 0};
}

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

__device__ __forceinline__ float elem_f(const void* p, int dt, long long i) {
  if (dt == VALI_DTYPE_F32)
    return ((const float*)p)[i];
  const u32 b = ((const uint16_t*)p)[i];
  return dt == VALI_DTYPE_F16 ? (float)__builtin_bit_cast(_Float16, (uint16_t)b) : __uint_as_float(b << 16);
}

__device__ __forceinline__ void load_row(const int32_t* dets, int i, int (&r)[8]) {
  const uint4 a = load16_u((const uint8_t*)(dets + (size_t)i * 8)), b = load16_u((const uint8_t*)(dets + (size_t)i * 8) + 16);
  r[0] = (int)a.x, r[1] = (int)a.y, r[2] = (int)a.z, r[3] = (int)a.w;
  r[4] = (int)b.x, r[5] = (int)b.y, r[6] = (int)b.z, r[7] = (int)b.w;
}

__device__ __forceinline__ int clampi(long long v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : (int)v; }

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
    cf[tid] = elem_f(a.coeffs, a.cdt, (long long)f * a.cn + (long long)o.k * a.ck + (long long)tid * a.cm);
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
// what a lane keeps of one of its pieces (annotate.hip)
struct Piece {
  uint8_t* p;  // where it lives
  int n;       // bytes of it inside the image area: 0 (none: the lane has no such piece) .. 16
  int y;       // its row, in samples of its plane
  int bx;      // its first byte within the plane's row
  int lbx;     // ... and within the tile's row
};

// t / 255 for 0 <= t < 65536
__device__ __forceinline__ u32 div255(u32 t) { return (t * 0x8081u) >> 23; }

__device__ __forceinline__ float dot_rgb(const float (&m)[4], float r, float g, float b) {
  return __builtin_fmaf(m[2], b, __builtin_fmaf(m[1], g, __builtin_fmaf(m[0], r, m[3])));
}

// Ordered compaction over the workgroup: the flagged lanes' values go to out[base ...] in lane order; returns the new
// end.  Every lane of the workgroup calls it.
__device__ __forceinline__ int compact_put(bool flag, int value, uint16_t* out, int base, int* wtot) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const unsigned long long b = __ballot(flag);
  const int before = __popcll(b & ((1ull << lane) - 1ull));
  if (lane == 0)
    wtot[wave] = __popcll(b);
  __syncthreads();
  int off = base, tot = 0;
#pragma unroll
  for (int w = 0; w < kWavesPerBlock; ++w) {
    const int c = wtot[w];
    off += w < wave ? c : 0;
    tot += c;
  }
  if (flag)
    out[off + before] = (uint16_t)value;
  __syncthreads();
  return base + tot;
}

// the colour of byte b of a piece is c[b % nc]: packed RGB pieces start at any of the three channels
template <int FMT, int S>
__device__ __forceinline__ void piece_colours(int lbx, const u32 (&col)[3], u32 (&c)[3]) {
  constexpr Slot sl = slot_of(FMT, S);
  constexpr int nc = sl.nc;
  if constexpr (nc == 3) {
    const u32 ch0 = (u32)lbx % 3u;
    const unsigned long long pk = (unsigned long long)(col[0] | col[1] << 8 | col[2] << 16 | col[0] << 24) |
                                  (unsigned long long)col[1] << 32;
    c[0] = (u32)(pk >> (8u * ch0)) & 0xffu, c[1] = (u32)(pk >> (8u * ch0 + 8u)) & 0xffu;
    c[2] = (u32)(pk >> (8u * ch0 + 16u)) & 0xffu;
  } else if constexpr (nc == 2) {
    c[0] = col[sl.c0], c[1] = col[sl.c0 + 1], c[2] = 0;
  } else {
    c[0] = col[sl.c0], c[1] = 0, c[2] = 0;
  }
}

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

// annotate.hip's stamp_piece, the weights from mask_cov
template <int FMT, int S>
__device__ __forceinline__ void mask_piece(const Hit& h, const Piece& pc, const u32 (&col)[3], u32 alpha, u32 (&w)[4]) {
  constexpr Slot sl = slot_of(FMT, S);
  constexpr int nc = sl.nc, sh = sl.sh;
  // the luma pixels under the piece: `span` columns from X, 1 << sh rows from Y
  constexpr int span = nc == 3 ? 6 : (16 / nc) << sh;
  const int X = nc == 3 ? pc.bx / 3 : (pc.bx / nc) << sh, Y = pc.y << sh;
  if (pc.n <= 0 || Y >= h.ry1 || Y + (1 << sh) <= h.ry0 || X >= h.rx1 || X + span <= h.rx0)
    return;
  u32 k[4] = {0u, 0u, 0u, 0u};  // the weight of every byte of the piece
  if constexpr (nc == 3) {
    // byte b belongs to pixel (ch0 + b) / 3 of the six, ch0 the channel the piece starts with
    u32 cv[2];
    mask_cov<6>(h, X, Y, cv);
    if ((cv[0] | cv[1]) == 0u)
      return;
    const u32 ch0 = (u32)pc.bx - 3u * (u32)X;
    const u32 e0 = __builtin_amdgcn_perm(0u, cv[0], 0x01000000u), e1 = __builtin_amdgcn_perm(0u, cv[0], 0x02020101u);
    const u32 e2 = __builtin_amdgcn_perm(0u, cv[0], 0x03030302u), e3 = __builtin_amdgcn_perm(0u, cv[1], 0x01000000u);
    const u32 e4 = __builtin_amdgcn_perm(0u, cv[1], 0x01010101u);
    k[0] = __builtin_amdgcn_alignbyte(e1, e0, ch0), k[1] = __builtin_amdgcn_alignbyte(e2, e1, ch0);
    k[2] = __builtin_amdgcn_alignbyte(e3, e2, ch0), k[3] = __builtin_amdgcn_alignbyte(e4, e3, ch0);
  } else if constexpr (sh == 0) {
    mask_cov<16>(h, X, Y, k);
  } else {
    // a 4:2:0 chroma sample: the rounded mean of the coverage of its four luma pixels, two 16-bit sums to a word
#pragma unroll
    for (int g = 0; g < span / 16; ++g) {
      u32 r0[4], r1[4];
      mask_cov<16>(h, X + 16 * g, Y, r0);
      mask_cov<16>(h, X + 16 * g, Y + 1, r1);
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const u32 sum = (r0[d] & 0xff00ffu) + ((r0[d] >> 8) & 0xff00ffu) + (r1[d] & 0xff00ffu) + ((r1[d] >> 8) & 0xff00ffu);
        const u32 q = ((sum + 0x20002u) >> 2) & 0xff00ffu;
        if constexpr (nc == 2)
          k[d] = q | q << 8;  // U and V of a sample share its weight
        else
          k[2 * g + d / 2] |= ((q | q >> 8) & 0xffffu) << (16 * (d % 2));
      }
    }
  }
  if ((k[0] | k[1] | k[2] | k[3]) == 0u)
    return;
  u32 c[3];
  piece_colours<FMT, S>(pc.lbx, col, c);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    u32 out = w[q];
#pragma unroll
    for (int b = 4 * q; b < 4 * q + 4; ++b) {
      const u32 ae = div255(((k[q] >> (8 * (b % 4))) & 0xffu) * alpha + 127u);
      const u32 v = (w[q] >> (8 * (b % 4))) & 0xffu;
      const u32 nv = div255(v * (255u - ae) + c[b % nc] * ae + 127u);  // ae = 0: v
      out = (out & ~(0xffu << (8 * (b % 4)))) | (nv << (8 * (b % 4)));
    }
    w[q] = out;
  }
}

// a lane's piece S of the tile at (tx0, ty0): where it is, how much of it the image holds, and its bytes
template <int FMT, int S>
__device__ __forceinline__ void load_piece(const vali_surface* d, int tid, int tx0, int ty0, int W, int H, Piece& pc,
                                           u32 (&cur)[4], u32 (&orig)[4]) {
  constexpr Slot sl = slot_of(FMT, S);
  constexpr int rows = kTile >> sl.sh, row_pieces = rows * sl.nc / 16;
  const int k = tid + sl.first;
  const int prow = k / row_pieces, pcol = k - prow * row_pieces;
  pc.y = (ty0 >> sl.sh) + prow;
  pc.lbx = pcol * 16;
  pc.bx = (tx0 >> sl.sh) * sl.nc + pc.lbx;
  const int row_bytes = (W >> sl.sh) * sl.nc;
  pc.n = (k < row_pieces * rows && pc.y < (H >> sl.sh)) ? max(min(row_bytes - pc.bx, 16), 0) : 0;
  pc.p = (uint8_t*)d->plane[sl.plane] + (size_t)pc.y * (size_t)d->pitch[sl.plane] + pc.bx;
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (pc.n > 0)
    v = load16_n(pc.p, pc.n);
  cur[0] = orig[0] = v.x, cur[1] = orig[1] = v.y, cur[2] = orig[2] = v.z, cur[3] = orig[3] = v.w;
}

__device__ __forceinline__ void store_piece(const Piece& pc, const u32 (&cur)[4], const u32 (&orig)[4]) {
  const bool changed = ((cur[0] ^ orig[0]) | (cur[1] ^ orig[1]) | (cur[2] ^ orig[2]) | (cur[3] ^ orig[3])) != 0u;
  if (pc.n > 0 && changed)
    store16_n(pc.p, make_uint4(cur[0], cur[1], cur[2], cur[3]), pc.n);
}

// once per slot of the format: a slot's layout is a template argument, so the slots are spelled out, not looped over
#define VALI_SLOTS(CALL)    \
  {                         \
    CALL(0)                 \
    CALL(1)                 \
    if constexpr (NS > 2) { \
      CALL(2)               \
    }                       \
  }

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
    Hit h;
    h.L = a.ws + (size_t)row * (size_t)a.Hp * (size_t)a.Wp;
    h.Wp = a.Wp;
    h.rx0 = o.x0, h.ry0 = o.y0, h.rx1 = o.x1, h.ry1 = o.y1;
    h.tx0 = tx0, h.ty0 = ty0;
    h.colp = colp, h.rowp = rowp;
#define VALI_SLOT(S) mask_piece<FMT, S>(h, pc[S], col, alpha, cur[S]);
    VALI_SLOTS(VALI_SLOT)
#undef VALI_SLOT
  }

  // only what a mask changed goes back
#define VALI_SLOT(S) store_piece(pc[S], cur[S], orig[S]);
  VALI_SLOTS(VALI_SLOT)
#undef VALI_SLOT
}
#undef VALI_SLOTS

int mask_format(int format) {
  switch (format) {
  case VALI_FMT_NV12: return A_NV12;
  case VALI_FMT_YUV420: return A_YUV420;
  case VALI_FMT_YUV444: return A_YUV444;
  case VALI_FMT_RGB: return A_RGB;
  case VALI_FMT_BGR: return A_BGR;
  case VALI_FMT_RGB_PLANAR: return A_RGBP;
  default: return -1;
  }
}

// vali_annotate_batch's rules for the frames of a batch; *max_tiles: the tiles of the largest one
int check_frames(const char* who, int n, const vali_surface* frames, int format, int* max_tiles) {
  const int fmt = mask_format(format);
  if (fmt < 0)
    return fail(VALI_ERR_UNSUPPORTED, "%s: format %d (NV12, YUV420, YUV444, RGB, BGR, RGB_PLANAR)", who, format);
  const int planes = (fmt == A_RGB || fmt == A_BGR) ? 1 : fmt == A_NV12 ? 2 : 3;
  int tiles = 0;
  for (int i = 0; i < n; ++i) {
    const vali_surface& s = frames[i];
    if (s.format != format)
      return fail(VALI_ERR_INVALID_ARG, "%s: frame %d has format %d, the batch %d: one format per batch", who, i,
                  s.format, format);
    if (s.width < 1 || s.height < 1 || s.width > 65535 || s.height > 65535)
      return fail(VALI_ERR_INVALID_ARG, "%s: frame %d: size %dx%d outside 1..65535", who, i, s.width, s.height);
    if (!subsampled_sizes_ok(format, s.width, s.height))
      return fail(VALI_ERR_INVALID_ARG, "%s: frame %d: 4:2:0 formats need an even width and height, got %dx%d", who, i,
                  s.width, s.height);
    for (int p = 0; p < planes; ++p) {
      const Slot sl = slot_of(fmt, (fmt == A_RGB || fmt == A_BGR) ? 0 : p);
      if (!s.plane[p])
        return fail(VALI_ERR_INVALID_ARG, "%s: frame %d: plane %d is null", who, i, p);
      if (s.pitch[p] < (s.width >> sl.sh) * sl.nc)
        return fail(VALI_ERR_INVALID_ARG, "%s: frame %d: pitch %d of plane %d is shorter than a row", who, i, s.pitch[p], p);
    }
    const int t = ((s.width + kTile - 1) / kTile) * ((s.height + kTile - 1) / kTile);
    tiles = t > tiles ? t : tiles;
  }
  *max_tiles = tiles;
  return VALI_OK;
}

bool dims_ok(int n, int D, int hp, int wp) {
  return n >= 1 && n <= kMaxN && D >= 1 && D <= kMaxD && (long long)n * D <= 65535 && hp >= 1 && hp <= kMaxP && wp >= 1 &&
         wp <= kMaxP;
}

int check_tensor(const char* who, const char* name, const void* data, int dtype, int64_t s0, int64_t s1, int64_t s2) {
  if (!data)
    return fail(VALI_ERR_INVALID_ARG, "%s: %s has a null pointer", who, name);
  if (dtype != VALI_DTYPE_F32 && dtype != VALI_DTYPE_F16 && dtype != VALI_DTYPE_BF16)
    return fail(VALI_ERR_INVALID_ARG, "%s: %s: dtype %d is not float32, float16 or bfloat16", who, name, dtype);
  const int es = dtype == VALI_DTYPE_F32 ? 4 : 2;
  if (((uintptr_t)data & (uintptr_t)(es - 1)) != 0)
    return fail(VALI_ERR_INVALID_ARG, "%s: %s is not aligned to its element size", who, name);
  const int64_t lim = (int64_t)1 << 40;
  if (s0 < 0 || s1 < 0 || s2 < 0 || s0 > lim || s1 > lim || s2 > lim)
    return fail(VALI_ERR_INVALID_ARG, "%s: %s: strides (%lld, %lld, %lld) outside 0..2^40", who, name, (long long)s0,
                (long long)s1, (long long)s2);
  return VALI_OK;
}

template <int FMT>
void launch_paint(const dim3& grid, hipStream_t s, const MaskArgs& a) {
  hipLaunchKernelGGL((k_mask_paint<FMT>), grid, dim3(kBlock), 0, s, a);
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
  int rc = check_tensor(__func__, "protos", in->protos.data, in->protos.dtype, in->protos.stride_n, in->protos.stride_m,
                        in->protos.stride_y);
  if (rc != VALI_OK)
    return rc;
  rc = check_tensor(__func__, "coeffs", in->coeffs.data, in->coeffs.dtype, in->coeffs.stride_n, in->coeffs.stride_k,
                    in->coeffs.stride_c);
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
  const int fmt = mask_format(format);
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
  switch (a.pdt) {
  case VALI_DTYPE_F32: hipLaunchKernelGGL(k_mask_logits<VALI_DTYPE_F32>, lgrid, dim3(kBlock), 0, s, a); break;
  case VALI_DTYPE_F16: hipLaunchKernelGGL(k_mask_logits<VALI_DTYPE_F16>, lgrid, dim3(kBlock), 0, s, a); break;
  default: hipLaunchKernelGGL(k_mask_logits<VALI_DTYPE_BF16>, lgrid, dim3(kBlock), 0, s, a); break;
  }
  VALI_LAUNCH_CHECK();
  const dim3 grid(tiles, n);
  switch (fmt) {
  case A_NV12: launch_paint<A_NV12>(grid, s, a); break;
  case A_YUV420: launch_paint<A_YUV420>(grid, s, a); break;
  case A_YUV444: launch_paint<A_YUV444>(grid, s, a); break;
  case A_RGB: launch_paint<A_RGB>(grid, s, a); break;
  case A_BGR: launch_paint<A_BGR>(grid, s, a); break;
  default: launch_paint<A_RGBP>(grid, s, a); break;
  }
  VALI_LAUNCH_CHECK();
  return VALI_OK;
}

} // extern "C"
