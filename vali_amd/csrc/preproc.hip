// Fused inference pre-processing: NV12 -> (bilinear resize) -> RGB -> float -> normalised,
// planar or packed, in ONE pass.
//
// The reference has no such kernel; its samples and tests/test_TorchSegmentation.py:176-240
// run the chain
//   PySurfaceConverter NV12 -> RGB            (nppiNV12ToRGB*_8u_P2C3R)
//   PySurfaceConverter RGB -> RGB_32F         (nppiScale_8u32f_C3R: v / 255)
//   PySurfaceConverter RGB_32F -> RGB_32F_PLANAR
//   torch.divide(x, 255.0) ; torchvision Normalize: (x - mean[c]) / std[c]
// (optionally behind a PySurfaceResizer), i.e. three to four surface launches plus two torch
// kernels and ~80 bytes of HBM traffic per pixel.  Here: 1.5 B read + 12 B written per pixel.
//
// DEFINITION = that chain, step by step, so the result is bit-identical to running the chain
// with this library's own kernels (tests/test_gpu_preproc.py checks exactly that):
//   1. sizes differ: NV12' = bilinear resize of the Y plane and of the interleaved UV plane on
//      the grid src = dst * (src_size / dst_size), each rounded half-even to u8 (resize.hip)
//   2. q_c = the u8 RGB of cvt_nv12_rgb.hip (vali_csc coefficients, round-half-even, saturate)
//   3. out_c = ((q_c / 255.0f) / div - mean[c]) / std[c]            three IEEE divisions
// Step 3 depends only on (c, q): each workgroup evaluates it ONCE for all 3 x 256 inputs into
// an LDS table with exactly those operations and every pixel then costs one ds_read_b32 --
// same bits, no per-pixel divisions.
//
// Work decomposition: lane = 4 dst px x 2 rows (one chroma sample pair per row pair), so each
// planar store instruction is one float4 per lane = 1 KiB contiguous per wave; a workgroup
// covers 1024 x 8 dst pixels (the 4 waves side by side, each walking 4 row pairs, so a plane
// row leaves the workgroup as 4 KiB contiguous) and the table is built once per workgroup.  Same-size inputs stream (dword luma loads); resized inputs gather their taps
// through L1/L2 (the destination of a network input is small, the traffic is the source).
// Oracle: composition of vali_oracle_resize_plane, vali_oracle_nv12_to_rgb and float32
// numpy arithmetic (tests/test_gpu_preproc.py, tests/test_oracle_preproc.py).
#include "common.hpp"
#include "dev_util.hpp"
#include "tensor_out.hpp"

namespace vali {

struct PreprocArgs {
  const vali_surface* d_src;
  const vali_surface* d_dst;
  vali_surface src, dst;
  vali_preproc_params prm;
  TileMap map;
  int row_pairs; // dst row pairs a wave walks: kPpRowPairsPerWave, or 2 / 1 when the launch is small
};

constexpr int kPpRowPairsPerWave = 4;
constexpr int kPpTileH = kPpRowPairsPerWave * 2;                 // 8 dst rows
constexpr int kPpTileW = kWavesPerBlock * kWave * 4;             // 1024 dst px: the 4 waves sit side by side

// SAME = source and destination sizes are equal (decided on the host): that instantiation
// carries none of the resize code and fits twice as many waves per SIMD.
// OUT: destination layout.  The float layouts apply step 3 through the table; the 8-bit ones
// stop after step 2 (resize + colour conversion only: the other two-task chain of the samples).
enum : int { PP_F32_PLANAR = 0, PP_F32_PACKED = 1, PP_U8_RGB = 2, PP_U8_BGR = 3, PP_U8_PLANAR = 4 };

template <bool SAME, int OUT>
__global__ void __launch_bounds__(kBlock) k_nv12_preproc(const PreprocArgs a) {
  constexpr bool kFloat = OUT == PP_F32_PLANAR || OUT == PP_F32_PACKED;
  __shared__ float lut[kFloat ? 3 : 1][256];
  u32 tile_x, tile_y, frame;
  if (!tile_of_block(a.map, tile_x, tile_y, frame))
    return;
  if constexpr (kFloat) {
    // step 3 for every (channel, u8 value)
    for (int e = threadIdx.x; e < 3 * 256; e += kBlock) {
      const int c = e >> 8, q = e & 255;
      const float f = (float)q / 255.0f;
      const float g = f / a.prm.div;
      lut[c][q] = (g - a.prm.mean[c]) / a.prm.std_[c];
    }
    __syncthreads();
  }

  const SurfRef s = load_surface(a.d_src, a.src, frame);
  const SurfRef d = load_surface(a.d_dst, a.dst, frame);
  const uint8_t* py = s.p[0];
  const uint8_t* puv = s.p[1];
  const int sp_y = s.pitch[0], sp_uv = s.pitch[1], sw = s.width, sh = s.height;
  const int dw = d.width, dh = d.height, dp = d.pitch[0];
  const vali_csc k = a.prm.csc;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int x0 = tile_x * kPpTileW + (wave * kWave + lane) * 4;
  if (x0 >= dw)
    return;
  const int n = min(4, dw - x0); // dw is even: n is 2 or 4
  constexpr bool same = SAME;
  const bool fast_luma = same && ((((uintptr_t)py) | (uintptr_t)sp_y | ((uintptr_t)puv) | (uintptr_t)sp_uv) & 3u) == 0;

  // resize geometry (resize.hip): per plane scale = src_size / dst_size
  const float lsx = (float)sw / (float)dw, lsy = (float)sh / (float)dh;
  const float csx = (float)(sw >> 1) / (float)(dw >> 1), csy = (float)(sh >> 1) / (float)(dh >> 1);
  Lerp lx[4], cxl[2];
  if constexpr (!same) {
#pragma unroll
    for (int p = 0; p < 4; ++p)
      lx[p] = make_lerp(min(x0 + p, dw - 1), lsx, sw);
#pragma unroll
    for (int j = 0; j < 2; ++j)
      cxl[j] = make_lerp(min((x0 >> 1) + j, (dw >> 1) - 1), csx, sw >> 1);
  }

#pragma unroll 1
  for (int it = 0; it < a.row_pairs; ++it) {
    const int y0 = (tile_y * a.row_pairs + it) * 2; // wave-uniform
    if (y0 >= dh)
      break;
    // ---- the resized NV12' texels of this lane: 2 x 4 luma, 2 chroma pairs ----
    float yv[2][4], uu[2], vv[2];
    if constexpr (same) {
      const uint8_t* r0 = py + (u32)(y0 * sp_y) + x0;
      const uint8_t* r1 = py + (u32)((y0 + 1) * sp_y) + x0;
      const uint8_t* rc = puv + (u32)((y0 >> 1) * sp_uv) + x0;
      u32 w0, w1, wc;
      if (fast_luma && n == 4) {
        w0 = gload<u32>(r0); w1 = gload<u32>(r1); wc = gload<u32>(rc);
      } else {
        w0 = w1 = wc = 0;
        for (int p = 0; p < n; ++p) {
          w0 |= (u32)gload<uint8_t>(r0 + p) << (8 * p);
          w1 |= (u32)gload<uint8_t>(r1 + p) << (8 * p);
          wc |= (u32)gload<uint8_t>(rc + p) << (8 * p);
        }
      }
      yv[0][0] = ubyte_f32<0>(w0); yv[0][1] = ubyte_f32<1>(w0); yv[0][2] = ubyte_f32<2>(w0); yv[0][3] = ubyte_f32<3>(w0);
      yv[1][0] = ubyte_f32<0>(w1); yv[1][1] = ubyte_f32<1>(w1); yv[1][2] = ubyte_f32<2>(w1); yv[1][3] = ubyte_f32<3>(w1);
      uu[0] = ubyte_f32<0>(wc); vv[0] = ubyte_f32<1>(wc); uu[1] = ubyte_f32<2>(wc); vv[1] = ubyte_f32<3>(wc);
    } else {
      // bilinear taps, arithmetic of resize_tile (t0, t1, v; then round-half-even to u8)
      // The two horizontal taps are neighbours (i1 = min(i0 + 1, last)), so a row's pair comes from
      // ONE (unaligned) load -- 2 bytes of luma, 4 bytes = two UV pairs of chroma: 20 vector-memory
      // instructions per lane and row pair instead of 48; the texture addresser was this path's
      // bound (profiles/r01_ud_down2.md: ~16 cycles per wave instruction whatever its width).
      // At the right edge (i0 = last) the load starts one texel earlier and both taps take its
      // second half.
      typedef uint16_t u16_unaligned __attribute__((aligned(1)));
      typedef u32 u32_unaligned __attribute__((aligned(1)));
      auto lerp3 = [](float t00, float t10, float t01, float t11, float ax, float ay) {
        const float t0 = __builtin_fmaf(ax, t10 - t00, t00);
        const float t1 = __builtin_fmaf(ax, t11 - t01, t01);
        return (float)quantize_u8(__builtin_fmaf(ay, t1 - t0, t0));
      };
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const Lerp ly = make_lerp(min(y0 + r, dh - 1), lsy, sh);
        const uint8_t* r0 = py + (size_t)ly.i0 * sp_y;
        const uint8_t* r1 = py + (size_t)ly.i1 * sp_y;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int base = min(lx[p].i0, sw - 2);
          const bool edge = lx[p].i0 != base;
          const u32 w0 = *(const VALI_GLOBAL u16_unaligned*)(r0 + base);
          const u32 w1 = *(const VALI_GLOBAL u16_unaligned*)(r1 + base);
          const float t10 = (float)(w0 >> 8), t11 = (float)(w1 >> 8);
          const float t00 = edge ? t10 : (float)(w0 & 0xffu), t01 = edge ? t11 : (float)(w1 & 0xffu);
          yv[r][p] = lerp3(t00, t10, t01, t11, lx[p].a, ly.a);
        }
      }
      const Lerp cy = make_lerp(y0 >> 1, csy, sh >> 1);
      const uint8_t* c0 = puv + (size_t)cy.i0 * sp_uv;
      const uint8_t* c1 = puv + (size_t)cy.i1 * sp_uv;
      if (sw >= 4) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int base = min(cxl[j].i0, (sw >> 1) - 2);
          const bool edge = cxl[j].i0 != base;
          const u32 w0 = *(const VALI_GLOBAL u32_unaligned*)(c0 + 2 * base); // U V U' V'
          const u32 w1 = *(const VALI_GLOBAL u32_unaligned*)(c1 + 2 * base);
          const float u10 = ubyte_f32<2>(w0), v10 = ubyte_f32<3>(w0), u11 = ubyte_f32<2>(w1), v11 = ubyte_f32<3>(w1);
          const float u00 = edge ? u10 : ubyte_f32<0>(w0), v00 = edge ? v10 : ubyte_f32<1>(w0);
          const float u01 = edge ? u11 : ubyte_f32<0>(w1), v01 = edge ? v11 : ubyte_f32<1>(w1);
          uu[j] = lerp3(u00, u10, u01, u11, cxl[j].a, cy.a);
          vv[j] = lerp3(v00, v10, v01, v11, cxl[j].a, cy.a);
        }
      } else { // a 2-pixel-wide source has ONE chroma pair per row: no neighbour to fetch with it
        const float u0 = (float)gload<uint8_t>(c0), v0 = (float)gload<uint8_t>(c0 + 1);
        const float u1 = (float)gload<uint8_t>(c1), v1 = (float)gload<uint8_t>(c1 + 1);
        uu[0] = uu[1] = lerp3(u0, u0, u1, u1, 0.0f, cy.a);
        vv[0] = vv[1] = lerp3(v0, v0, v1, v1, 0.0f, cy.a);
      }
    }
    // ---- step 2 + 3 ----
    const ChromaTerm ct[2] = {chroma_term(uu[0], vv[0], k), chroma_term(uu[1], vv[1], k)};
    if constexpr (kFloat) {
      float o[2][3][4]; // [row][channel][pixel]
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const float yf = luma_term(yv[r][p], k);
          const ChromaTerm& c = ct[p >> 1];
          o[r][0][p] = lut[0][quantize_u8(yf + c.rv)];
          o[r][1][p] = lut[1][quantize_u8(yf + c.guv)];
          o[r][2][p] = lut[2][quantize_u8(yf + c.bu)];
        }
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int y = y0 + r;
        if (y >= dh)
          break;
        if constexpr (OUT == PP_F32_PLANAR) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            uint8_t* q = d.p[c] + (u32)(y * dp) + (size_t)x0 * 4;
            // a wave writes 1 KiB, the workgroup 4 KiB contiguous per plane row: non-temporal pays
            // in this layout (5.55 -> 5.29 us at 1080p; it cost 5-9 % with 256 x 32 tiles)
            if (n == 4 && (((uintptr_t)q) & 15u) == 0)
              store16f_nt(q, make_float4(o[r][c][0], o[r][c][1], o[r][c][2], o[r][c][3]));
            else
              for (int p = 0; p < n; ++p) gstore<float>(q + 4 * p, o[r][c][p]);
          }
        } else {
          uint8_t* q = d.p[0] + (u32)(y * dp) + (size_t)x0 * 12;
          if (n == 4 && (((uintptr_t)q) & 15u) == 0) {
            store16f(q + 0, make_float4(o[r][0][0], o[r][1][0], o[r][2][0], o[r][0][1]));
            store16f(q + 16, make_float4(o[r][1][1], o[r][2][1], o[r][0][2], o[r][1][2]));
            store16f(q + 32, make_float4(o[r][2][2], o[r][0][3], o[r][1][3], o[r][2][3]));
          } else {
            for (int p = 0; p < n; ++p) {
              gstore<float>(q + 12 * p, o[r][0][p]); gstore<float>(q + 12 * p + 4, o[r][1][p]); gstore<float>(q + 12 * p + 8, o[r][2][p]);
            }
          }
        }
      }
    } else {
      // 8-bit outputs: the quantised bytes themselves
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int y = y0 + r;
        if (y >= dh)
          break;
        float cr[4], cg[4], cb[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const float yf = luma_term(yv[r][p], k);
          const ChromaTerm& c = ct[p >> 1];
          cr[p] = yf + c.rv; cg[p] = yf + c.guv; cb[p] = yf + c.bu;
        }
        if constexpr (OUT == PP_U8_PLANAR) {
          u32 w[3] = {0u, 0u, 0u};
          w[0] = pack_u8<0>(cr[0], w[0]); w[0] = pack_u8<1>(cr[1], w[0]); w[0] = pack_u8<2>(cr[2], w[0]); w[0] = pack_u8<3>(cr[3], w[0]);
          w[1] = pack_u8<0>(cg[0], w[1]); w[1] = pack_u8<1>(cg[1], w[1]); w[1] = pack_u8<2>(cg[2], w[1]); w[1] = pack_u8<3>(cg[3], w[1]);
          w[2] = pack_u8<0>(cb[0], w[2]); w[2] = pack_u8<1>(cb[1], w[2]); w[2] = pack_u8<2>(cb[2], w[2]); w[2] = pack_u8<3>(cb[3], w[2]);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            uint8_t* q = d.p[c] + (u32)(y * dp) + x0;
            if (n == 4 && (((uintptr_t)q) & 3u) == 0)
              gstore<u32>(q, w[c]);
            else
              for (int p = 0; p < n; ++p) gstore<uint8_t>(q + p, (uint8_t)(w[c] >> (8 * p)));
          }
        } else {
          // memory order f g l per pixel: f = R (RGB) or B (BGR), l the other one
          const float (&cf)[4] = OUT == PP_U8_RGB ? cr : cb;
          const float (&cl)[4] = OUT == PP_U8_RGB ? cb : cr;
          u32 d0 = 0u, d1 = 0u, d2 = 0u;
          d0 = pack_u8<0>(cf[0], d0); d0 = pack_u8<1>(cg[0], d0); d0 = pack_u8<2>(cl[0], d0); d0 = pack_u8<3>(cf[1], d0);
          d1 = pack_u8<0>(cg[1], d1); d1 = pack_u8<1>(cl[1], d1); d1 = pack_u8<2>(cf[2], d1); d1 = pack_u8<3>(cg[2], d1);
          d2 = pack_u8<0>(cl[2], d2); d2 = pack_u8<1>(cf[3], d2); d2 = pack_u8<2>(cg[3], d2); d2 = pack_u8<3>(cl[3], d2);
          uint8_t* q = d.p[0] + (u32)(y * dp) + (size_t)x0 * 3;
          if (n == 4 && (((uintptr_t)q) & 3u) == 0) {
            typedef unsigned v3u32 __attribute__((ext_vector_type(3)));
            const v3u32 w = {d0, d1, d2};
            *(VALI_GLOBAL v3u32*)q = w;
          } else {
            const u32 ww[3] = {d0, d1, d2};
            for (int b = 0; b < 3 * n; ++b) gstore<uint8_t>(q + b, (uint8_t)(ww[b >> 2] >> (8 * (b & 3))));
          }
        }
      }
    }
  }
}

static int launch_preproc(PreprocArgs& a, int src_w, int src_h, int dst_w, int dst_h, int dst_fmt, int n,
                          hipStream_t stream) {
  int out;
  switch (dst_fmt) {
  case VALI_FMT_RGB_32F_PLANAR: out = PP_F32_PLANAR; break;
  case VALI_FMT_RGB_32F: out = PP_F32_PACKED; break;
  case VALI_FMT_RGB: out = PP_U8_RGB; break;
  case VALI_FMT_BGR: out = PP_U8_BGR; break;
  case VALI_FMT_RGB_PLANAR: out = PP_U8_PLANAR; break;
  default:
    return fail(VALI_ERR_UNSUPPORTED,
                "nv12_preproc: destination must be RGB_32F[_PLANAR], RGB, BGR or RGB_PLANAR (got %d)", dst_fmt);
  }
  // Row pairs per wave: 4, or 2 / 1 while that would leave SIMDs without a wave (the pairs of a wave run one memory round
  // trip after the other: ONE 1080p -> 640x384 frame took 8.3 us through 4-pair waves, 48 workgroups on 256 CUs).
  a.row_pairs = kPpRowPairsPerWave;
  {
    const int forced = tuning(VALI_TUNE_ROWS_PER_WAVE); // 2 / 4 / 8 dst rows
    const long long tiles_x = (dst_w + kPpTileW - 1) / kPpTileW;
    if (forced == 2 || forced == 4 || forced == 8)
      a.row_pairs = forced / 2;
    else
      while (a.row_pairs > 1 && tiles_x * ((dst_h + 2 * a.row_pairs - 1) / (2 * a.row_pairs)) * n * kWavesPerBlock < 2048)
        a.row_pairs /= 2;
  }
  a.map = make_tile_map((dst_w + kPpTileW - 1) / kPpTileW, (dst_h + 2 * a.row_pairs - 1) / (2 * a.row_pairs), (u32)n);
  const dim3 grid = tile_grid(a.map), block(kBlock);
  const bool same = src_w == dst_w && src_h == dst_h;
#define VALI_PP_CASE(O)                                                                      \
  case O:                                                                                   \
    if (same)                                                                               \
      hipLaunchKernelGGL((k_nv12_preproc<true, O>), grid, block, 0, stream, a);              \
    else                                                                                    \
      hipLaunchKernelGGL((k_nv12_preproc<false, O>), grid, block, 0, stream, a);             \
    break;
  switch (out) {
    VALI_PP_CASE(PP_F32_PLANAR)
    VALI_PP_CASE(PP_F32_PACKED)
    VALI_PP_CASE(PP_U8_RGB)
    VALI_PP_CASE(PP_U8_BGR)
    VALI_PP_CASE(PP_U8_PLANAR)
  }
#undef VALI_PP_CASE
  VALI_LAUNCH_CHECK();
  return VALI_OK;
}

// ---- regions: crop -> place inside a canvas, the rest padded or left alone -------------------
// Item i: crop (sx, sy, sw, sh) of src[i] onto place (dx, dy, dw, dh) of dst[i].  Inside the
// placement every pixel is k_nv12_preproc's on view(src, crop) -> view(dst, place): the same
// make_lerp grid on scales (float)sw / (float)dw, the same one-load two-tap fetch, quantisation
// and table.  Equal crop and placement sizes take the same path: the scale is exactly 1, every
// tap weight 0, and the lerp returns the texel itself.  Outside it: the pad colour, or nothing.
// The rectangles are workgroup-uniform: loaded with scalar loads and sanitised in SGPRs, so a
// device-supplied record can never move an access outside the item's own surfaces.
// Tiles: 4 px x 2 rows per lane as in k_nv12_preproc.  WIDE: the 4 waves side by side (1024 px);
// TALL (canvases of at most 256 px, the classifier inputs): each wave spans the canvas and the
// 4 waves take consecutive row pairs -- a 224-wide canvas keeps 7 of 8 lanes busy instead of 1 of 5.
struct RoiArgs {
  const vali_surface* d_src;
  const vali_surface* d_dst;
  const vali_roi* d_roi;
  vali_surface src, dst;
  vali_roi roi;
  vali_preproc_params prm;
  TileMap map;
  int row_pairs; // row pairs a wave walks
  int pad;       // 0: pixels outside the placement are not written
  u32 pad_rgb;   // R | G << 8 | B << 16
  vali_tensor_dst tdst; // the tensor forms (DST != TD_SURF): the destination of every item, instead of d_dst / dst
  int whole;            // the tensor forms of NV12: no rectangle records, every item is its whole source onto the canvas
};

// DST: where the float outputs go.  TD_SURF: the items' own surfaces (d_dst / dst), float32.  TD_F32 / TD_F16 / TD_BF16:
// ONE batch tensor of that element type (a.tdst; OUT names its layout: PP_F32_PLANAR x stride 1, PP_F32_PACKED channels
// last).  The 16-bit forms convert WHEN THE TABLE IS FILLED (a u16 table) and convert the pad colour once: the per-pixel
// path moves finished bits and contains no conversion, so each element is convert(the float32 of the surface form) by
// construction.
enum : int { TD_SURF = 0, TD_F32 = 1, TD_F16 = 2, TD_BF16 = 3 };

// a table entry / an output element of the form DST: the float itself, or the finished 16 bits
template <int DST> struct TdElem {
  typedef float lut_t;
  typedef float val_t;
  static __device__ __forceinline__ float make(float v) { return v; }
};
template <> struct TdElem<TD_F16> {
  typedef uint16_t lut_t;
  typedef u32 val_t;
  static __device__ __forceinline__ u32 make(float v) { return f32_to_f16_bits(v); }
};
template <> struct TdElem<TD_BF16> {
  typedef uint16_t lut_t;
  typedef u32 val_t;
  static __device__ __forceinline__ u32 make(float v) { return f32_to_bf16_bits(v); }
};

// the 16-bit stores of one lane and row: 4 elements of a plane (8 bytes) / its 4 channels-last pixels (24 bytes) as
// 8-byte stores when the lane has all 4 pixels and the address is 8-byte aligned, single elements under wr[] otherwise
// (a view whose rows start 2, 4 or 6 bytes off): every access naturally aligned
__device__ __forceinline__ void store_h4_planar(uint8_t* q, const u32 (&o)[4], bool full, const bool (&wr)[4]) {
  if (full && (((uintptr_t)q) & 7u) == 0) {
    const v2u32 w = {o[0] | o[1] << 16, o[2] | o[3] << 16};
    gstore_nt<v2u32>(q, w); // a wave writes 512 contiguous bytes: whole lines, as the f32 planar form
  } else {
#pragma unroll
    for (int p = 0; p < 4; ++p)
      if (wr[p]) gstore<uint16_t>(q + 2 * p, (uint16_t)o[p]);
  }
}
__device__ __forceinline__ void store_h4_packed(uint8_t* q, const u32 (&o)[3][4], bool full, const bool (&wr)[4]) {
  if (full && (((uintptr_t)q) & 7u) == 0) {
    const v2u32 w0 = {o[0][0] | o[1][0] << 16, o[2][0] | o[0][1] << 16};
    const v2u32 w1 = {o[1][1] | o[2][1] << 16, o[0][2] | o[1][2] << 16};
    const v2u32 w2 = {o[2][2] | o[0][3] << 16, o[1][3] | o[2][3] << 16};
    gstore<v2u32>(q, w0); gstore<v2u32>(q + 8, w1); gstore<v2u32>(q + 16, w2);
  } else {
#pragma unroll
    for (int p = 0; p < 4; ++p)
      if (wr[p]) {
        gstore<uint16_t>(q + 6 * p, (uint16_t)o[0][p]); gstore<uint16_t>(q + 6 * p + 2, (uint16_t)o[1][p]);
        gstore<uint16_t>(q + 6 * p + 4, (uint16_t)o[2][p]);
      }
  }
}

__device__ __forceinline__ SurfRef surf_ref(const vali_surface& v) {
  SurfRef r;
  r.p[0] = (uint8_t*)v.plane[0]; r.p[1] = (uint8_t*)v.plane[1]; r.p[2] = (uint8_t*)v.plane[2];
  r.pitch[0] = v.pitch[0]; r.pitch[1] = v.pitch[1]; r.pitch[2] = v.pitch[2];
  r.width = v.width; r.height = v.height;
  return r;
}

// clamp (x, w) into [0, size], both even (the batch form's sanitising rule)
__device__ __forceinline__ void roi_clamp(int& x, int& w, int size) {
  size = max(size, 0);
  x = min(max(x, 0), size) & ~1;
  w = min(max(w, 0), size - x) & ~1;
}

template <int OUT, bool TALL, int DST = TD_SURF>
__global__ void __launch_bounds__(kBlock) k_nv12_preproc_roi(const RoiArgs a) {
  constexpr bool kFloat = OUT == PP_F32_PLANAR || OUT == PP_F32_PACKED;
  constexpr bool kHalf = DST == TD_F16 || DST == TD_BF16; // 16-bit elements: finished bits from the table on
  static_assert(DST == TD_SURF || kFloat, "the tensor forms are float layouts");
  constexpr int kTileW = TALL ? kWave * 4 : kPpTileW;
  typedef TdElem<DST> Elem;
  __shared__ typename Elem::lut_t lut[kFloat ? 3 : 1][256];
  u32 tile_x, tile_y, frame;
  if (!tile_of_block(a.map, tile_x, tile_y, frame))
    return;
  const SurfRef s = surf_ref(load_uniform(a.d_src, frame, &a.src));
  SurfRef d;
  if constexpr (DST == TD_SURF)
    d = surf_ref(load_uniform(a.d_dst, frame, &a.dst));
  else
    d = tensor_ref<kHalf ? 2 : 4>(a.tdst, frame);
  const vali_roi r = load_uniform(a.d_roi, frame, &a.roi);
  int sx = r.src_x, sy = r.src_y, sw = r.src_w, sh = r.src_h;
  int dx = r.dst_x, dy = r.dst_y, dw = r.dst_w, dh = r.dst_h;
  if constexpr (DST != TD_SURF) {
    if (a.whole) {
      sx = sy = dx = dy = 0;
      sw = s.width; sh = s.height; dw = d.width; dh = d.height;
    }
  }
  roi_clamp(sx, sw, s.width);
  roi_clamp(sy, sh, s.height);
  const int cw = max(d.width, 0) & ~1, ch = max(d.height, 0) & ~1; // the canvas
  roi_clamp(dx, dw, cw);
  roi_clamp(dy, dh, ch);
  const bool empty = sw < 2 || sh < 2 || dw < 2 || dh < 2;

  // does this workgroup's tile meet the placement?  (block-uniform)
  const int tx0 = tile_x * kTileW;
  const int ty0 = tile_y * a.row_pairs * (TALL ? 8 : 2);
  const int th = a.row_pairs * (TALL ? 8 : 2);
  const bool hits = !empty && tx0 < dx + dw && tx0 + kTileW > dx && ty0 < dy + dh && ty0 + th > dy;
  if (!hits && !a.pad)
    return;
  if constexpr (kFloat) {
    if (hits) {
      for (int e = threadIdx.x; e < 3 * 256; e += kBlock)
        lut[e >> 8][e & 255] = Elem::make(normalise_u8(e & 255, e >> 8, a.prm));
      __syncthreads();
    }
  }

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int x0 = tx0 + (TALL ? 0 : wave * kWave * 4) + lane * 4;
  if (x0 >= cw)
    return;
  const int n = min(4, cw - x0); // cw is even: n is 2 or 4
  // the lane's two pixel pairs (x0, x0 + 1) and (x0 + 2, x0 + 3): dx, dw and x0 are even, so each
  // pair is wholly inside or wholly outside the placement
  const bool in0 = hits && x0 >= dx && x0 < dx + dw;
  const bool in1 = hits && x0 + 2 >= dx && x0 + 2 < dx + dw;
  // the pad colour: the normalised value (float outputs; its finished bits for 16-bit elements) or the byte (8-bit outputs)
  typename Elem::val_t pv[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int q = (a.pad_rgb >> (8 * c)) & 255u;
    const auto v = kFloat ? Elem::make(normalise_u8(q, c, a.prm)) : Elem::make((float)q);
    pv[c] = __builtin_bit_cast(typename Elem::val_t, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); // uniform: SGPRs
  }

  // the view of the crop, and the resize geometry of view -> view (k_nv12_preproc's expressions)
  const int sp_y = s.pitch[0], sp_uv = s.pitch[1], dp = d.pitch[0];
  const uint8_t* py = s.p[0] + (size_t)sy * sp_y + sx;
  const uint8_t* puv = s.p[1] + (size_t)(sy >> 1) * sp_uv + sx;
  const vali_csc k = a.prm.csc;
  const float lsx = (float)sw / (float)dw, lsy = (float)sh / (float)dh;
  const float csx = (float)(sw >> 1) / (float)(dw >> 1), csy = (float)(sh >> 1) / (float)(dh >> 1);
  const int vx0 = x0 - dx; // the lane's first pixel in view coordinates (even; clamped below for pad lanes)
  const bool same = sw == dw && sh == dh; // item-uniform
  Lerp lx[4], cxl[2];
#pragma unroll
  for (int p = 0; p < 4; ++p)
    lx[p] = make_lerp(min(max(vx0 + p, 0), dw - 1), lsx, sw);
#pragma unroll
  for (int j = 0; j < 2; ++j)
    cxl[j] = make_lerp(min(max((vx0 >> 1) + j, 0), (dw >> 1) - 1), csx, sw >> 1);

#pragma unroll 1
  for (int it = 0; it < a.row_pairs; ++it) {
    const int y0 = TALL ? ty0 + (it * kWavesPerBlock + wave) * 2 : ty0 + it * 2; // wave-uniform
    if (y0 >= ch)
      break;
    const bool row_in = y0 >= dy && y0 < dy + dh; // both rows of the pair (dy, dh even)
    const bool c0 = row_in && in0, c1 = row_in && in1;
    if (!a.pad && !c0 && !c1)
      continue;
    // which of the 4 pixels this lane stores, and is that all of them
    const bool w01 = c0 || a.pad, w23 = c1 || a.pad;
    const bool full = n == 4 && w01 && w23;
    float yv[2][4], uu[2], vv[2];
    if (same && c0 && c1) {
      // ---- equal sizes, all 4 pixels inside: the taps are the texels themselves (scale 1, weights 0), so the
      // lane streams them as k_nv12_preproc<true, *> does -- one dword per row and one of chroma (any alignment:
      // the crop and the placement may each sit at 2 mod 4) ----
      const int vy0 = y0 - dy;
      const u32 w0 = gload_u<u32>(py + (size_t)vy0 * sp_y + vx0);
      const u32 w1 = gload_u<u32>(py + (size_t)(vy0 + 1) * sp_y + vx0);
      const u32 wc = gload_u<u32>(puv + (size_t)(vy0 >> 1) * sp_uv + vx0);
      yv[0][0] = ubyte_f32<0>(w0); yv[0][1] = ubyte_f32<1>(w0); yv[0][2] = ubyte_f32<2>(w0); yv[0][3] = ubyte_f32<3>(w0);
      yv[1][0] = ubyte_f32<0>(w1); yv[1][1] = ubyte_f32<1>(w1); yv[1][2] = ubyte_f32<2>(w1); yv[1][3] = ubyte_f32<3>(w1);
      uu[0] = ubyte_f32<0>(wc); vv[0] = ubyte_f32<1>(wc); uu[1] = ubyte_f32<2>(wc); vv[1] = ubyte_f32<3>(wc);
    } else if (c0 || c1) {
      // ---- bilinear taps of k_nv12_preproc<false, *> on the view ----
      typedef uint16_t u16_unaligned __attribute__((aligned(1)));
      typedef u32 u32_unaligned __attribute__((aligned(1)));
      auto lerp3 = [](float t00, float t10, float t01, float t11, float ax, float ay) {
        const float t0 = __builtin_fmaf(ax, t10 - t00, t00);
        const float t1 = __builtin_fmaf(ax, t11 - t01, t01);
        return (float)quantize_u8(__builtin_fmaf(ay, t1 - t0, t0));
      };
      const int vy0 = y0 - dy;
#pragma unroll
      for (int rr = 0; rr < 2; ++rr) {
        const Lerp ly = make_lerp(min(vy0 + rr, dh - 1), lsy, sh);
        const uint8_t* r0 = py + (size_t)ly.i0 * sp_y;
        const uint8_t* r1 = py + (size_t)ly.i1 * sp_y;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int base = min(lx[p].i0, sw - 2);
          const bool edge = lx[p].i0 != base;
          const u32 w0 = *(const VALI_GLOBAL u16_unaligned*)(r0 + base);
          const u32 w1 = *(const VALI_GLOBAL u16_unaligned*)(r1 + base);
          const float t10 = (float)(w0 >> 8), t11 = (float)(w1 >> 8);
          const float t00 = edge ? t10 : (float)(w0 & 0xffu), t01 = edge ? t11 : (float)(w1 & 0xffu);
          yv[rr][p] = lerp3(t00, t10, t01, t11, lx[p].a, ly.a);
        }
      }
      const Lerp cy = make_lerp(vy0 >> 1, csy, sh >> 1);
      const uint8_t* q0 = puv + (size_t)cy.i0 * sp_uv;
      const uint8_t* q1 = puv + (size_t)cy.i1 * sp_uv;
      if (sw >= 4) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int base = min(cxl[j].i0, (sw >> 1) - 2);
          const bool edge = cxl[j].i0 != base;
          const u32 w0 = *(const VALI_GLOBAL u32_unaligned*)(q0 + 2 * base); // U V U' V'
          const u32 w1 = *(const VALI_GLOBAL u32_unaligned*)(q1 + 2 * base);
          const float u10 = ubyte_f32<2>(w0), v10 = ubyte_f32<3>(w0), u11 = ubyte_f32<2>(w1), v11 = ubyte_f32<3>(w1);
          const float u00 = edge ? u10 : ubyte_f32<0>(w0), v00 = edge ? v10 : ubyte_f32<1>(w0);
          const float u01 = edge ? u11 : ubyte_f32<0>(w1), v01 = edge ? v11 : ubyte_f32<1>(w1);
          uu[j] = lerp3(u00, u10, u01, u11, cxl[j].a, cy.a);
          vv[j] = lerp3(v00, v10, v01, v11, cxl[j].a, cy.a);
        }
      } else { // a 2-pixel-wide crop has ONE chroma pair per row
        const float u0 = (float)gload<uint8_t>(q0), v0 = (float)gload<uint8_t>(q0 + 1);
        const float u1 = (float)gload<uint8_t>(q1), v1 = (float)gload<uint8_t>(q1 + 1);
        uu[0] = uu[1] = lerp3(u0, u0, u1, u1, 0.0f, cy.a);
        vv[0] = vv[1] = lerp3(v0, v0, v1, v1, 0.0f, cy.a);
      }
    } else {
#pragma unroll
      for (int rr = 0; rr < 2; ++rr)
#pragma unroll
        for (int p = 0; p < 4; ++p) yv[rr][p] = 0.0f;
      uu[0] = uu[1] = vv[0] = vv[1] = 128.0f;
    }
    // ---- step 2 + 3, the pad colour where the pixel lies outside the placement ----
    const ChromaTerm ct[2] = {chroma_term(uu[0], vv[0], k), chroma_term(uu[1], vv[1], k)};
    // (the two rows stay a rolled loop: unrolled, the packed float form holds both rows' 24 values at once)
#pragma unroll 1
    for (int rr = 0; rr < 2; ++rr) {
      const int y = y0 + rr;
      typename Elem::val_t o[3][4]; // [channel][pixel]: float outputs the final value, 8-bit outputs the pre-quantised one
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const bool inside = p < 2 ? c0 : c1;
        const float yf = luma_term(rr ? yv[1][p] : yv[0][p], k);
        const ChromaTerm& c = ct[p >> 1];
        if constexpr (kFloat) {
          o[0][p] = inside ? lut[0][quantize_u8(yf + c.rv)] : pv[0];
          o[1][p] = inside ? lut[1][quantize_u8(yf + c.guv)] : pv[1];
          o[2][p] = inside ? lut[2][quantize_u8(yf + c.bu)] : pv[2];
        } else {
          o[0][p] = inside ? yf + c.rv : pv[0];
          o[1][p] = inside ? yf + c.guv : pv[1];
          o[2][p] = inside ? yf + c.bu : pv[2];
        }
      }
      auto writes = [&](int p) { return p < n && (p < 2 ? w01 : w23); };
      if constexpr (kHalf) {
        const bool wr[4] = {writes(0), writes(1), writes(2), writes(3)};
        if constexpr (OUT == PP_F32_PLANAR) {
#pragma unroll
          for (int c = 0; c < 3; ++c)
            store_h4_planar(d.p[c] + (u32)(y * dp) + (size_t)x0 * 2, o[c], full, wr);
        } else {
          store_h4_packed(d.p[0] + (u32)(y * dp) + (size_t)x0 * 6, o, full, wr);
        }
      } else if constexpr (OUT == PP_F32_PLANAR) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          uint8_t* q = d.p[c] + (u32)(y * dp) + (size_t)x0 * 4;
          if (full && (((uintptr_t)q) & 15u) == 0)
            store16f_nt(q, make_float4(o[c][0], o[c][1], o[c][2], o[c][3]));
          else
            for (int p = 0; p < 4; ++p)
              if (writes(p)) gstore<float>(q + 4 * p, o[c][p]);
        }
      } else if constexpr (OUT == PP_F32_PACKED) {
        uint8_t* q = d.p[0] + (u32)(y * dp) + (size_t)x0 * 12;
        if (full && (((uintptr_t)q) & 15u) == 0) {
          store16f(q + 0, make_float4(o[0][0], o[1][0], o[2][0], o[0][1]));
          store16f(q + 16, make_float4(o[1][1], o[2][1], o[0][2], o[1][2]));
          store16f(q + 32, make_float4(o[2][2], o[0][3], o[1][3], o[2][3]));
        } else { // per pixel pair (the unit that is inside or outside): 24 bytes each
          if (writes(0)) {
            gstore<float>(q + 0, o[0][0]); gstore<float>(q + 4, o[1][0]); gstore<float>(q + 8, o[2][0]);
            gstore<float>(q + 12, o[0][1]); gstore<float>(q + 16, o[1][1]); gstore<float>(q + 20, o[2][1]);
          }
          if (writes(2)) {
            gstore<float>(q + 24, o[0][2]); gstore<float>(q + 28, o[1][2]); gstore<float>(q + 32, o[2][2]);
            gstore<float>(q + 36, o[0][3]); gstore<float>(q + 40, o[1][3]); gstore<float>(q + 44, o[2][3]);
          }
        }
      } else if constexpr (OUT == PP_U8_PLANAR) {
        u32 w[3] = {0u, 0u, 0u};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          w[c] = pack_u8<0>(o[c][0], w[c]); w[c] = pack_u8<1>(o[c][1], w[c]);
          w[c] = pack_u8<2>(o[c][2], w[c]); w[c] = pack_u8<3>(o[c][3], w[c]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          uint8_t* q = d.p[c] + (u32)(y * dp) + x0;
          if (full && (((uintptr_t)q) & 3u) == 0)
            gstore<u32>(q, w[c]);
          else
            for (int p = 0; p < 4; ++p)
              if (writes(p)) gstore<uint8_t>(q + p, (uint8_t)(w[c] >> (8 * p)));
        }
      } else {
        // memory order f g l per pixel: f = R (RGB) or B (BGR), l the other one
        const float (&cf)[4] = OUT == PP_U8_RGB ? o[0] : o[2];
        const float (&cg)[4] = o[1];
        const float (&cl)[4] = OUT == PP_U8_RGB ? o[2] : o[0];
        u32 d0 = 0u, d1 = 0u, d2 = 0u;
        d0 = pack_u8<0>(cf[0], d0); d0 = pack_u8<1>(cg[0], d0); d0 = pack_u8<2>(cl[0], d0); d0 = pack_u8<3>(cf[1], d0);
        d1 = pack_u8<0>(cg[1], d1); d1 = pack_u8<1>(cl[1], d1); d1 = pack_u8<2>(cf[2], d1); d1 = pack_u8<3>(cg[2], d1);
        d2 = pack_u8<0>(cl[2], d2); d2 = pack_u8<1>(cf[3], d2); d2 = pack_u8<2>(cg[3], d2); d2 = pack_u8<3>(cl[3], d2);
        uint8_t* q = d.p[0] + (u32)(y * dp) + (size_t)x0 * 3;
        if (full && (((uintptr_t)q) & 3u) == 0) {
          typedef unsigned v3u32 __attribute__((ext_vector_type(3)));
          const v3u32 wv = {d0, d1, d2};
          *(VALI_GLOBAL v3u32*)q = wv;
        } else {
          const u32 ww[3] = {d0, d1, d2};
          for (int b = 0; b < 12; ++b)
            if (writes(b / 3)) gstore<uint8_t>(q + b, (uint8_t)(ww[b >> 2] >> (8 * (b & 3))));
        }
      }
    }
  }
}

// td: TD_SURF, or the element type of the batch tensor a.tdst (dst_fmt then names its layout)
static int launch_preproc_roi(RoiArgs& a, int canvas_w, int canvas_h, int dst_fmt, int n, hipStream_t stream,
                              int td = TD_SURF) {
  int out;
  switch (dst_fmt) {
  case VALI_FMT_RGB_32F_PLANAR: out = PP_F32_PLANAR; break;
  case VALI_FMT_RGB_32F: out = PP_F32_PACKED; break;
  case VALI_FMT_RGB: out = PP_U8_RGB; break;
  case VALI_FMT_BGR: out = PP_U8_BGR; break;
  case VALI_FMT_RGB_PLANAR: out = PP_U8_PLANAR; break;
  default:
    return fail(VALI_ERR_UNSUPPORTED,
                "nv12_preproc_roi: destination must be RGB_32F[_PLANAR], RGB, BGR or RGB_PLANAR (got %d)", dst_fmt);
  }
  // the tile shape follows the canvas width: narrow canvases stack the waves (see RoiArgs)
  const bool tall = canvas_w <= kWave * 4;
  const int tile_w = tall ? kWave * 4 : kPpTileW, rows_per_pair_step = tall ? 2 * kWavesPerBlock : 2;
  const long long tiles_x = (canvas_w + tile_w - 1) / tile_w;
  // row pairs per wave: 4, or 2 / 1 while that would leave SIMDs without a wave (launch_preproc's rule)
  a.row_pairs = kPpRowPairsPerWave;
  auto tiles_y = [&](int rp) { return (canvas_h + rows_per_pair_step * rp - 1) / (rows_per_pair_step * rp); };
  while (a.row_pairs > 1 && tiles_x * tiles_y(a.row_pairs) * n * kWavesPerBlock < 2048)
    a.row_pairs /= 2;
  a.map = make_tile_map((u32)tiles_x, (u32)tiles_y(a.row_pairs), (u32)n);
  const dim3 grid = tile_grid(a.map), block(kBlock);
#define VALI_PPR_LAUNCH(O, D)                                                                \
  do {                                                                                      \
    if (tall)                                                                               \
      hipLaunchKernelGGL((k_nv12_preproc_roi<O, true, D>), grid, block, 0, stream, a);      \
    else                                                                                    \
      hipLaunchKernelGGL((k_nv12_preproc_roi<O, false, D>), grid, block, 0, stream, a);     \
  } while (0)
#define VALI_PPR_CASE(O)                                                                     \
  case O: VALI_PPR_LAUNCH(O, TD_SURF); break;
#define VALI_PPT_CASE(D)                                                                     \
  case D:                                                                                   \
    if (out == PP_F32_PLANAR) VALI_PPR_LAUNCH(PP_F32_PLANAR, D); else VALI_PPR_LAUNCH(PP_F32_PACKED, D); \
    break;
  if (td != TD_SURF) {
    switch (td) {
      VALI_PPT_CASE(TD_F32)
      VALI_PPT_CASE(TD_F16)
      VALI_PPT_CASE(TD_BF16)
    }
  } else {
    switch (out) {
      VALI_PPR_CASE(PP_F32_PLANAR)
      VALI_PPR_CASE(PP_F32_PACKED)
      VALI_PPR_CASE(PP_U8_RGB)
      VALI_PPR_CASE(PP_U8_BGR)
      VALI_PPR_CASE(PP_U8_PLANAR)
    }
  }
#undef VALI_PPT_CASE
#undef VALI_PPR_CASE
#undef VALI_PPR_LAUNCH
  VALI_LAUNCH_CHECK();
  return VALI_OK;
}

// ---- regions of RGB-family sources (RGB, BGR, RGB_PLANAR; 8 bit) ------------------------------
// The same item as above without a colour matrix and without evenness: inside the placement
//   q_c = the bilinear resize of view(src, crop) to dw x dh, channel by channel (resize.hip's arithmetic and grid),
//   out = step 3 on q_R, q_G, q_B (float outputs) or the bytes themselves (8-bit outputs),
// i.e. vali_resize(LINEAR) on the views, then the plain converters, then the normalisation.
// A lane owns 4 px of ONE row (no chroma couples rows or columns here), so every predicate is per pixel.
// Fetch: the two horizontal taps of a packed pixel are 6 contiguous bytes at 3 (sx + i0), any alignment: ONE
// 8-byte load per tap row (its window slides left at the end of the SURFACE row and is shifted back in registers,
// load_tap_pair's rule), 8 loads per lane and row instead of 48.  Planar sources take 2 bytes per plane and tap row.
// Equal sizes, all 4 pixels inside: the 12 bytes (packed) / 3 x 4 bytes (planar) of the lane stream in as they lie.
// A crop that is 1 pixel wide, or a packed surface narrower than the 8-byte window (< 3 px), has one or two
// texels per row: they are gathered byte by byte into the same 6-byte form (the second texel repeats the first
// when there is only one), so the arithmetic below never knows.
// BGR sources differ from RGB ones by a channel swap where the colours are named (a.swap), not by a kernel.
struct RgbRoiArgs {
  RoiArgs r;
  int swap;  // packed source is B G R in memory
  int whole; // no rectangle records: every item is its whole source onto its whole destination
};

// clamp (x, w) into [0, size] (the batch form's sanitising rule for these sources: no rounding)
__device__ __forceinline__ void roi_clamp_any(int& x, int& w, int size) {
  size = max(size, 0);
  x = min(max(x, 0), size);
  w = min(max(w, 0), size - x);
}

template <bool PLANAR, int OUT, bool TALL, int DST = TD_SURF>
__global__ void __launch_bounds__(kBlock) k_rgb_preproc_roi(const RgbRoiArgs ar) {
  constexpr bool kFloat = OUT == PP_F32_PLANAR || OUT == PP_F32_PACKED;
  constexpr bool kHalf = DST == TD_F16 || DST == TD_BF16; // 16-bit elements: finished bits from the table on
  static_assert(DST == TD_SURF || kFloat, "the tensor forms are float layouts");
  constexpr int kTileW = TALL ? kWave * 4 : kPpTileW;
  typedef unsigned long long u64;
  typedef unsigned v3u32 __attribute__((ext_vector_type(3)));
  typedef TdElem<DST> Elem;
  const RoiArgs& a = ar.r;
  __shared__ typename Elem::lut_t lut[kFloat ? 3 : 1][256];
  u32 tile_x, tile_y, frame;
  if (!tile_of_block(a.map, tile_x, tile_y, frame))
    return;
  const SurfRef s = surf_ref(load_uniform(a.d_src, frame, &a.src));
  SurfRef d;
  if constexpr (DST == TD_SURF)
    d = surf_ref(load_uniform(a.d_dst, frame, &a.dst));
  else
    d = tensor_ref<kHalf ? 2 : 4>(a.tdst, frame);
  const vali_roi r = load_uniform(a.d_roi, frame, &a.roi);
  int sx = r.src_x, sy = r.src_y, sw = r.src_w, sh = r.src_h;
  int dx = r.dst_x, dy = r.dst_y, dw = r.dst_w, dh = r.dst_h;
  if (ar.whole) {
    sx = sy = dx = dy = 0;
    sw = s.width; sh = s.height; dw = d.width; dh = d.height;
  }
  roi_clamp_any(sx, sw, s.width);
  roi_clamp_any(sy, sh, s.height);
  const int cw = max(d.width, 0), ch = max(d.height, 0); // the canvas
  roi_clamp_any(dx, dw, cw);
  roi_clamp_any(dy, dh, ch);
  const bool empty = sw < 1 || sh < 1 || dw < 1 || dh < 1;

  // does this workgroup's tile meet the placement?  (block-uniform)
  const int rows = a.row_pairs * 2; // rows a wave walks
  const int tx0 = tile_x * kTileW;
  const int th = rows * (TALL ? kWavesPerBlock : 1);
  const int ty0 = tile_y * th;
  const bool hits = !empty && tx0 < dx + dw && tx0 + kTileW > dx && ty0 < dy + dh && ty0 + th > dy;
  if (!hits && !a.pad)
    return;
  if constexpr (kFloat) {
    if (hits) {
      for (int e = threadIdx.x; e < 3 * 256; e += kBlock)
        lut[e >> 8][e & 255] = Elem::make(normalise_u8(e & 255, e >> 8, a.prm));
      __syncthreads();
    }
  }

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int x0 = tx0 + (TALL ? 0 : wave * kWave * 4) + lane * 4;
  if (x0 >= cw)
    return;
  const int n = min(4, cw - x0);
  bool inx[4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
    inx[p] = hits && x0 + p >= dx && x0 + p < dx + dw;
  const bool any_x = inx[0] || inx[1] || inx[2] || inx[3];
  const bool all_x = inx[0] && inx[1] && inx[2] && inx[3];
  // the pad colour: the normalised value (float outputs; its finished bits for 16-bit elements); the byte itself is padq
  typename Elem::val_t pv[3];
  u32 padq[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    padq[c] = (a.pad_rgb >> (8 * c)) & 255u;
    const auto v = Elem::make(kFloat ? normalise_u8((int)padq[c], c, a.prm) : 0.0f);
    pv[c] = __builtin_bit_cast(typename Elem::val_t, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); // uniform: SGPRs
  }

  // the resize geometry of view -> view (resize_tile's expressions) and the lane's column taps
  const int sp = s.pitch[0], dp = d.pitch[0];
  const float lsx = (float)sw / (float)max(dw, 1), lsy = (float)sh / (float)max(dh, 1);
  const int vx0 = x0 - dx; // the lane's first pixel in view coordinates (clamped below for pixels outside)
  const bool same = sw == dw && sh == dh; // item-uniform
  // one or two texels per crop row: gathered byte by byte
  const bool narrow = sw == 1 || (!PLANAR && s.width < 3);
  float ax[4];
  int off[4];   // byte offset of the pixel's tap window from the start of the surface row
  int shl[4];   // packed: bits to shift the window right (it slid left at the end of the row)
  bool edge[4]; // the coordinate sits on the crop's last column: both taps are the window's second texel
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const Lerp l = make_lerp(min(max(vx0 + p, 0), max(dw - 1, 0)), lsx, max(sw, 1));
    const int base = max(min(l.i0, sw - 2), 0);
    ax[p] = l.a;
    edge[p] = l.i0 != base;
    if constexpr (PLANAR) {
      off[p] = sx + base;
      shl[p] = 0;
    } else {
      const int want = 3 * (sx + base);
      off[p] = max(min(want, 3 * s.width - 8), 0);
      shl[p] = 8 * (want - off[p]);
    }
  }

#pragma unroll 1
  for (int it = 0; it < rows; ++it) {
    const int y = TALL ? ty0 + it * kWavesPerBlock + wave : ty0 + it; // wave-uniform
    if (y >= ch)
      break;
    const bool row_in = y >= dy && y < dy + dh;
    const bool any = row_in && any_x, all = row_in && all_x;
    if (!a.pad && !any)
      continue;
    bool in[4], wr[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      in[p] = row_in && inx[p];
      wr[p] = p < n && (in[p] || a.pad);
    }
    const bool full = wr[0] && wr[1] && wr[2] && wr[3];
    u32 q[3][4]; // [channel in the source's memory order][pixel]: the resized u8 texels
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int p = 0; p < 4; ++p) q[c][p] = 0u;
    if (any) {
      const int vy = y - dy;
      if (same && all) {
        // ---- equal sizes, all 4 pixels inside: the texels themselves (scale 1, weights 0), streamed ----
        if constexpr (PLANAR) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const u32 w = gload_u<u32>(s.p[c] + (size_t)(sy + vy) * s.pitch[c] + sx + vx0);
            q[c][0] = ubyte<0>(w); q[c][1] = ubyte<1>(w); q[c][2] = ubyte<2>(w); q[c][3] = ubyte<3>(w);
          }
        } else {
          const v3u32 w = gload_u<v3u32>(s.p[0] + (size_t)(sy + vy) * sp + 3 * (sx + vx0));
          q[0][0] = ubyte<0>(w.x); q[1][0] = ubyte<1>(w.x); q[2][0] = ubyte<2>(w.x); q[0][1] = ubyte<3>(w.x);
          q[1][1] = ubyte<0>(w.y); q[2][1] = ubyte<1>(w.y); q[0][2] = ubyte<2>(w.y); q[1][2] = ubyte<3>(w.y);
          q[2][2] = ubyte<0>(w.z); q[0][3] = ubyte<1>(w.z); q[1][3] = ubyte<2>(w.z); q[2][3] = ubyte<3>(w.z);
        }
      } else {
        // ---- bilinear taps of resize_tile on the view: t0, t1 along x on the two tap rows, then along y ----
        Lerp ly = make_lerp(min(vy, dh - 1), lsy, sh);
        if (ly.a == 0.0f) // (wave-uniform) fma(0, t1 - t0, t0) == t0: integer ratios never fetch the second tap row
          ly.i1 = ly.i0;
        auto lerp3 = [](float t00, float t10, float t01, float t11, float fx, float fy) {
          const float t0 = __builtin_fmaf(fx, t10 - t00, t00);
          const float t1 = __builtin_fmaf(fx, t11 - t01, t01);
          return quantize_u8(__builtin_fmaf(fy, t1 - t0, t0));
        };
        if constexpr (PLANAR) {
          u32 w0[3][4], w1[3][4]; // tap row 0 / 1: texel | next texel << 8
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const uint8_t* r0 = s.p[c] + (size_t)(sy + ly.i0) * s.pitch[c];
            const uint8_t* r1 = s.p[c] + (size_t)(sy + ly.i1) * s.pitch[c];
            if (!narrow) {
#pragma unroll
              for (int p = 0; p < 4; ++p) {
                w0[c][p] = gload_u<uint16_t>(r0 + off[p]);
                w1[c][p] = gload_u<uint16_t>(r1 + off[p]);
              }
            } else {
              const u32 b0 = gload<uint8_t>(r0 + sx), b1 = gload<uint8_t>(r1 + sx);
#pragma unroll
              for (int p = 0; p < 4; ++p) {
                w0[c][p] = b0 | b0 << 8;
                w1[c][p] = b1 | b1 << 8;
              }
            }
          }
#pragma unroll
          for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int p = 0; p < 4; ++p) {
              const float t10 = ubyte_f32<1>(w0[c][p]), t11 = ubyte_f32<1>(w1[c][p]);
              const float t00 = edge[p] ? t10 : ubyte_f32<0>(w0[c][p]), t01 = edge[p] ? t11 : ubyte_f32<0>(w1[c][p]);
              q[c][p] = lerp3(t00, t10, t01, t11, ax[p], ly.a);
            }
        } else {
          const uint8_t* r0 = s.p[0] + (size_t)(sy + ly.i0) * sp;
          const uint8_t* r1 = s.p[0] + (size_t)(sy + ly.i1) * sp;
          u64 w0[4], w1[4]; // tap row 0 / 1: the 6 bytes of the texel and its right neighbour
          if (!narrow) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
              w0[p] = gload_u<u64>(r0 + off[p]) >> shl[p];
              w1[p] = gload_u<u64>(r1 + off[p]) >> shl[p];
            }
          } else {
            u64 n0 = 0, n1 = 0;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
              const int b = 3 * sx + (k < 3 || sw >= 2 ? k : k - 3);
              n0 |= (u64)gload<uint8_t>(r0 + b) << (8 * k);
              n1 |= (u64)gload<uint8_t>(r1 + b) << (8 * k);
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
              w0[p] = n0;
              w1[p] = n1;
            }
          }
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            const u32 lo0 = (u32)w0[p], hi0 = (u32)(w0[p] >> 32), lo1 = (u32)w1[p], hi1 = (u32)(w1[p] >> 32);
            const float t10[3] = {ubyte_f32<3>(lo0), ubyte_f32<0>(hi0), ubyte_f32<1>(hi0)};
            const float t11[3] = {ubyte_f32<3>(lo1), ubyte_f32<0>(hi1), ubyte_f32<1>(hi1)};
            const float t00[3] = {ubyte_f32<0>(lo0), ubyte_f32<1>(lo0), ubyte_f32<2>(lo0)};
            const float t01[3] = {ubyte_f32<0>(lo1), ubyte_f32<1>(lo1), ubyte_f32<2>(lo1)};
#pragma unroll
            for (int c = 0; c < 3; ++c)
              q[c][p] = lerp3(edge[p] ? t10[c] : t00[c], t10[c], edge[p] ? t11[c] : t01[c], t11[c], ax[p], ly.a);
          }
        }
      }
    }
    // ---- the colours by name, the pad colour where the pixel lies outside the placement ----
    u32 qc[3][4]; // [R, G, B][pixel]
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      qc[0][p] = in[p] ? (ar.swap ? q[2][p] : q[0][p]) : padq[0];
      qc[1][p] = in[p] ? q[1][p] : padq[1];
      qc[2][p] = in[p] ? (ar.swap ? q[0][p] : q[2][p]) : padq[2];
    }
    if constexpr (kFloat) {
      typename Elem::val_t o[3][4];
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int p = 0; p < 4; ++p) o[c][p] = in[p] ? lut[c][qc[c][p]] : pv[c];
      if constexpr (kHalf) {
        if constexpr (OUT == PP_F32_PLANAR) {
#pragma unroll
          for (int c = 0; c < 3; ++c)
            store_h4_planar(d.p[c] + (u32)(y * d.pitch[c]) + (size_t)x0 * 2, o[c], full, wr);
        } else {
          store_h4_packed(d.p[0] + (u32)(y * dp) + (size_t)x0 * 6, o, full, wr);
        }
      } else if constexpr (OUT == PP_F32_PLANAR) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          uint8_t* w = d.p[c] + (u32)(y * d.pitch[c]) + (size_t)x0 * 4;
          if (full && (((uintptr_t)w) & 15u) == 0)
            store16f_nt(w, make_float4(o[c][0], o[c][1], o[c][2], o[c][3]));
          else
#pragma unroll
            for (int p = 0; p < 4; ++p)
              if (wr[p]) gstore<float>(w + 4 * p, o[c][p]);
        }
      } else {
        uint8_t* w = d.p[0] + (u32)(y * dp) + (size_t)x0 * 12;
        if (full && (((uintptr_t)w) & 15u) == 0) {
          store16f(w + 0, make_float4(o[0][0], o[1][0], o[2][0], o[0][1]));
          store16f(w + 16, make_float4(o[1][1], o[2][1], o[0][2], o[1][2]));
          store16f(w + 32, make_float4(o[2][2], o[0][3], o[1][3], o[2][3]));
        } else {
#pragma unroll
          for (int p = 0; p < 4; ++p)
            if (wr[p]) {
              gstore<float>(w + 12 * p, o[0][p]); gstore<float>(w + 12 * p + 4, o[1][p]); gstore<float>(w + 12 * p + 8, o[2][p]);
            }
        }
      }
    } else if constexpr (OUT == PP_U8_PLANAR) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        uint8_t* w = d.p[c] + (u32)(y * d.pitch[c]) + x0;
        if (full)
          gstore_u<u32>(w, qc[c][0] | qc[c][1] << 8 | qc[c][2] << 16 | qc[c][3] << 24);
        else
#pragma unroll
          for (int p = 0; p < 4; ++p)
            if (wr[p]) gstore<uint8_t>(w + p, (uint8_t)qc[c][p]);
      }
    } else {
      // memory order f g l per pixel: f = R (RGB) or B (BGR), l the other one
      const u32 (&cf)[4] = OUT == PP_U8_RGB ? qc[0] : qc[2];
      const u32 (&cg)[4] = qc[1];
      const u32 (&cl)[4] = OUT == PP_U8_RGB ? qc[2] : qc[0];
      uint8_t* w = d.p[0] + (u32)(y * dp) + (size_t)x0 * 3;
      if (full) {
        const v3u32 wv = {cf[0] | cg[0] << 8 | cl[0] << 16 | cf[1] << 24, cg[1] | cl[1] << 8 | cf[2] << 16 | cg[2] << 24,
                          cl[2] | cf[3] << 8 | cg[3] << 16 | cl[3] << 24};
        gstore_u<v3u32>(w, wv);
      } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
          if (wr[p]) {
            gstore<uint8_t>(w + 3 * p, (uint8_t)cf[p]); gstore<uint8_t>(w + 3 * p + 1, (uint8_t)cg[p]);
            gstore<uint8_t>(w + 3 * p + 2, (uint8_t)cl[p]);
          }
      }
    }
  }
}

static int rgb_out_form(int dst_fmt) {
  switch (dst_fmt) {
  case VALI_FMT_RGB_32F_PLANAR: return PP_F32_PLANAR;
  case VALI_FMT_RGB_32F: return PP_F32_PACKED;
  case VALI_FMT_RGB: return PP_U8_RGB;
  case VALI_FMT_BGR: return PP_U8_BGR;
  case VALI_FMT_RGB_PLANAR: return PP_U8_PLANAR;
  default: return -1;
  }
}

static bool rgb_src_ok(int fmt) { return fmt == VALI_FMT_RGB || fmt == VALI_FMT_BGR || fmt == VALI_FMT_RGB_PLANAR; }

static int launch_rgb_preproc_roi(RgbRoiArgs& ar, int src_fmt, int canvas_w, int canvas_h, int dst_fmt, int n,
                                  hipStream_t stream, int td = TD_SURF) {
  RoiArgs& a = ar.r;
  const int out = rgb_out_form(dst_fmt);
  ar.swap = src_fmt == VALI_FMT_BGR;
  const bool planar = src_fmt == VALI_FMT_RGB_PLANAR;
  // tile shapes and rows per wave: launch_preproc_roi's rules
  const bool tall = canvas_w <= kWave * 4;
  const int tile_w = tall ? kWave * 4 : kPpTileW, rows_per_pair_step = tall ? 2 * kWavesPerBlock : 2;
  const long long tiles_x = (canvas_w + tile_w - 1) / tile_w;
  a.row_pairs = kPpRowPairsPerWave;
  auto tiles_y = [&](int rp) { return (canvas_h + rows_per_pair_step * rp - 1) / (rows_per_pair_step * rp); };
  while (a.row_pairs > 1 && tiles_x * tiles_y(a.row_pairs) * n * kWavesPerBlock < 2048)
    a.row_pairs /= 2;
  a.map = make_tile_map((u32)tiles_x, (u32)tiles_y(a.row_pairs), (u32)n);
  const dim3 grid = tile_grid(a.map), block(kBlock);
#define VALI_PPR_LAUNCH(P, O, T, D) hipLaunchKernelGGL((k_rgb_preproc_roi<P, O, T, D>), grid, block, 0, stream, ar)
#define VALI_PPR_FORM(O, D)                                                                  \
  do {                                                                                      \
    if (planar) {                                                                           \
      if (tall) VALI_PPR_LAUNCH(true, O, true, D); else VALI_PPR_LAUNCH(true, O, false, D); \
    } else {                                                                                \
      if (tall) VALI_PPR_LAUNCH(false, O, true, D); else VALI_PPR_LAUNCH(false, O, false, D); \
    }                                                                                       \
  } while (0)
#define VALI_PPR_CASE(O)                                                                     \
  case O: VALI_PPR_FORM(O, TD_SURF); break;
#define VALI_PPT_CASE(D)                                                                     \
  case D:                                                                                   \
    if (out == PP_F32_PLANAR) VALI_PPR_FORM(PP_F32_PLANAR, D); else VALI_PPR_FORM(PP_F32_PACKED, D); \
    break;
  if (td != TD_SURF) {
    switch (td) {
      VALI_PPT_CASE(TD_F32)
      VALI_PPT_CASE(TD_F16)
      VALI_PPT_CASE(TD_BF16)
    }
  } else {
    switch (out) {
      VALI_PPR_CASE(PP_F32_PLANAR)
      VALI_PPR_CASE(PP_F32_PACKED)
      VALI_PPR_CASE(PP_U8_RGB)
      VALI_PPR_CASE(PP_U8_BGR)
      VALI_PPR_CASE(PP_U8_PLANAR)
    }
  }
#undef VALI_PPT_CASE
#undef VALI_PPR_CASE
#undef VALI_PPR_FORM
#undef VALI_PPR_LAUNCH
  VALI_LAUNCH_CHECK();
  return VALI_OK;
}

} // namespace vali

using namespace vali;

extern "C" {

int vali_nv12_preproc(const vali_surface* src, const vali_surface* dst, const vali_preproc_params* params,
                      vali_stream_t stream) {
  VALI_REQUIRE(src && dst && params, "null argument");
  VALI_REQUIRE(src->format == VALI_FMT_NV12, "source must be NV12");
  VALI_REQUIRE(src->width >= 2 && src->height >= 2 && dst->width >= 2 && dst->height >= 2, "empty surface");
  VALI_REQUIRE(((src->width | src->height | dst->width | dst->height) & 1) == 0, "4:2:0 needs even sizes");
  VALI_REQUIRE(src->plane[0] && src->plane[1] && dst->plane[0], "null plane");
  VALI_REQUIRE(planes_fit_32bit(*src) && planes_fit_32bit(*dst), "plane of 4 GiB or more");
  if (dst->format == VALI_FMT_RGB_32F_PLANAR || dst->format == VALI_FMT_RGB_PLANAR)
    VALI_REQUIRE(dst->plane[1] && dst->plane[2], "null dst plane");
  PreprocArgs a = {};
  a.src = *src;
  a.dst = *dst;
  a.prm = *params;
  hipStream_t s = as_stream(stream);
  VALI_ENTRY(s);
  return launch_preproc(a, src->width, src->height, dst->width, dst->height, dst->format, 1, s);
}

int vali_nv12_preproc_batch(const vali_surface* d_src, const vali_surface* d_dst, int n, int src_width,
                            int src_height, int dst_width, int dst_height, int dst_format,
                            const vali_preproc_params* params, vali_stream_t stream) {
  VALI_REQUIRE(d_src && d_dst && params, "null argument");
  VALI_REQUIRE(src_width >= 2 && src_height >= 2 && dst_width >= 2 && dst_height >= 2 &&
                   ((src_width | src_height | dst_width | dst_height) & 1) == 0,
               "bad geometry");
  VALI_REQUIRE(n >= 0 && n <= 65535, "batch size out of range (0..65535)");
  if (n == 0)
    return VALI_OK;
  PreprocArgs a = {};
  a.d_src = d_src;
  a.d_dst = d_dst;
  a.prm = *params;
  hipStream_t s = as_stream(stream);
  VALI_ENTRY(s);
  return launch_preproc(a, src_width, src_height, dst_width, dst_height, dst_format, n, s);
}

static bool roi_axis_ok(int x, int w, int size) {
  return x >= 0 && w >= 2 && ((x | w) & 1) == 0 && x <= size - w;
}

int vali_nv12_preproc_roi(const vali_surface* src, const vali_surface* dst, const vali_roi* roi,
                          const vali_preproc_params* params, int pad, const uint8_t pad_rgb[3],
                          vali_stream_t stream) {
  VALI_REQUIRE(src && dst && roi && params, "null argument");
  VALI_REQUIRE(!pad || pad_rgb, "null pad colour");
  VALI_REQUIRE(src->format == VALI_FMT_NV12, "source must be NV12");
  VALI_REQUIRE(src->width >= 2 && src->height >= 2 && dst->width >= 2 && dst->height >= 2, "empty surface");
  VALI_REQUIRE(((src->width | src->height | dst->width | dst->height) & 1) == 0, "4:2:0 needs even sizes");
  VALI_REQUIRE(src->plane[0] && src->plane[1] && dst->plane[0], "null plane");
  VALI_REQUIRE(planes_fit_32bit(*src) && planes_fit_32bit(*dst), "plane of 4 GiB or more");
  if (dst->format == VALI_FMT_RGB_32F_PLANAR || dst->format == VALI_FMT_RGB_PLANAR)
    VALI_REQUIRE(dst->plane[1] && dst->plane[2], "null dst plane");
  VALI_REQUIRE(roi_axis_ok(roi->src_x, roi->src_w, src->width) && roi_axis_ok(roi->src_y, roi->src_h, src->height),
               "crop must be even, at least 2 x 2 and inside the source");
  VALI_REQUIRE(roi_axis_ok(roi->dst_x, roi->dst_w, dst->width) && roi_axis_ok(roi->dst_y, roi->dst_h, dst->height),
               "placement must be even, at least 2 x 2 and inside the destination");
  RoiArgs a = {};
  a.src = *src;
  a.dst = *dst;
  a.roi = *roi;
  a.prm = *params;
  a.pad = pad != 0;
  a.pad_rgb = pad_colour(pad, pad_rgb);
  hipStream_t s = as_stream(stream);
  VALI_ENTRY(s);
  return launch_preproc_roi(a, dst->width, dst->height, dst->format, 1, s);
}

int vali_nv12_preproc_roi_batch(const vali_surface* d_src, const vali_surface* d_dst, const vali_roi* d_roi, int n,
                                int dst_width, int dst_height, int dst_format, const vali_preproc_params* params,
                                int pad, const uint8_t pad_rgb[3], vali_stream_t stream) {
  VALI_REQUIRE(d_src && d_dst && d_roi && params, "null argument");
  VALI_REQUIRE(!pad || pad_rgb, "null pad colour");
  VALI_REQUIRE(dst_width >= 2 && dst_height >= 2 && ((dst_width | dst_height) & 1) == 0, "bad geometry");
  VALI_REQUIRE(n >= 0 && n <= 65535, "batch size out of range (0..65535)");
  if (n == 0)
    return VALI_OK;
  RoiArgs a = {};
  a.d_src = d_src;
  a.d_dst = d_dst;
  a.d_roi = d_roi;
  a.prm = *params;
  a.pad = pad != 0;
  a.pad_rgb = pad_colour(pad, pad_rgb);
  hipStream_t s = as_stream(stream);
  VALI_ENTRY(s);
  return launch_preproc_roi(a, dst_width, dst_height, dst_format, n, s);
}

static bool rgb_roi_axis_ok(int x, int w, int size) { return x >= 0 && w >= 1 && x <= size - w; }

int vali_rgb_preproc_roi(const vali_surface* src, const vali_surface* dst, const vali_roi* roi,
                         const vali_preproc_params* params, int pad, const uint8_t pad_rgb[3], vali_stream_t stream) {
  VALI_REQUIRE(src && dst && params, "null argument");
  VALI_REQUIRE(!pad || pad_rgb, "null pad colour");
  if (!rgb_src_ok(src->format))
    return fail(VALI_ERR_UNSUPPORTED, "rgb_preproc_roi: source must be RGB, BGR or RGB_PLANAR (got %d)", src->format);
  if (rgb_out_form(dst->format) < 0)
    return fail(VALI_ERR_UNSUPPORTED,
                "rgb_preproc_roi: destination must be RGB_32F[_PLANAR], RGB, BGR or RGB_PLANAR (got %d)", dst->format);
  VALI_REQUIRE(src->width >= 1 && src->height >= 1 && dst->width >= 1 && dst->height >= 1, "empty surface");
  VALI_REQUIRE(src->plane[0] && dst->plane[0], "null plane");
  if (src->format == VALI_FMT_RGB_PLANAR)
    VALI_REQUIRE(src->plane[1] && src->plane[2], "null src plane");
  if (dst->format == VALI_FMT_RGB_32F_PLANAR || dst->format == VALI_FMT_RGB_PLANAR)
    VALI_REQUIRE(dst->plane[1] && dst->plane[2], "null dst plane");
  VALI_REQUIRE(planes_fit_32bit(*src) && planes_fit_32bit(*dst), "plane of 4 GiB or more");
  const vali_roi whole = {0, 0, src->width, src->height, 0, 0, dst->width, dst->height};
  if (!roi)
    roi = &whole;
  VALI_REQUIRE(rgb_roi_axis_ok(roi->src_x, roi->src_w, src->width) && rgb_roi_axis_ok(roi->src_y, roi->src_h, src->height),
               "crop must be at least 1 x 1 and inside the source");
  VALI_REQUIRE(rgb_roi_axis_ok(roi->dst_x, roi->dst_w, dst->width) && rgb_roi_axis_ok(roi->dst_y, roi->dst_h, dst->height),
               "placement must be at least 1 x 1 and inside the destination");
  RgbRoiArgs ar = {};
  RoiArgs& a = ar.r;
  a.src = *src;
  a.dst = *dst;
  a.roi = *roi;
  a.prm = *params;
  a.pad = pad != 0;
  a.pad_rgb = pad_colour(pad, pad_rgb);
  hipStream_t s = as_stream(stream);
  VALI_ENTRY(s);
  return launch_rgb_preproc_roi(ar, src->format, dst->width, dst->height, dst->format, 1, s);
}

int vali_rgb_preproc_roi_batch(const vali_surface* d_src, const vali_surface* d_dst, const vali_roi* d_roi, int n,
                               int src_format, int dst_width, int dst_height, int dst_format,
                               const vali_preproc_params* params, int pad, const uint8_t pad_rgb[3],
                               vali_stream_t stream) {
  VALI_REQUIRE(d_src && d_dst && params, "null argument");
  VALI_REQUIRE(!pad || pad_rgb, "null pad colour");
  if (!rgb_src_ok(src_format))
    return fail(VALI_ERR_UNSUPPORTED, "rgb_preproc_roi_batch: sources must be RGB, BGR or RGB_PLANAR (got %d)", src_format);
  if (rgb_out_form(dst_format) < 0)
    return fail(VALI_ERR_UNSUPPORTED,
                "rgb_preproc_roi_batch: destination must be RGB_32F[_PLANAR], RGB, BGR or RGB_PLANAR (got %d)", dst_format);
  VALI_REQUIRE(dst_width >= 1 && dst_height >= 1, "bad geometry");
  VALI_REQUIRE(n >= 0 && n <= 65535, "batch size out of range (0..65535)");
  if (n == 0)
    return VALI_OK;
  RgbRoiArgs ar = {};
  RoiArgs& a = ar.r;
  a.d_src = d_src;
  a.d_dst = d_dst;
  a.d_roi = d_roi;
  ar.whole = d_roi == nullptr;
  a.prm = *params;
  a.pad = pad != 0;
  a.pad_rgb = pad_colour(pad, pad_rgb);
  hipStream_t s = as_stream(stream);
  VALI_ENTRY(s);
  return launch_rgb_preproc_roi(ar, src_format, dst_width, dst_height, dst_format, n, s);
}

static void tensor_dst_args(RoiArgs& a, const vali_surface* d_src, const vali_roi* d_roi, const vali_tensor_dst* dst,
                            const vali_preproc_params* params, int pad, const uint8_t* pad_rgb) {
  a.d_src = d_src;
  a.d_roi = d_roi;
  a.whole = d_roi == nullptr;
  a.tdst = *dst;
  a.prm = *params;
  a.pad = pad != 0;
  a.pad_rgb = pad_colour(pad, pad_rgb);
}

int vali_nv12_preproc_roi_tensor(const vali_surface* d_src, const vali_roi* d_roi, const vali_tensor_dst* dst,
                                 const vali_preproc_params* params, int pad, const uint8_t pad_rgb[3],
                                 vali_stream_t stream) {
  VALI_REQUIRE(d_src && dst && params, "null argument");
  VALI_REQUIRE(!pad || pad_rgb, "null pad colour");
  if (const int rc = check_tensor_dst(__func__, dst, true))
    return rc;
  RoiArgs a = {};
  tensor_dst_args(a, d_src, d_roi, dst, params, pad, pad_rgb);
  hipStream_t s = as_stream(stream);
  VALI_ENTRY(s);
  return launch_preproc_roi(a, dst->width, dst->height, dst->packed ? VALI_FMT_RGB_32F : VALI_FMT_RGB_32F_PLANAR, dst->n,
                            s, TD_F32 + dst->dtype);
}

int vali_rgb_preproc_roi_tensor(const vali_surface* d_src, const vali_roi* d_roi, int src_format,
                                const vali_tensor_dst* dst, const vali_preproc_params* params, int pad,
                                const uint8_t pad_rgb[3], vali_stream_t stream) {
  VALI_REQUIRE(d_src && dst && params, "null argument");
  VALI_REQUIRE(!pad || pad_rgb, "null pad colour");
  if (!rgb_src_ok(src_format))
    return fail(VALI_ERR_UNSUPPORTED, "rgb_preproc_roi_tensor: sources must be RGB, BGR or RGB_PLANAR (got %d)", src_format);
  if (const int rc = check_tensor_dst(__func__, dst, false))
    return rc;
  RgbRoiArgs ar = {};
  tensor_dst_args(ar.r, d_src, d_roi, dst, params, pad, pad_rgb);
  ar.whole = d_roi == nullptr;
  hipStream_t s = as_stream(stream);
  VALI_ENTRY(s);
  return launch_rgb_preproc_roi(ar, src_format, dst->width, dst->height,
                                dst->packed ? VALI_FMT_RGB_32F : VALI_FMT_RGB_32F_PLANAR, dst->n, s, TD_F32 + dst->dtype);
}

} // extern "C"
