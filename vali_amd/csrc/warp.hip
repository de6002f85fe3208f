// Aligned and rotated crops (vali_warp_fit, vali_warp_tensor): every slot of an (M, 3, h, w) batch tensor is one affine
// view of one frame of a batch of NV12, RGB, BGR or RGB_PLANAR frames, sampled bilinearly with edge replication,
// normalised and converted to the tensor's element type in ONE launch; the six coefficients of a slot come from a row of
// a DEVICE array, which the caller fills (rotated boxes, anything computed on the GPU) or vali_warp_fit does: the
// least-squares similarity that takes a template onto the visible keypoints of a detection (a face onto the ArcFace
// canvas), from the rows of vali_detect_select and a pose head, in one more launch.
//
// Definition: include/vali_hip.h ("aligned crops"); tests/warp_model.py restates it in numpy.
//
//   k_warp_fit<DT>              one lane per dets row: two passes over the row's keypoints in ascending order (the sums,
//                               then the centred products), so the summation order is the definition's.  The mapping and
//                               the visibility rule are kpt_map.hpp's, the rows det_rows.hpp's.
//   k_warp_sample<SRC, DT, CL>  a 1-D grid over slots x canvas tiles of 16 lanes x 16 rows.  A lane owns the consecutive
//                               pixels of one row that make a 16-byte store of the planar layout (8 of a 16-bit type, 4 of
//                               float32).  The slot's row and the frame's descriptor are workgroup-uniform: scalar loads;
//                               a skipped slot returns, or stores pad, without touching a frame.  Every pixel's position
//                               is evaluated from its own (x, y) as the definition writes it.  The taps are a gather through
//                               the vector cache and L2: neighbouring lanes read neighbouring texels; nothing is staged
//                               in LDS but the 3 x 256 table of step 5, filled once per workgroup as k_nv12_preproc_roi
//                               fills its own, so the per-pixel path moves finished elements.
// The float16 / bfloat16 conversions, step 5 (normalise_u8), the scalar loads and the checks of the tensor are
// tensor_out.hpp's, shared with preproc.hip; the check of the keypoint head is tensor_in.hpp's.
#include <math.h>

#include "det_rows.hpp"
#include "kpt_map.hpp"
#include "tensor_in.hpp"
#include "tensor_out.hpp"

#pragma clang fp contract(off)

namespace vali {
namespace {

constexpr int kMaxN = 1024, kMaxK = 1 << 20, kMaxD = 1024, kMaxP = 64, kMaxM = 65535;
constexpr int kLanesX = 16, kTileRows = kBlock / kLanesX;

// ---- the fit ---------------------------------------------------------------------------------------------------------------
struct FitArgs {
  const vali_surface* d_frames;
  const int32_t* dets;
  const vali_roi* rects;
  const float* tmpl;  // P pairs (u, v)
  const void* kpts;
  int4* mats;  // n * D rows of two int4
  long long sn, sk, sp, sc;
  int kdim;
  int n, D, K, P, min_points;
  float thr;
};

template <int DT>
__global__ void __launch_bounds__(kBlock) k_warp_fit(const FitArgs a) {
  typedef TensorElem<DT> E;
  typedef typename E::Bits Bits;
  const int row = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (row >= a.n * a.D)
    return;
  const int f = row / a.D;
  int4* out = a.mats + 2 * (size_t)row;
  const int4 skip0 = make_int4(-1, 0, 0, 0), skip1 = make_int4(0, 0, 0, 0);
  int r[8];
  load_row(a.dets, row, r);
  const int W = a.d_frames[f].width, H = a.d_frames[f].height;
  const vali_roi rc = a.rects[f];
  Row o;
  if (!resolve_row(r, f, W, H, a.K, rc, o)) {
    out[0] = skip0, out[1] = skip1;
    return;
  }
  const Bits* base = (const Bits*)a.kpts + (long long)f * a.sn + (long long)o.k * a.sk;
  // keypoint j in frame pixels, and whether it takes part
  const auto point = [&](int j, float& u, float& v, float& fx, float& fy) -> bool {
    const Bits* p = base + (long long)j * a.sp;
    const float kx = E::f((u32)p[0]), ky = E::f((u32)p[a.sc]);
    const float conf = a.kdim == 3 ? E::f((u32)p[2 * a.sc]) : 1.0f;
    u = a.tmpl[2 * j], v = a.tmpl[2 * j + 1];
    fx = map_axis(kx, rc.dst_x, rc.src_w, rc.dst_w, rc.src_x);
    fy = map_axis(ky, rc.dst_y, rc.src_h, rc.dst_h, rc.src_y);
    return kpt_visible(conf, a.thr, kx, ky, fx, fy) && u == u && v == v;
  };
  int n = 0;
  float su = 0.0f, sv = 0.0f, sx = 0.0f, sy = 0.0f;
  for (int j = 0; j < a.P; ++j) {
    float u, v, fx, fy;
    if (point(j, u, v, fx, fy)) {
      ++n;
      su = __fadd_rn(su, u), sv = __fadd_rn(sv, v), sx = __fadd_rn(sx, fx), sy = __fadd_rn(sy, fy);
    }
  }
  if (n < a.min_points) {
    out[0] = skip0, out[1] = skip1;
    return;
  }
  const float fn = (float)n;
  const float mu = __fdiv_rn(su, fn), mv = __fdiv_rn(sv, fn), mx = __fdiv_rn(sx, fn), my = __fdiv_rn(sy, fn);
  float A = 0.0f, B = 0.0f, Dn = 0.0f;
  for (int j = 0; j < a.P; ++j) {
    float u, v, fx, fy;
    if (point(j, u, v, fx, fy)) {
      const float du = __fsub_rn(u, mu), dv = __fsub_rn(v, mv), dx = __fsub_rn(fx, mx), dy = __fsub_rn(fy, my);
      A = __fadd_rn(A, __fadd_rn(__fmul_rn(du, dx), __fmul_rn(dv, dy)));
      B = __fadd_rn(B, __fsub_rn(__fmul_rn(du, dy), __fmul_rn(dv, dx)));
      Dn = __fadd_rn(Dn, __fadd_rn(__fmul_rn(du, du), __fmul_rn(dv, dv)));
    }
  }
  const float al = __fdiv_rn(A, Dn), be = __fdiv_rn(B, Dn);
  if (Dn == 0.0f || !(fabsf(al) < INFINITY) || !(fabsf(be) < INFINITY)) {
    out[0] = skip0, out[1] = skip1;
    return;
  }
  const float c = __fsub_rn(mx, __fsub_rn(__fmul_rn(al, mu), __fmul_rn(be, mv)));
  const float ff = __fsub_rn(my, __fadd_rn(__fmul_rn(be, mu), __fmul_rn(al, mv)));
  out[0] = make_int4(f, __float_as_int(al), __float_as_int(-be), __float_as_int(c));
  out[1] = make_int4(__float_as_int(be), __float_as_int(al), __float_as_int(ff), n);
}

// ---- the sampler -----------------------------------------------------------------------------------------------------------
enum : int { SRC_NV12 = 0, SRC_PACKED = 1, SRC_PLANAR = 2 };

struct MatRow {
  int32_t frame;
  float a, b, c, d, e, f;
  int32_t status;
};
static_assert(sizeof(MatRow) == 32, "a row of matrices");

struct WarpArgs {
  const vali_surface* d_frames;
  const MatRow* mats;
  vali_tensor_dst t;
  vali_preproc_params prm;
  int n;               // frames
  u32 tiles_x, tiles;  // of one slot
  int pad;             // 0: pixels that sample nothing are not written
  u32 pad_rgb;         // R | G << 8 | B << 16
  int bgr;             // SRC_PACKED: the first stored colour is blue
};

// an element of the tensor as its bits, and the table's entry
template <int DT> struct WElem {
  typedef u32 lut_t;
  static constexpr int ES = 4;
  static __device__ __forceinline__ u32 make(float v) { return __float_as_uint(v); }
};
template <> struct WElem<VALI_DTYPE_F16> {
  typedef uint16_t lut_t;
  static constexpr int ES = 2;
  static __device__ __forceinline__ u32 make(float v) { return f32_to_f16_bits(v); }
};
template <> struct WElem<VALI_DTYPE_BF16> {
  typedef uint16_t lut_t;
  static constexpr int ES = 2;
  static __device__ __forceinline__ u32 make(float v) { return f32_to_bf16_bits(v); }
};

// step 3 along one axis for a position s inside [0, n): g in [-0.5, n - 0.5), so floor(g) is -1 .. n - 1
struct WTap {
  int i0, i1;
  float t;
};
__device__ __forceinline__ WTap warp_tap(float s, int n) {
  const float g = __fsub_rn(s, 0.5f);
  const float fl = floorf(g);
  WTap k;
  k.t = __fsub_rn(g, fl);
  const int i = (int)fl;
  k.i0 = min(max(i, 0), n - 1), k.i1 = min(max(i + 1, 0), n - 1);
  return k;
}
__device__ __forceinline__ float warp_lerp(float p00, float p01, float p10, float p11, float tx, float ty) {
  const float top = __fadd_rn(p00, __fmul_rn(tx, __fsub_rn(p01, p00)));
  const float bot = __fadd_rn(p10, __fmul_rn(tx, __fsub_rn(p11, p10)));
  return __fadd_rn(top, __fmul_rn(ty, __fsub_rn(bot, top)));
}
__device__ __forceinline__ float ldb(const uint8_t* p) { return (float)gload<uint8_t>(p); }

// q_R | q_G << 8 | q_B << 16 of the pixel that samples (sx, sy), a position inside the frame (steps 3 and 4)
template <int SRC>
__device__ __forceinline__ u32 warp_pixel(const vali_surface& s, float sx, float sy, const vali_csc& k, int bgr) {
  const WTap tx = warp_tap(sx, s.width), ty = warp_tap(sy, s.height);
  if constexpr (SRC == SRC_NV12) {
    const uint8_t* r0 = (const uint8_t*)s.plane[0] + (size_t)ty.i0 * (size_t)s.pitch[0];
    const uint8_t* r1 = (const uint8_t*)s.plane[0] + (size_t)ty.i1 * (size_t)s.pitch[0];
    const float y = warp_lerp(ldb(r0 + tx.i0), ldb(r0 + tx.i1), ldb(r1 + tx.i0), ldb(r1 + tx.i1), tx.t, ty.t);
    // chroma: centre-sited samples of the (W / 2) x (H / 2) plane; a pair (U, V) is one 16-bit load
    const WTap cx = warp_tap(__fmul_rn(sx, 0.5f), s.width >> 1), cy = warp_tap(__fmul_rn(sy, 0.5f), s.height >> 1);
    const uint8_t* c0 = (const uint8_t*)s.plane[1] + (size_t)cy.i0 * (size_t)s.pitch[1];
    const uint8_t* c1 = (const uint8_t*)s.plane[1] + (size_t)cy.i1 * (size_t)s.pitch[1];
    const u32 w00 = gload<uint16_t>(c0 + 2 * cx.i0), w01 = gload<uint16_t>(c0 + 2 * cx.i1);
    const u32 w10 = gload<uint16_t>(c1 + 2 * cx.i0), w11 = gload<uint16_t>(c1 + 2 * cx.i1);
    const float u = warp_lerp((float)(w00 & 255u), (float)(w01 & 255u), (float)(w10 & 255u), (float)(w11 & 255u), cx.t, cy.t);
    const float v = warp_lerp((float)(w00 >> 8), (float)(w01 >> 8), (float)(w10 >> 8), (float)(w11 >> 8), cx.t, cy.t);
    // the u8 pixel (q_Y, q_U, q_V) through vali_convert's YUV444 -> RGB
    const float qy = (float)quantize_u8(y), qu = (float)quantize_u8(u), qv = (float)quantize_u8(v);
    const ChromaTerm ct = chroma_term(qu, qv, k);
    const float yf = luma_term(qy, k);
    return quantize_u8(yf + ct.rv) | quantize_u8(yf + ct.guv) << 8 | quantize_u8(yf + ct.bu) << 16;
  } else if constexpr (SRC == SRC_PACKED) {
    const uint8_t* r0 = (const uint8_t*)s.plane[0] + (size_t)ty.i0 * (size_t)s.pitch[0];
    const uint8_t* r1 = (const uint8_t*)s.plane[0] + (size_t)ty.i1 * (size_t)s.pitch[0];
    const int o0 = 3 * tx.i0, o1 = 3 * tx.i1;
    u32 q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
      q[c] = quantize_u8(warp_lerp(ldb(r0 + o0 + c), ldb(r0 + o1 + c), ldb(r1 + o0 + c), ldb(r1 + o1 + c), tx.t, ty.t));
    return (bgr ? q[2] : q[0]) | q[1] << 8 | (bgr ? q[0] : q[2]) << 16;
  } else {
    u32 q = 0u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint8_t* r0 = (const uint8_t*)s.plane[c] + (size_t)ty.i0 * (size_t)s.pitch[c];
      const uint8_t* r1 = (const uint8_t*)s.plane[c] + (size_t)ty.i1 * (size_t)s.pitch[c];
      q |= quantize_u8(warp_lerp(ldb(r0 + tx.i0), ldb(r0 + tx.i1), ldb(r1 + tx.i0), ldb(r1 + tx.i1), tx.t, ty.t)) << (8 * c);
    }
    return q;
  }
}

// CL: channels last
template <int SRC, int DT, bool CL>
__global__ void __launch_bounds__(kBlock) k_warp_sample(const WarpArgs a) {
  typedef WElem<DT> Elem;
  constexpr int ES = Elem::ES, PX = 16 / ES;
  __shared__ typename Elem::lut_t lut[3][256];

  const u32 slot = blockIdx.x / a.tiles, tile = blockIdx.x - slot * a.tiles;
  if (slot >= (u32)a.t.n)
    return;
  const u32 tile_y = tile / a.tiles_x, tile_x = tile - tile_y * a.tiles_x;
  const MatRow m = load_uniform(a.mats, slot);
  const bool skipped = m.frame < 0 || m.frame >= a.n;  // step 1
  if (skipped && !a.pad)
    return;
  vali_surface s = {};
  if (!skipped) {
    s = load_uniform(a.d_frames, (u32)m.frame);
    for (int e = threadIdx.x; e < 3 * 256; e += kBlock)
      lut[e >> 8][e & 255] = (typename Elem::lut_t)Elem::make(normalise_u8(e & 255, e >> 8, a.prm));
    __syncthreads();
  }
  const int w = a.t.width, h = a.t.height;
  const int x0 = (int)(tile_x * kLanesX + (threadIdx.x & (kLanesX - 1))) * PX;
  const int y = (int)(tile_y * kTileRows + threadIdx.x / kLanesX);
  if (x0 >= w || y >= h)
    return;
  u32 pv[3];  // the pad colour through step 5
#pragma unroll
  for (int c = 0; c < 3; ++c)
    pv[c] = (u32)__builtin_amdgcn_readfirstlane((int)Elem::make(normalise_u8((a.pad_rgb >> (8 * c)) & 255u, c, a.prm)));

  // step 2 for each of the lane's pixels, from its own (x, y)
  const float v = __fadd_rn((float)y, 0.5f);
  const float bv = __fmul_rn(m.b, v), ev = __fmul_rn(m.e, v);
  const float fw = (float)s.width, fh = (float)s.height;
  u32 o[3][PX];
  u32 wr = 0u;  // the pixels that are written
#pragma unroll
  for (int p = 0; p < PX; ++p) {
    const float u = __fadd_rn((float)(x0 + p), 0.5f);
    const float sx = __fadd_rn(__fadd_rn(__fmul_rn(m.a, u), bv), m.c);
    const float sy = __fadd_rn(__fadd_rn(__fmul_rn(m.d, u), ev), m.f);
    const bool inside = !skipped && x0 + p < w && sx >= 0.0f && sx < fw && sy >= 0.0f && sy < fh;  // a NaN never is
    o[0][p] = pv[0], o[1][p] = pv[1], o[2][p] = pv[2];
    if (inside) {
      const u32 q = warp_pixel<SRC>(s, sx, sy, a.prm.csc, a.bgr);
      o[0][p] = lut[0][q & 255u], o[1][p] = lut[1][(q >> 8) & 255u], o[2][p] = lut[2][q >> 16];
    }
    if (x0 + p < w && (inside || a.pad))
      wr |= 1u << p;
  }
  if (wr == 0u)
    return;

  // the lane's elements: whole 16-byte pieces when it writes all of its pixels to an aligned address, single elements
  // otherwise (a ragged right edge, pad = none, a view whose rows start off the 16-byte grid)
  typedef typename std::conditional<ES == 4, u32, uint16_t>::type elem_t;
  const bool full = wr == (1u << PX) - 1u;
  uint8_t* item = (uint8_t*)a.t.data + ((long long)slot * a.t.stride_n + (long long)y * a.t.stride_y) * ES;
  if constexpr (!CL) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      uint8_t* q = item + ((long long)c * a.t.stride_c + x0) * ES;
      if (full && (((uintptr_t)q) & 15u) == 0) {
        v4u32 pk;
        if constexpr (ES == 4)
          pk = v4u32{o[c][0], o[c][1], o[c][2], o[c][3]};
        else
          pk = v4u32{o[c][0] | o[c][1] << 16, o[c][2] | o[c][3] << 16, o[c][4] | o[c][5] << 16, o[c][6] | o[c][7] << 16};
        gstore<v4u32>(q, pk);
      } else {
#pragma unroll
        for (int p = 0; p < PX; ++p)
          if (wr & (1u << p))
            gstore<elem_t>(q + p * ES, (elem_t)o[c][p]);
      }
    }
  } else {
    uint8_t* q = item + (long long)(3 * x0) * ES;
    if (full && (((uintptr_t)q) & 15u) == 0) {
      // 3 PX elements in memory order: element e is channel e % 3 of pixel e / 3
      u32 d[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) {
        if constexpr (ES == 4)
          d[k] = o[k % 3][k / 3];
        else
          d[k] = o[(2 * k) % 3][(2 * k) / 3] | o[(2 * k + 1) % 3][(2 * k + 1) / 3] << 16;
      }
#pragma unroll
      for (int k = 0; k < 3; ++k)
        gstore<v4u32>(q + 16 * k, v4u32{d[4 * k], d[4 * k + 1], d[4 * k + 2], d[4 * k + 3]});
    } else {
#pragma unroll
      for (int p = 0; p < PX; ++p)
        if (wr & (1u << p)) {
#pragma unroll
          for (int c = 0; c < 3; ++c)
            gstore<elem_t>(q + (3 * p + c) * ES, (elem_t)o[c][p]);
        }
    }
  }
}

template <int SRC, int DT>
void launch_sample(const dim3& grid, hipStream_t s, const WarpArgs& a) {
  if (a.t.packed)
    hipLaunchKernelGGL((k_warp_sample<SRC, DT, true>), grid, dim3(kBlock), 0, s, a);
  else
    hipLaunchKernelGGL((k_warp_sample<SRC, DT, false>), grid, dim3(kBlock), 0, s, a);
}
template <int SRC>
void launch_sample_dt(const dim3& grid, hipStream_t s, const WarpArgs& a) {
  with_float_dtype(a.t.dtype, [&](auto dt) { launch_sample<SRC, dt>(grid, s, a); });
}

} // namespace
} // namespace vali

using namespace vali;

extern "C" {

int vali_warp_fit(const vali_surface* d_frames, int n, const vali_warp_fit_in* in, const int32_t* d_dets,
                  const vali_roi* d_rects, int32_t* d_matrices, vali_stream_t stream) {
  VALI_REQUIRE(d_frames && in && d_dets && d_rects && d_matrices, "null argument");
  VALI_REQUIRE(n >= 1 && n <= kMaxN, "n outside 1..1024");
  VALI_REQUIRE(in->k >= 1 && in->k <= kMaxK, "k outside 1..2^20");
  VALI_REQUIRE(in->p >= 2 && in->p <= kMaxP, "p outside 2..64");
  VALI_REQUIRE(in->kdim == 2 || in->kdim == 3, "kdim is neither 2 nor 3");
  VALI_REQUIRE(in->max_det >= 1 && in->max_det <= kMaxD, "max_det outside 1..1024");
  VALI_REQUIRE((long long)n * in->max_det <= kMaxM, "n * max_det exceeds 65535");
  VALI_REQUIRE(in->min_points >= 2 && in->min_points <= in->p, "min_points outside 2..p");
  VALI_REQUIRE(in->kpts, "kpts has a null pointer");
  VALI_REQUIRE(in->d_template, "template has a null pointer");  // between the null kpts above and the rest of its rule
  const int64_t strides[4] = {in->stride_n, in->stride_k, in->stride_p, in->stride_c};
  if (const int rc = check_head_tensor(__func__, "kpts", in->kpts, in->dtype, strides, 4))
    return rc;
  VALI_REQUIRE(in->kpt_thr == in->kpt_thr, "kpt_thr is a NaN");
  VALI_REQUIRE((((uintptr_t)d_dets | (uintptr_t)d_rects | (uintptr_t)in->d_template | (uintptr_t)d_frames) & 3u) == 0,
               "frames, dets, rects or template are not 4-byte aligned");
  VALI_REQUIRE(((uintptr_t)d_matrices & 15u) == 0, "matrices is not 16-byte aligned");

  FitArgs a = {};
  a.d_frames = d_frames, a.dets = d_dets, a.rects = d_rects, a.tmpl = in->d_template, a.kpts = in->kpts;
  a.mats = (int4*)d_matrices;
  a.sn = in->stride_n, a.sk = in->stride_k, a.sp = in->stride_p, a.sc = in->stride_c;
  a.kdim = in->kdim;
  a.n = n, a.D = in->max_det, a.K = in->k, a.P = in->p, a.min_points = in->min_points;
  a.thr = in->kpt_thr;

  hipStream_t s = as_stream(stream);
  VALI_ENTRY(s);
  const dim3 grid((unsigned)((n * in->max_det + kBlock - 1) / kBlock));
  with_float_dtype(in->dtype, [&](auto dt) { hipLaunchKernelGGL(k_warp_fit<dt>, grid, dim3(kBlock), 0, s, a); });
  VALI_LAUNCH_CHECK();
  return VALI_OK;
}

int vali_warp_tensor(const vali_surface* frames, const vali_surface* d_frames, int n, int format,
                     const int32_t* d_matrices, const vali_tensor_dst* dst, const vali_preproc_params* params, int pad,
                     const uint8_t pad_rgb[3], vali_stream_t stream) {
  VALI_REQUIRE(frames && d_frames && d_matrices && dst && params, "null argument");
  VALI_REQUIRE(!pad || pad_rgb, "null pad colour");
  VALI_REQUIRE(n >= 1 && n <= kMaxN, "n outside 1..1024");
  if (format != VALI_FMT_NV12 && format != VALI_FMT_RGB && format != VALI_FMT_BGR && format != VALI_FMT_RGB_PLANAR)
    return fail(VALI_ERR_UNSUPPORTED, "%s: format %d (NV12, RGB, BGR, RGB_PLANAR)", __func__, format);
  int unused = 0;
  if (const int rc = check_frames(__func__, n, frames, format, &unused))
    return rc;
  if (const int rc = check_tensor_dst(__func__, dst, false))
    return rc;
  VALI_REQUIRE((((uintptr_t)d_matrices | (uintptr_t)d_frames) & 3u) == 0, "frames or matrices are not 4-byte aligned");
  const int px = dst->dtype == VALI_DTYPE_F32 ? 4 : 2 * 4;
  const uint64_t tiles_x = ((uint64_t)dst->width + (uint64_t)(kLanesX * px) - 1) / (uint64_t)(kLanesX * px);
  const uint64_t tiles_y = ((uint64_t)dst->height + kTileRows - 1) / kTileRows;
  VALI_REQUIRE(tiles_x * tiles_y * (uint64_t)dst->n <= 0x7fffffffull, "more than 2^31 - 1 tiles: the canvas is too large");

  WarpArgs a = {};
  a.d_frames = d_frames, a.mats = (const MatRow*)d_matrices;
  a.t = *dst, a.prm = *params;
  a.n = n;
  a.tiles_x = (u32)tiles_x, a.tiles = (u32)(tiles_x * tiles_y);
  a.pad = pad != 0;
  a.pad_rgb = pad_colour(pad, pad_rgb);
  a.bgr = format == VALI_FMT_BGR;

  hipStream_t s = as_stream(stream);
  VALI_ENTRY(s);
  const dim3 grid((unsigned)(tiles_x * tiles_y * (uint64_t)dst->n));
  switch (format) {
  case VALI_FMT_NV12: launch_sample_dt<SRC_NV12>(grid, s, a); break;
  case VALI_FMT_RGB_PLANAR: launch_sample_dt<SRC_PLANAR>(grid, s, a); break;
  default: launch_sample_dt<SRC_PACKED>(grid, s, a); break;
  }
  VALI_LAUNCH_CHECK();
  return VALI_OK;
}

} // extern "C"
