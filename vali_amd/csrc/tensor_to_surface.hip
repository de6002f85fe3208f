// One (N, 3, H, W) batch tensor -> N 8-bit surfaces (vali_tensor_to_surfaces): the way back from a network's output to
// video frames, the mirror image of the fused NV12 -> tensor pre-processor.  Replaces the chain
//   torch quantise (7 elementwise launches) -> permute/contiguous -> N x from_dlpack(RGB) -> N x RGB->YUV420 -> N x YUV420->NV12
// with one launch that reads every element once and writes every destination byte once.
//
// Definition (include/vali_hip.h): p = the quantiser of vali_jpeg_encode_tensor (tensor_in.hpp: the same code), then
//   RGB / RGB_PLANAR   the bytes
//   YUV444             c = fma(kB, B, fma(kG, G, fma(kR, R, offset))), round-half-even + saturate   (cvt_generic.hip)
//   YUV420 / NV12      Y likewise; chroma = ((c00 + c01) + (c10 + c11)) * 0.25 over the un-rounded values
// so a YUV destination holds byte for byte what vali_convert writes for an RGB surface that holds p.
//
// Work decomposition = k_cvt8's (cvt_generic.hip): a lane owns 16 pixels x 2 rows (the 2 x 2 chroma footprint), narrow
// frames stack row pairs in a workgroup; the grid is (strips, row pairs, N).
//   loads   16-byte loads when the lane's six row pieces are 16-byte aligned (dwords for uint8), both rows' issued before
//           either is used (16 and 8 bit elements); per-element loads (TensorIn::pixels4, clamped, four pixels a turn in
//           a rolled loop) for the group the right edge cuts and for rows that do not start on 16 bytes
//           (big[:, :, 1:1+H, 1:1+W])
//   stores  whole pieces per lane and line: 16 B of Y, 16 B of UV (NV12), 8 B of U and of V (YUV420), packed RGB through
//           the per-wave LDS strip as 3 x 1 KiB -- non-temporal when the width is a multiple of 16 and every plane and
//           pitch is aligned (a line piece then leaves in ONE instruction); otherwise the misaligned / byte forms of the
//           same stores, the cut group slid left to end with the row (k_cvt8's ragged path)
#include <cmath>

#include "common.hpp"
#include "dev_util.hpp"
#include "tensor_in.hpp"

namespace vali {
namespace {

enum T2sDst : int { D_NV12 = 0, D_YUV420 = 1, D_YUV444 = 2, D_RGB = 3, D_RGBP = 4 };

constexpr bool d_is420(int d) { return d == D_NV12 || d == D_YUV420; }
constexpr bool d_isyuv(int d) { return d == D_NV12 || d == D_YUV420 || d == D_YUV444; }

struct T2sArgs {
  TensorArgs in;              // the tensor, scale, offset; swap_rb: tensor channel 0 is blue
  const vali_surface* d_dst;  // device array of in.t.n descriptors
  float m[3][4];              // rgb2yuv rows (YUV destinations)
  int rp;                     // row pairs stacked in one workgroup
};

// cvt_generic.hip's dot_rgb
__device__ __forceinline__ float dot_rgb(const float (&m)[4], float r, float g, float b) {
  return __builtin_fmaf(m[2], b, __builtin_fmaf(m[1], g, __builtin_fmaf(m[0], r, m[3])));
}

// One row of a lane's 16 pixels as it was loaded.  VEC (the lane's pieces are whole and aligned): the elements' bits, planar
// as the planes that feed R, G, B in w[0 .. 4 ES), [4 ES .. 8 ES), [8 ES .. 12 ES), channels last as the 48 elements in
// memory order; quantised four pixels at a time when they are needed, which keeps a row's live state at its raw bits.
// !VEC (the group the right edge cuts, rows off the vector alignment): the quantised pixels as bytes,
// R in w[0 .. 4), G in w[4 .. 8), B in w[8 .. 12).
template <int DT, bool PACKED, bool VEC>
struct RowRaw {
  typedef TensorIn<DT, PACKED, false> In;
  typedef typename In::E E;
  static constexpr int ES = In::ES;
  u32 w[VEC ? 12 * ES : 12];

  __device__ __forceinline__ void load(const TensorArgs& a, typename In::Item base, int y, int xs, int W) {
    if constexpr (!VEC) {
      // A ROLLED loop, four pixels a turn: 12 element loads in flight and registers for no more.  Unrolled, the 48
      // element loads of a row with their 64-bit addresses set the register count of the whole kernel (130 to 170,
      // 3 waves per SIMD) and the vector path, which needs 60 to 80, paid for it.
      u32 t[3][4] = {};  // tensor channel k, quantised, 4 pixels per dword
#pragma unroll 1
      for (int q = 0; q < 4; ++q) {
        float e[3][4];
        In::pixels4(a, base, y, xs + 4 * q, W, e);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          u32 d = 0;
#define VALI_PX(I) d = pack_u8<I>(quantise_elem_f(e[k][I], a.scale[k], a.offset[k]), d);
          VALI_PX(0) VALI_PX(1) VALI_PX(2) VALI_PX(3)
#undef VALI_PX
          // the finished dwords move down one place and the new one comes in at the top: no run-time index
          t[k][0] = t[k][1], t[k][1] = t[k][2], t[k][2] = t[k][3], t[k][3] = d;
        }
      }
      const bool swap = a.swap_rb != 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        w[j] = swap ? t[2][j] : t[0][j];
        w[4 + j] = t[1][j];
        w[8 + j] = swap ? t[0][j] : t[2][j];
      }
    } else if constexpr (PACKED) {
      load_elems<ES, 48>(base + (size_t)y * (size_t)a.t.stride_y + 3 * xs, w);
    } else {
      // the channel order decides which plane feeds R and B, not what is computed (TensorIn::rgb_row)
      const int cr = a.swap_rb ? 2 : 0;
      const typename In::Bits* row = base + (size_t)y * (size_t)a.t.stride_y + xs;
      load_elems<ES, 16>(row + (size_t)cr * (size_t)a.t.stride_c, w);
      load_elems<ES, 16>(row + (size_t)a.t.stride_c, w + 4 * ES);
      load_elems<ES, 16>(row + (size_t)(2 - cr) * (size_t)a.t.stride_c, w + 8 * ES);
    }
  }

  // pixels 4 j .. 4 j + 3, quantised (0 .. 255 as floats), colours by name
  __device__ __forceinline__ void px4(const TensorArgs& a, int j, float (&R)[4], float (&G)[4], float (&B)[4]) const {
    const bool swap = a.swap_rb != 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (!VEC) {
        R[i] = (float)((w[j] >> (8 * i)) & 0xffu);
        G[i] = (float)((w[4 + j] >> (8 * i)) & 0xffu);
        B[i] = (float)((w[8 + j] >> (8 * i)) & 0xffu);
      } else if constexpr (PACKED) {
        const int k = 3 * (4 * j + i);
        const float p0 = quantise_elem_f(E::f(elem_bits<ES>(w, k)), a.scale[0], a.offset[0]);
        const float p2 = quantise_elem_f(E::f(elem_bits<ES>(w, k + 2)), a.scale[2], a.offset[2]);
        G[i] = quantise_elem_f(E::f(elem_bits<ES>(w, k + 1)), a.scale[1], a.offset[1]);
        R[i] = swap ? p2 : p0;
        B[i] = swap ? p0 : p2;
      } else {
        const float sr = swap ? a.scale[2] : a.scale[0], orr = swap ? a.offset[2] : a.offset[0];
        const float sb = swap ? a.scale[0] : a.scale[2], ob = swap ? a.offset[0] : a.offset[2];
        R[i] = quantise_elem_f(E::f(elem_bits<ES>(w, 4 * j + i)), sr, orr);
        G[i] = quantise_elem_f(E::f(elem_bits<ES>(w + 4 * ES, 4 * j + i)), a.scale[1], a.offset[1]);
        B[i] = quantise_elem_f(E::f(elem_bits<ES>(w + 8 * ES, 4 * j + i)), sb, ob);
      }
    }
  }
};

// can the lane take the vector loads: 16 whole pixels, and every piece of both rows on the vector path's alignment
template <int DT, bool PACKED>
__device__ __forceinline__ bool rows_vectorisable(const TensorArgs& a, typename TensorIn<DT, PACKED, false>::Item base,
                                                  int y0, int y1, int xs, int W) {
  typedef TensorIn<DT, PACKED, false> In;
  if (xs + 16 > W)
    return false;
  const size_t sy = (size_t)a.t.stride_y, sc = (size_t)a.t.stride_c;
  uintptr_t bits;
  if (PACKED) {
    bits = (uintptr_t)(base + (size_t)y0 * sy + 3 * xs) | (uintptr_t)(base + (size_t)y1 * sy + 3 * xs);
  } else {
    const uintptr_t p0 = (uintptr_t)(base + (size_t)y0 * sy + xs), p1 = (uintptr_t)(base + (size_t)y1 * sy + xs);
    const uintptr_t c1 = (uintptr_t)(sc * In::ES);
    bits = p0 | p1 | (p0 + c1) | (p0 + 2 * c1) | (p1 + c1) | (p1 + 2 * c1);
  }
  return (bits & In::kAlign) == 0;
}

typedef v2u32 v2u32_any __attribute__((aligned(1)));

// one 16-byte piece of a plane row: FAST = aligned and whole (non-temporal); otherwise any address, n valid bytes
template <bool FAST>
__device__ __forceinline__ void put16(uint8_t* p, const u32 (&w)[4], int n) {
  const uint4 v = make_uint4(w[0], w[1], w[2], w[3]);
  if constexpr (FAST)
    store16_nt(p, v);
  else
    store16_n(p, v, n);
}
template <bool FAST>
__device__ __forceinline__ void put8(uint8_t* p, u32 lo, u32 hi, int n) {
  if constexpr (FAST) {
    store8_nt(p, make_uint2(lo, hi));
  } else if (n >= 8) {
    const v2u32 w = {lo, hi};
    *(v2u32_any*)p = w;
  } else {
    store_bytes16(p, make_uint4(lo, hi, 0u, 0u), n);
  }
}

// The lane's 16 x 2 pixels: load, quantise, convert; the finished bytes in c0 / c1 / c2 (Y, U, V or R, G, B) and cu / cv
template <int DT, bool PACKED, int DST, bool VEC>
__device__ __forceinline__ void t2s_block(const T2sArgs& a, typename TensorIn<DT, PACKED, false>::Item base, int row0,
                                          int row1, int xs, u32 (&c0)[2][4], u32 (&c1)[2][4], u32 (&c2)[2][4],
                                          u32 (&cu)[2], u32 (&cv)[2]) {
  typedef RowRaw<DT, PACKED, VEC> Row;
  const int W = a.in.t.width;
  // both rows' loads are issued before either row is used where their bits fit the registers (16 and 8 bit elements)
  constexpr bool kBoth = VEC && Row::ES <= 2;
  Row raw[2];
  if constexpr (kBoth) {
    raw[0].load(a.in, base, row0, xs, W);
    raw[1].load(a.in, base, row1, xs, W);
  }
  float su[8], sv[8];  // row-0 pair sums of the 8 chroma samples
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if constexpr (!kBoth)
      raw[r].load(a.in, base, r ? row1 : row0, xs, W);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float R[4], G[4], B[4];
      raw[r].px4(a.in, j, R, G, B);
      if constexpr (!d_isyuv(DST)) {
        // whole numbers 0..255: the packing instruction's own rounding and saturation have nothing left to do
        u32 r4 = 0, g4 = 0, b4 = 0;
#define VALI_PX(I) r4 = pack_u8<I>(R[I], r4), g4 = pack_u8<I>(G[I], g4), b4 = pack_u8<I>(B[I], b4);
        VALI_PX(0) VALI_PX(1) VALI_PX(2) VALI_PX(3)
#undef VALI_PX
        c0[r][j] = r4, c1[r][j] = g4, c2[r][j] = b4;
      } else {
        u32 y = 0, u = 0, v = 0;
        float fu[4], fv[4];
#define VALI_PX(I)                                                                                              \
  {                                                                                                             \
    y = pack_u8<I>(dot_rgb(a.m[0], R[I], G[I], B[I]), y);                                                       \
    fu[I] = dot_rgb(a.m[1], R[I], G[I], B[I]);                                                                  \
    fv[I] = dot_rgb(a.m[2], R[I], G[I], B[I]);                                                                  \
    if constexpr (DST == D_YUV444) {                                                                            \
      u = pack_u8<I>(fu[I], u);                                                                                 \
      v = pack_u8<I>(fv[I], v);                                                                                 \
    }                                                                                                           \
  }
        VALI_PX(0) VALI_PX(1) VALI_PX(2) VALI_PX(3)
#undef VALI_PX
        c0[r][j] = y;
        if constexpr (DST == D_YUV444) {
          c1[r][j] = u;
          c2[r][j] = v;
        } else {
          // 2 x 2 mean of the un-rounded chroma, ((c00 + c01) + (c10 + c11)) * 0.25: row 0 leaves its pair sums
          const float ua = fu[0] + fu[1], ub = fu[2] + fu[3], va = fv[0] + fv[1], vb = fv[2] + fv[3];
          if (r == 0) {
            su[2 * j] = ua, su[2 * j + 1] = ub, sv[2 * j] = va, sv[2 * j + 1] = vb;
          } else {
            const float mu0 = (su[2 * j] + ua) * 0.25f, mu1 = (su[2 * j + 1] + ub) * 0.25f;
            const float mv0 = (sv[2 * j] + va) * 0.25f, mv1 = (sv[2 * j + 1] + vb) * 0.25f;
            u32& qu = cu[j >> 1];
            u32& qv = cv[j >> 1];
            if (j & 1) {
              qu = pack_u8<2>(mu0, qu), qu = pack_u8<3>(mu1, qu), qv = pack_u8<2>(mv0, qv), qv = pack_u8<3>(mv1, qv);
            } else {
              qu = pack_u8<0>(mu0, 0u), qu = pack_u8<1>(mu1, qu), qv = pack_u8<0>(mv0, 0u), qv = pack_u8<1>(mv1, qv);
            }
          }
        }
      }
      // one 4-pixel group at a time (k_cvt8): interleaved, the groups' floats all live at once cost a wave per SIMD
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

template <int DT, bool PACKED, int DST, bool FAST>
__device__ __forceinline__ void t2s_body(const T2sArgs& a, PackedStrip* strip, const uint8_t* const (&plane)[3],
                                         const int (&pitch)[3], int item, int lane, int wave_g0, int crow) {
  typedef TensorIn<DT, PACKED, false> In;
  const int W = a.in.t.width, H = a.in.t.height;
  const int groups = (W + kLanePx - 1) / kLanePx;
  const int g = wave_g0 + lane;
  const bool lane_valid = g < groups;
  const int x0 = g * kLanePx;
  const bool cut = lane_valid && x0 + kLanePx > W;  // never when FAST
  const int xs = cut ? max(W - kLanePx, 0) : x0;    // the cut group slides left to end with the row
  const int n_px = min(kLanePx, W);                 // fewer than 16 only for frames narrower than one group
  const int row0 = crow * 2;
  const bool has_row1 = row0 + 1 < H;
  const int row1 = row0 + (has_row1 ? 1 : 0);

  u32 c0[2][4], c1[2][4], c2[2][4];  // full-resolution channels: Y, U, V or R, G, B
  u32 cu[2], cv[2];                  // 4:2:0 chroma: 8 samples each
  if (lane_valid) {
    const typename In::Item base = In::item(a.in, item);
    if (rows_vectorisable<DT, PACKED>(a.in, base, row0, row1, xs, W))
      t2s_block<DT, PACKED, DST, true>(a, base, row0, row1, xs, c0, c1, c2, cu, cv);
    else
      t2s_block<DT, PACKED, DST, false>(a, base, row0, row1, xs, c0, c1, c2, cu, cv);
  }

  uint8_t* const p0 = const_cast<uint8_t*>(plane[0]);
  uint8_t* const p1 = const_cast<uint8_t*>(plane[1]);
  uint8_t* const p2 = const_cast<uint8_t*>(plane[2]);
  if constexpr (DST == D_RGB) {
    // whole groups through the wave's strip (every lane of the wave takes part); the cut group's 48 bytes go direct
    const int full_lanes = min(kWave, W / kLanePx - wave_g0);
    const int vb = full_lanes * 48;
    u32 o[12];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (r == 1 && !has_row1)
        break;
      if (lane_valid)
        interleave3(c0[r], c1[r], c2[r], o);
      uint8_t* rb = p0 + (size_t)(row0 + r) * pitch[0];
      if constexpr (FAST) {
        strip_store_row(*strip, lane, o, lane_valid, rb + (size_t)wave_g0 * 48, vb);
      } else {
        strip_store_row_u(*strip, lane, o, lane_valid && !cut, rb + (size_t)wave_g0 * 48, vb);
        if (cut)
          packed_group_store(rb + (size_t)xs * 3, n_px, o);
      }
    }
    return;
  }
  if (!lane_valid)
    return;
  put16<FAST>(p0 + (size_t)row0 * pitch[0] + xs, c0[0], n_px);
  if (has_row1)
    put16<FAST>(p0 + (size_t)(row0 + 1) * pitch[0] + xs, c0[1], n_px);
  if constexpr (DST == D_YUV444 || DST == D_RGBP) {
    put16<FAST>(p1 + (size_t)row0 * pitch[1] + xs, c1[0], n_px);
    put16<FAST>(p2 + (size_t)row0 * pitch[2] + xs, c2[0], n_px);
    if (has_row1) {
      put16<FAST>(p1 + (size_t)(row0 + 1) * pitch[1] + xs, c1[1], n_px);
      put16<FAST>(p2 + (size_t)(row0 + 1) * pitch[2] + xs, c2[1], n_px);
    }
  } else if constexpr (DST == D_NV12) {
    const u32 uv[4] = {__builtin_amdgcn_perm(cv[0], cu[0], 0x05010400u), __builtin_amdgcn_perm(cv[0], cu[0], 0x07030602u),
                       __builtin_amdgcn_perm(cv[1], cu[1], 0x05010400u), __builtin_amdgcn_perm(cv[1], cu[1], 0x07030602u)};
    put16<FAST>(p1 + (size_t)crow * pitch[1] + xs, uv, n_px);
  } else if constexpr (DST == D_YUV420) {
    put8<FAST>(p1 + (size_t)crow * pitch[1] + xs / 2, cu[0], cu[1], n_px / 2);
    put8<FAST>(p2 + (size_t)crow * pitch[2] + xs / 2, cv[0], cv[1], n_px / 2);
  }
}

template <int DT, bool PACKED, int DST>
__global__ void __launch_bounds__(kBlock) k_tensor_to_surface(const T2sArgs a) {
  __shared__ PackedStrip strips[DST == D_RGB ? kWavesPerBlock : 1];
  const int W = a.in.t.width, H = a.in.t.height;
  // the wave's number as the scalar it is: row pointers then stay in scalar registers and a lane's address is one
  // 32-bit offset, not a 64-bit pointer per load (the per-element path holds up to 24 loads in flight)
  const int lane = threadIdx.x & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int wpr = (int)(blockDim.x / kWave) / a.rp;  // waves side by side on one row pair
  const int wave_g0 = ((int)blockIdx.x * wpr + wave % wpr) * kWave;
  const int crow = (int)blockIdx.y * a.rp + wave / wpr;  // row pair of this wave
  if (wave_g0 >= (W + kLanePx - 1) / kLanePx || crow * 2 >= H)
    return;  // the whole wave: the strip is per wave, there is no workgroup barrier
  const vali_surface* d = a.d_dst + blockIdx.z;
  const uint8_t* const plane[3] = {(const uint8_t*)d->plane[0], (const uint8_t*)d->plane[1], (const uint8_t*)d->plane[2]};
  const int pitch[3] = {d->pitch[0], d->pitch[1], d->pitch[2]};

  // uniform per surface: whole 16-pixel groups on aligned planes and pitches, or the ragged forms of the same stores
  uintptr_t bits = (uintptr_t)plane[0] | (uintptr_t)pitch[0];
  if constexpr (DST == D_NV12)
    bits |= (uintptr_t)plane[1] | (uintptr_t)pitch[1];
  if constexpr (DST == D_YUV444 || DST == D_RGBP)
    bits |= (uintptr_t)plane[1] | (uintptr_t)plane[2] | (uintptr_t)pitch[1] | (uintptr_t)pitch[2];
  if constexpr (DST == D_YUV420)  // 8-byte chroma pieces
    bits |= (((uintptr_t)plane[1] | (uintptr_t)plane[2] | (uintptr_t)pitch[1] | (uintptr_t)pitch[2]) & 7u) << 1;
  const bool fast = (W & (kLanePx - 1)) == 0 && (bits & 15u) == 0;
  PackedStrip* strip = &strips[DST == D_RGB ? wave : 0];
  if (fast)
    t2s_body<DT, PACKED, DST, true>(a, strip, plane, pitch, (int)blockIdx.z, lane, wave_g0, crow);
  else
    t2s_body<DT, PACKED, DST, false>(a, strip, plane, pitch, (int)blockIdx.z, lane, wave_g0, crow);
}

template <int DT, bool PACKED>
void launch_t2s(int dst, dim3 grid, int block, hipStream_t s, const T2sArgs& a) {
  switch (dst) {
  case D_NV12:
    hipLaunchKernelGGL((k_tensor_to_surface<DT, PACKED, D_NV12>), grid, dim3(block), 0, s, a);
    break;
  case D_YUV420:
    hipLaunchKernelGGL((k_tensor_to_surface<DT, PACKED, D_YUV420>), grid, dim3(block), 0, s, a);
    break;
  case D_YUV444:
    hipLaunchKernelGGL((k_tensor_to_surface<DT, PACKED, D_YUV444>), grid, dim3(block), 0, s, a);
    break;
  case D_RGB:
    hipLaunchKernelGGL((k_tensor_to_surface<DT, PACKED, D_RGB>), grid, dim3(block), 0, s, a);
    break;
  default:
    hipLaunchKernelGGL((k_tensor_to_surface<DT, PACKED, D_RGBP>), grid, dim3(block), 0, s, a);
    break;
  }
}

template <int DT>
void launch_t2s(bool packed, int dst, dim3 grid, int block, hipStream_t s, const T2sArgs& a) {
  if (packed)
    launch_t2s<DT, true>(dst, grid, block, s, a);
  else
    launch_t2s<DT, false>(dst, grid, block, s, a);
}

} // namespace
} // namespace vali

using namespace vali;

extern "C" {

int vali_tensor_to_surfaces(const vali_tensor_src* src, const float scale[3], const float offset[3], int bgr,
                            const vali_surface* d_dst, int dst_format, const vali_cvt_params* params,
                            vali_stream_t stream) {
  VALI_REQUIRE(src && scale && offset && d_dst, "null argument");
  int dst;
  switch (dst_format) {
  case VALI_FMT_NV12: dst = D_NV12; break;
  case VALI_FMT_YUV420: dst = D_YUV420; break;
  case VALI_FMT_YUV444: dst = D_YUV444; break;
  case VALI_FMT_RGB: dst = D_RGB; break;
  case VALI_FMT_RGB_PLANAR: dst = D_RGBP; break;
  default:
    return fail(VALI_ERR_UNSUPPORTED, "%s: destination format %d (NV12, YUV420, YUV444, RGB, RGB_PLANAR)", __func__,
                dst_format);
  }
  VALI_REQUIRE(params || !d_isyuv(dst), "a YUV destination needs params (rgb2yuv)");
  if (const int rc = check_tensor_src(__func__, src, scale, offset))
    return rc;
  VALI_REQUIRE(bgr == 0 || bgr == 1, "bgr must be 0 or 1");
  VALI_REQUIRE(!d_is420(dst) || ((src->width | src->height) & 1) == 0,
               "4:2:0 destinations (NV12, YUV420) need even width and height");

  T2sArgs a = {};
  a.in.t = *src;
  for (int c = 0; c < 3; ++c)
    a.in.scale[c] = scale[c], a.in.offset[c] = offset[c];
  a.in.swap_rb = bgr;
  a.d_dst = d_dst;
  if (d_isyuv(dst))
    for (int k = 0; k < 3; ++k)
      for (int j = 0; j < 4; ++j)
        a.m[k][j] = params->rgb2yuv[k][j];
  // k_cvt8's shape: a row of waves covers the width, narrow frames stack row pairs into the 256 threads
  const int groups = (src->width + kLanePx - 1) / kLanePx;
  int row_block = ((groups + kWave - 1) / kWave) * kWave;
  if (row_block > kBlock)
    row_block = kBlock;
  a.rp = kBlock / row_block;
  const int pairs = (src->height + 1) / 2;
  const dim3 grid((groups + row_block - 1) / row_block, (pairs + a.rp - 1) / a.rp, src->n);
  const int block = row_block * a.rp;
  const bool packed = src->packed != 0;

  hipStream_t s = as_stream(stream);
  VALI_ENTRY(s);
  with_src_dtype(src->dtype, [&](auto dt) { launch_t2s<dt>(packed, dst, grid, block, s, a); });
  VALI_LAUNCH_CHECK();
  return VALI_OK;
}

} // extern "C"
