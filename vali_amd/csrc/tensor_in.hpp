// What the kernels that READ a tensor share.  For one (N, 3, H, W) batch tensor (vali_jpeg_encode_tensor,
// vali_tensor_to_surfaces): the element types, the row loaders and the quantiser of the definition in include/vali_hip.h,
// and the host rules of a vali_tensor_src.  For the heads of a network, whose strides are free (vali_detect_select,
// vali_mask_paint, vali_semantic_paint, vali_pose_paint, vali_warp_fit, vali_kpt_decode): the element types and the host
// rule of such a tensor.  For both: the step from a run-time dtype to a kernel of that element type.  One copy, so the
// entry points cannot drift apart; tests/test_tensor_rules_host.py, tests/test_jpeg_tensor_host.py and
// tests/test_gpu_jpeg_tensor.py pin it.  The tensors that are WRITTEN have tensor_out.hpp.
// The host rules live here and not in a header of their own: every file that includes this one has common.hpp already.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <type_traits>

#include "../../include/vali_hip.h"
#include "common.hpp"

namespace vali {
namespace {

typedef uint32_t u32;
typedef uint8_t u8;

// ---- the host --------------------------------------------------------------------------------------------------------------
// A run-time dtype as a compile-time constant: f(std::integral_constant<int, DT>()) for the DT that `dtype` names, so a
// generic lambda launches the kernel of that element type.  The caller has checked the dtype; the last case takes the rest.
template <typename F> void with_float_dtype(int dtype, F&& f) {
  switch (dtype) {
  case VALI_DTYPE_F32: f(std::integral_constant<int, VALI_DTYPE_F32>()); break;
  case VALI_DTYPE_F16: f(std::integral_constant<int, VALI_DTYPE_F16>()); break;
  default: f(std::integral_constant<int, VALI_DTYPE_BF16>()); break;
  }
}
// ... and uint8, for the entry points that read a vali_tensor_src
template <typename F> void with_src_dtype(int dtype, F&& f) {
  if (dtype >= VALI_DTYPE_F32 && dtype <= VALI_DTYPE_BF16)
    with_float_dtype(dtype, f);
  else
    f(std::integral_constant<int, VALI_DTYPE_U8>());
}

// the predicates of a head tensor: a float dtype, its element size, strides in 0..2^40
inline bool float_dtype(int dtype) { return dtype == VALI_DTYPE_F32 || dtype == VALI_DTYPE_F16 || dtype == VALI_DTYPE_BF16; }
inline int float_dtype_size(int dtype) { return dtype == VALI_DTYPE_F32 ? 4 : 2; }
inline bool strides_ok(const int64_t* s, int n) {
  for (int i = 0; i < n; ++i)
    if (s[i] < 0 || s[i] > ((int64_t)1 << 40))
      return false;
  return true;
}

// The rule of a head tensor `name` of `count` (at most 4) strides, for the entry point `who`: a pointer, a float dtype,
// alignment to the element, strides in 0..2^40.
int check_head_tensor(const char* who, const char* name, const void* data, int dtype, const int64_t* strides, int count) {
  if (!data)
    return fail(VALI_ERR_INVALID_ARG, "%s: %s has a null pointer", who, name);
  if (!float_dtype(dtype))
    return fail(VALI_ERR_INVALID_ARG, "%s: %s: dtype %d is not float32, float16 or bfloat16", who, name, dtype);
  if (((uintptr_t)data & (uintptr_t)(float_dtype_size(dtype) - 1)) != 0)
    return fail(VALI_ERR_INVALID_ARG, "%s: %s is not aligned to its element size", who, name);
  if (!strides_ok(strides, count)) {
    char list[4 * 24];
    int at = 0;
    for (int i = 0; i < count && i < 4; ++i)
      at += snprintf(list + at, sizeof(list) - at, i ? ", %lld" : "%lld", (long long)strides[i]);
    return fail(VALI_ERR_INVALID_ARG, "%s: %s: strides (%s) outside 0..2^40", who, name, list);
  }
  return VALI_OK;
}

// The rules of a vali_tensor_src and of the scale and offset that go with it, for the entry point `who`.
int check_tensor_src(const char* who, const vali_tensor_src* src, const float scale[3], const float offset[3]) {
#define VALI_T_REQUIRE(cond, msg)                                              \
  do {                                                                         \
    if (!(cond))                                                               \
      return fail(VALI_ERR_INVALID_ARG, "%s: %s", who, msg);                   \
  } while (0)
  VALI_T_REQUIRE(src->data, "null tensor data");
  VALI_T_REQUIRE(src->dtype >= VALI_DTYPE_F32 && src->dtype <= VALI_DTYPE_U8,
                 "dtype must be VALI_DTYPE_F32, _F16, _BF16 or _U8");
  VALI_T_REQUIRE(src->packed == 0 || src->packed == 1, "packed must be 0 or 1");
  VALI_T_REQUIRE(src->n >= 1 && src->n <= 65535, "batch size out of range (1..65535)");
  VALI_T_REQUIRE(src->width >= 1 && src->height >= 1 && src->width <= 65535 && src->height <= 65535,
                 "size outside 1..65535");
  VALI_T_REQUIRE(src->stride_n > 0 && src->stride_y > 0 && (src->packed || src->stride_c > 0),
                 "strides must be positive");
  VALI_T_REQUIRE(src->stride_y >= (int64_t)src->width * (src->packed ? 3 : 1), "stride_y is shorter than a row");
  const uintptr_t esize = src->dtype == VALI_DTYPE_F32 ? 4 : src->dtype == VALI_DTYPE_U8 ? 1 : 2;
  VALI_T_REQUIRE(((uintptr_t)src->data & (esize - 1)) == 0, "data is not aligned to its element");
  for (int c = 0; c < 3; ++c)
    VALI_T_REQUIRE(isfinite(scale[c]) && isfinite(offset[c]), "scale and offset must be finite");
#undef VALI_T_REQUIRE
  return VALI_OK;
}

// ---- the device ------------------------------------------------------------------------------------------------------------

// One (N, 3, H, W) tensor (vali_jpeg_encode_tensor): elements are quantised in registers on their way in.
struct TensorArgs {
  vali_tensor_src t;
  float scale[3], offset[3];
  int swap_rb;  // BGR: tensor channel 0 is blue
};

// an element from its bits, as float32: exact for every dtype
template <int DT>
struct TensorElem;
template <>
struct TensorElem<VALI_DTYPE_F32> {
  typedef u32 Bits;
  static __device__ __forceinline__ float f(u32 b) { return __uint_as_float(b); }
};
template <>
struct TensorElem<VALI_DTYPE_F16> {
  typedef uint16_t Bits;
  static __device__ __forceinline__ float f(u32 b) { return (float)__builtin_bit_cast(_Float16, (uint16_t)b); }
};
template <>
struct TensorElem<VALI_DTYPE_BF16> {
  typedef uint16_t Bits;
  static __device__ __forceinline__ float f(u32 b) { return __uint_as_float(b << 16); }
};
template <>
struct TensorElem<VALI_DTYPE_U8> {
  typedef u8 Bits;
  static __device__ __forceinline__ float f(u32 b) { return (float)b; }
};

// element i of a float32, float16 or bfloat16 tensor whose dtype is known at run time only (the heads that
// vali_detect_select and vali_mask_paint read)
__device__ __forceinline__ float tensor_elem_f(const void* p, int dt, long long i) {
  if (dt == VALI_DTYPE_F32)
    return ((const float*)p)[i];
  const u32 b = ((const uint16_t*)p)[i];
  return dt == VALI_DTYPE_F16 ? TensorElem<VALI_DTYPE_F16>::f(b) : TensorElem<VALI_DTYPE_BF16>::f(b);
}

// element i of a run of elements held in dwords
template <int ES>
__device__ __forceinline__ u32 elem_bits(const u32* w, int i) {
  return ES == 4 ? w[i] : ES == 2 ? (w[i / 2] >> (16 * (i % 2))) & 0xFFFF : (w[i / 4] >> (8 * (i % 4))) & 0xFF;
}

// NE elements from p into dwords: 16-byte loads (p is 16-byte aligned), for uint8 dwords (p is 4-byte aligned)
template <int ES, int NE>
__device__ __forceinline__ void load_elems(const void* p, u32* w) {
  if (ES == 1) {
#pragma unroll
    for (int i = 0; i < NE / 4; ++i)
      w[i] = ((const u32*)p)[i];
  } else {
#pragma unroll
    for (int i = 0; i < NE * ES / 16; ++i) {
      const uint4 q = ((const uint4*)p)[i];
      w[4 * i] = q.x, w[4 * i + 1] = q.y, w[4 * i + 2] = q.z, w[4 * i + 3] = q.w;
    }
  }
}

// p of the definition (include/vali_hip.h): two roundings, never an FMA; NaN -> 0; clamping first leaves rint nothing
// outside 0..255 and changes no result
// (quantise_elem_f: p as the float it is before the conversion, for the kernels that go on in floating point)
__device__ __forceinline__ float quantise_elem_f(float e, float scale, float offset) {
#pragma clang fp contract(off)
  float v = __fadd_rn(__fmul_rn(e, scale), offset);
  v = v != v ? 0.0f : v;
  return rintf(fminf(fmaxf(v, 0.0f), 255.0f));
}
__device__ __forceinline__ int quantise_elem(float e, float scale, float offset) {
  return (int)quantise_elem_f(e, scale, offset);
}

template <int DT, bool PACKED, bool YUV>
struct TensorIn {
  static constexpr bool kYuv = YUV;
  typedef TensorArgs Args;
  typedef TensorElem<DT> E;
  typedef typename E::Bits Bits;
  static constexpr int ES = sizeof(Bits);
  static constexpr uintptr_t kAlign = ES == 1 ? 3 : 15;  // of the vector path
  typedef const Bits* Item;  // element (item, 0, 0, 0)
  static __device__ __forceinline__ Item item(const Args& a, int i) {
    return (const Bits*)a.t.data + (size_t)i * (size_t)a.t.stride_n;
  }

  // 8 raw elements of channel c of a planar row
  static __device__ __forceinline__ void planar_row(const Args& a, Item base, int c, int y, int x0, int cw,
                                                    float e[8]) {
    const Bits* row = base + (size_t)c * (size_t)a.t.stride_c + (size_t)y * (size_t)a.t.stride_y;
    const Bits* p = row + x0;
    if (x0 + 8 <= cw && (((uintptr_t)p) & kAlign) == 0) {
      u32 w[2 * ES];
      load_elems<ES, 8>(p, w);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        e[i] = E::f(elem_bits<ES>(w, i));
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        e[i] = E::f(row[min(x0 + i, cw - 1)]);
    }
  }
  // 8 raw pixels of a channels-last row: e[k] is tensor channel k
  static __device__ __forceinline__ void packed_row(const Args& a, Item base, int y, int x0, int cw, float e[3][8]) {
    const Bits* row = base + (size_t)y * (size_t)a.t.stride_y;
    const Bits* p = row + 3 * x0;
    if (x0 + 8 <= cw && (((uintptr_t)p) & kAlign) == 0) {
      u32 w[6 * ES];
      load_elems<ES, 24>(p, w);
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k)
          e[k][i] = E::f(elem_bits<ES>(w, 3 * i + k));
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const Bits* q = row + 3 * min(x0 + i, cw - 1);
#pragma unroll
        for (int k = 0; k < 3; ++k)
          e[k][i] = E::f(q[k]);
      }
    }
  }

  // 4 raw pixels from column x0, clamped to the last column, one load per element whatever the alignment: e[k][i] is
  // tensor channel k (the narrow form of the per-element paths above, for callers that walk a row in a rolled loop)
  static __device__ __forceinline__ void pixels4(const Args& a, Item base, int y, int x0, int cw, float e[3][4]) {
    const Bits* row = base + (size_t)y * (size_t)a.t.stride_y;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int x = min(x0 + i, cw - 1);
#pragma unroll
      for (int k = 0; k < 3; ++k)
        e[k][i] = E::f(PACKED ? row[3 * x + k] : row[(size_t)k * (size_t)a.t.stride_c + x]);
    }
  }

  static __device__ __forceinline__ void rgb_row(const Args& a, Item base, int y, int x0, int cw, int R[8], int G[8],
                                                 int B[8]) {
    const bool swap = a.swap_rb != 0;
    if (PACKED) {
      float e[3][8];
      packed_row(a, base, y, x0, cw, e);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int p0 = quantise_elem(e[0][i], a.scale[0], a.offset[0]);
        const int p2 = quantise_elem(e[2][i], a.scale[2], a.offset[2]);
        G[i] = quantise_elem(e[1][i], a.scale[1], a.offset[1]);
        R[i] = swap ? p2 : p0;
        B[i] = swap ? p0 : p2;
      }
    } else {
      // the channel order decides which plane feeds R and B, not what is computed
      const int cr = swap ? 2 : 0, cb = 2 - cr;
      const float sr = swap ? a.scale[2] : a.scale[0], orr = swap ? a.offset[2] : a.offset[0];
      const float sb = swap ? a.scale[0] : a.scale[2], ob = swap ? a.offset[0] : a.offset[2];
      float e[8];
      planar_row(a, base, cr, y, x0, cw, e);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        R[i] = quantise_elem(e[i], sr, orr);
      planar_row(a, base, 1, y, x0, cw, e);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        G[i] = quantise_elem(e[i], a.scale[1], a.offset[1]);
      planar_row(a, base, cb, y, x0, cw, e);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        B[i] = quantise_elem(e[i], sb, ob);
    }
  }
  static __device__ __forceinline__ void comp_row(const Args& a, Item base, int c, int y, int x0, int cw, int v[8]) {
    const float sc = c == 0 ? a.scale[0] : c == 1 ? a.scale[1] : a.scale[2];
    const float of = c == 0 ? a.offset[0] : c == 1 ? a.offset[1] : a.offset[2];
    float e[8];
    if (PACKED) {
      // the lane's own channel only: every third element, one load each (the clamped form serves the right edge too)
      const Bits* row = base + (size_t)y * (size_t)a.t.stride_y + c;
#pragma unroll
      for (int i = 0; i < 8; ++i)
        e[i] = E::f(row[3 * min(x0 + i, cw - 1)]);
    } else {
      planar_row(a, base, c, y, x0, cw, e);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
      v[i] = quantise_elem(e[i], sc, of);
  }
};

} // namespace
} // namespace vali
