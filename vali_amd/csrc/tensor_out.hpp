// What the kernels that WRITE one (N, 3, H, W) batch tensor share (vali_nv12_preproc_roi_tensor and
// vali_rgb_preproc_roi_tensor in preproc.hip, vali_warp_tensor in warp.hip), the counterpart of tensor_in.hpp: the
// conversions to the tensor's element types, the normalisation of a u8 value, the scalar load of a workgroup-uniform
// record, an item of the tensor as the planes of a surface, and on the host the rules of a vali_tensor_dst and the packing
// of the pad colour.  One copy, so the entry points cannot drift apart; tests/test_tensor_rules_host.py pins every refusal.
//
// The element TRAITS stay with their kernels (TdElem in preproc.hip, WElem in warp.hip): preproc.hip keeps a float32
// element as a float and a float table, warp.hip as its bits, and one trait for both would change the code of one of them.
// Both are thin: their 16-bit forms are the two conversions below.
#pragma once
#include "common.hpp"
#include "dev_util.hpp"

namespace vali {
namespace {

// float32 -> float16 bits, IEEE round-to-nearest-even in integers: independent of the wave's denormal mode (subnormal
// results are kept), magnitudes of 65520 and more give +-inf, NaN gives a quiet NaN.  torch.Tensor.to(torch.float16).
__device__ __forceinline__ u32 f32_to_f16_bits(float v) {
  const u32 x = __builtin_bit_cast(u32, v);
  const u32 sign = (x >> 16) & 0x8000u, a = x & 0x7fffffffu;
  if (a > 0x7f800000u)
    return sign | 0x7e00u;
  if (a >= 0x477ff000u) // 65520 = the tie between 65504 and 2^16, and everything above it
    return sign | 0x7c00u;
  if (a >= 0x38800000u) { // 2^-14 and more: a normal half; the carry of the rounding walks into the exponent
    const u32 r = a - 0x38000000u;
    return sign | ((r + 0xfffu + ((r >> 13) & 1u)) >> 13);
  }
  const u32 e = a >> 23;
  if (e < 102u) // below 2^-25: under half of the smallest subnormal (2^-25 itself is the tie with 0, handled below)
    return sign;
  // subnormal half: m * 2^(e - 150) in units of 2^-24 = m >> (126 - e), remainder rounded half to even
  const u32 m = (a & 0x7fffffu) | 0x800000u, sh = 126u - e; // sh = 14..24
  u32 q = m >> sh;
  const u32 rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1u);
  if (rem > half || (rem == half && (q & 1u)))
    ++q;
  return sign | q;
}

// float32 -> bfloat16 bits, round-to-nearest-even (torch.Tensor.to(torch.bfloat16)); NaN gives a quiet NaN
__device__ __forceinline__ u32 f32_to_bf16_bits(float v) {
  const u32 x = __builtin_bit_cast(u32, v);
  if ((x & 0x7fffffffu) > 0x7f800000u)
    return (x >> 16) | 0x40u;
  return (x + 0x7fffu + ((x >> 16) & 1u)) >> 16;
}

// the normalisation (q / 255 / div - mean[c]) / std[c] for (channel c, u8 value q): step 3 of vali_nv12_preproc, step 5 of
// vali_warp_tensor, operation for operation the table of k_nv12_preproc
__device__ __forceinline__ float normalise_u8(int q, int c, const vali_preproc_params& prm) {
  const float f = (float)q / 255.0f;
  const float g = f / prm.div;
  return (g - prm.mean[c]) / prm.std_[c];
}

// A workgroup-uniform record of a device array (descriptor, rectangle, matrix row) read through the constant address
// space: the index is uniform, so these are scalar loads into SGPRs (through generic pointers they would be flat vector
// loads).  `one` serves the entry points that pass ONE record by value instead of an array: `arr` is null, take `*one`.
#define VALI_CONST __attribute__((address_space(4)))
template <typename T> __device__ __forceinline__ T load_uniform(const T* arr, u32 index, const T* one = nullptr) {
  static_assert(sizeof(T) % 4 == 0, "records of whole dwords");
  if (one && !arr)
    return *one;
  const VALI_CONST u32* q = (const VALI_CONST u32*)(arr + index);
  u32 w[sizeof(T) / 4];
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / 4; ++i)
    w[i] = q[i];
  T v;
  __builtin_memcpy(&v, w, sizeof(T));
  return v;
}

// item `frame` of the batch tensor as the planes of a surface: addresses in 64 bits, the pitch in bytes (the host has
// checked that it and height x pitch fit the 32-bit in-plane offset)
template <int ESIZE> __device__ __forceinline__ SurfRef tensor_ref(const vali_tensor_dst& t, u32 frame) {
  SurfRef r;
  uint8_t* base = (uint8_t*)t.data + (long long)frame * t.stride_n * ESIZE;
  r.p[0] = base;
  r.p[1] = base + (t.packed ? 0 : t.stride_c * ESIZE);
  r.p[2] = base + (t.packed ? 0 : 2 * t.stride_c * ESIZE);
  r.pitch[0] = r.pitch[1] = r.pitch[2] = (int)(t.stride_y * ESIZE);
  r.width = t.width; r.height = t.height;
  return r;
}

// ---- the host ----------------------------------------------------------------------------------------------------------------
// The rules of a vali_tensor_dst, for the entry point `who`.  even: the canvas of a 4:2:0 source, at least 2 x 2 and even;
// otherwise any size from 1 x 1.
int check_tensor_dst(const char* who, const vali_tensor_dst* t, bool even) {
#define VALI_T_REQUIRE(cond, msg)                                              \
  do {                                                                         \
    if (!(cond))                                                               \
      return fail(VALI_ERR_INVALID_ARG, "%s: %s", who, msg);                   \
  } while (0)
  VALI_T_REQUIRE(t->data, "null tensor data");
  VALI_T_REQUIRE(t->dtype >= VALI_DTYPE_F32 && t->dtype <= VALI_DTYPE_BF16, "dtype must be VALI_DTYPE_F32, _F16 or _BF16");
  VALI_T_REQUIRE(t->packed == 0 || t->packed == 1, "packed must be 0 or 1");
  VALI_T_REQUIRE(t->n >= 1 && t->n <= 65535, "batch size out of range (1..65535)");
  if (even)
    VALI_T_REQUIRE(t->width >= 2 && t->height >= 2 && ((t->width | t->height) & 1) == 0, "bad geometry");
  else
    VALI_T_REQUIRE(t->width >= 1 && t->height >= 1, "bad geometry");
  VALI_T_REQUIRE(t->stride_n > 0 && t->stride_y > 0 && (t->packed || t->stride_c > 0), "strides must be positive");
  VALI_T_REQUIRE(t->stride_y >= (int64_t)t->width * (t->packed ? 3 : 1), "stride_y is shorter than a row");
  const int64_t esize = t->dtype == VALI_DTYPE_F32 ? 4 : 2;
  VALI_T_REQUIRE(((uintptr_t)t->data & (uintptr_t)(esize - 1)) == 0, "data is not aligned to its element");
  // the kernels address a row as (u32)(y * pitch) inside its plane
  VALI_T_REQUIRE(t->stride_y <= (int64_t)0x7fffffff / esize &&
                     (uint64_t)t->height * (uint64_t)(t->stride_y * esize) < (1ull << 32),
                 "row pitch of 2 GiB or plane of 4 GiB or more");
#undef VALI_T_REQUIRE
  return VALI_OK;
}

// the pad colour as the kernels take it, R | G << 8 | B << 16; 0 without padding (pad_rgb may be null then)
u32 pad_colour(int pad, const uint8_t* pad_rgb) {
  return pad ? (u32)pad_rgb[0] | (u32)pad_rgb[1] << 8 | (u32)pad_rgb[2] << 16 : 0u;
}

} // namespace
} // namespace vali
