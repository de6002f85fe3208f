// What the kernels that paint IN PLACE onto 64 x 64 luma tiles of a frame batch share (vali_annotate_batch and
// vali_annotate_batch_atlas in annotate.hip, vali_mask_paint in mask.hip): the formats and the rules for the frames, a
// lane's 16-byte pieces of the tile, the ordered hit list, the colour of a piece's bytes and the blend of that colour
// with a coverage byte per pixel.  One copy, so the painters cannot drift apart where labels and masks meet
// on one frame: the blend's rounding, the 4:2:0 chroma mean, the byte-to-channel mapping of packed RGB and the clipping
// at the right edge are pinned by tests/test_gpu_annotate.py, tests/test_gpu_annotate_stamps.py and
// tests/test_gpu_masks.py against tests/annotate_model.py and tests/mask_model.py.
#pragma once
#include "common.hpp"
#include "dev_util.hpp"

namespace vali {
namespace {

constexpr int kTile = 64;  // luma pixels a side

enum TileFmt : int { A_NV12 = 0, A_YUV420 = 1, A_YUV444 = 2, A_RGB = 3, A_BGR = 4, A_RGBP = 5 };

constexpr bool a_is420(int f) { return f == A_NV12 || f == A_YUV420; }
constexpr bool a_isyuv(int f) { return f == A_NV12 || f == A_YUV420 || f == A_YUV444; }

// A lane's share of the tile: piece (lane + first) of plane `plane`, whose bytes interleave `nc` channels starting with
// colour channel c0 (0, 1, 2 = Y, U, V or the format's first, second, third stored colour) at 1 >> sh samples per pixel
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

__device__ __forceinline__ int clampi(long long v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : (int)v; }

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

// what a lane keeps of one of its pieces
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

// the colour of byte b of a piece is c[b % nc]: packed RGB pieces start at any of the three channels
template <int FMT, int S>
__device__ __forceinline__ void piece_colours(int lbx, const u32 (&col)[3], u32 (&c)[3]) {
  constexpr Slot sl = slot_of(FMT, S);
  constexpr int nc = sl.nc;
  if constexpr (nc == 3) {
    // (shifts of one packed word: a select chain over col[] becomes a table in scratch memory)
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

// The colour blended onto one piece with a weight per pixel: lane-local.  Cov is where the weights come from: it has
// coverage inside its rectangle rx0 .. ry1 of the frame only, and get<N>(X, py, cv) gives the coverage of the N (16, or 6
// for a packed RGB piece) frame pixels X .. X + N - 1 of frame row py, a byte each, zero outside the rectangle.
template <int FMT, int S, class Cov>
__device__ __forceinline__ void cover_piece(const Cov& cov, const Piece& pc, const u32 (&col)[3], u32 alpha, u32 (&w)[4]) {
  constexpr Slot sl = slot_of(FMT, S);
  constexpr int nc = sl.nc, sh = sl.sh;
  // the luma pixels under the piece: `span` columns from X, 1 << sh rows from Y
  constexpr int span = nc == 3 ? 6 : (16 / nc) << sh;
  const int X = nc == 3 ? pc.bx / 3 : (pc.bx / nc) << sh, Y = pc.y << sh;
  if (pc.n <= 0 || Y >= cov.ry1 || Y + (1 << sh) <= cov.ry0 || X >= cov.rx1 || X + span <= cov.rx0)
    return;
  u32 k[4] = {0u, 0u, 0u, 0u};  // the weight of every byte of the piece
  if constexpr (nc == 3) {
    // byte b belongs to pixel (ch0 + b) / 3 of the six, ch0 the channel the piece starts with: every weight three times
    // (byte selects with constant selectors), then the 16 bytes from ch0 on -- nothing here but ch0 is the same for
    // every hit, so nothing else is kept in registers across the hits
    u32 cv[2];
    cov.template get<6>(X, Y, cv);
    if ((cv[0] | cv[1]) == 0u)
      return;
    const u32 ch0 = (u32)pc.bx - 3u * (u32)X;
    const u32 e0 = __builtin_amdgcn_perm(0u, cv[0], 0x01000000u), e1 = __builtin_amdgcn_perm(0u, cv[0], 0x02020101u);
    const u32 e2 = __builtin_amdgcn_perm(0u, cv[0], 0x03030302u), e3 = __builtin_amdgcn_perm(0u, cv[1], 0x01000000u);
    const u32 e4 = __builtin_amdgcn_perm(0u, cv[1], 0x01010101u);
    k[0] = __builtin_amdgcn_alignbyte(e1, e0, ch0), k[1] = __builtin_amdgcn_alignbyte(e2, e1, ch0);
    k[2] = __builtin_amdgcn_alignbyte(e3, e2, ch0), k[3] = __builtin_amdgcn_alignbyte(e4, e3, ch0);
  } else if constexpr (sh == 0) {
    cov.template get<16>(X, Y, k);
  } else {
    // a 4:2:0 chroma sample: the rounded mean of the coverage of its four luma pixels, two 16-bit sums to a word
#pragma unroll
    for (int g = 0; g < span / 16; ++g) {
      u32 r0[4], r1[4];
      cov.template get<16>(X + 16 * g, Y, r0);
      cov.template get<16>(X + 16 * g, Y + 1, r1);
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
  // per word, so that a word of weights is spent before the next is formed
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

// only what was changed goes back
__device__ __forceinline__ void store_piece(const Piece& pc, const u32 (&cur)[4], const u32 (&orig)[4]) {
  const bool changed = ((cur[0] ^ orig[0]) | (cur[1] ^ orig[1]) | (cur[2] ^ orig[2]) | (cur[3] ^ orig[3])) != 0u;
  if (pc.n > 0 && changed)
    store16_n(pc.p, make_uint4(cur[0], cur[1], cur[2], cur[3]), pc.n);
}

// Once per slot of the format (NS = nslots(FMT) in the kernel): a slot's layout is a template argument, so the slots are
// spelled out, not looped over.  A file that includes this header #undefs VALI_SLOTS after its last kernel.
#define VALI_SLOTS(CALL)    \
  {                         \
    CALL(0)                 \
    CALL(1)                 \
    if constexpr (NS > 2) { \
      CALL(2)               \
    }                       \
  }

// enum vali_format -> TileFmt, -1: not a format the painters draw on
int tile_format(int format) {
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

// A run-time TileFmt as a compile-time constant: f(std::integral_constant<int, FMT>()), so a generic lambda launches the
// painter of that format.  The caller has checked the format; the last case takes the rest.
template <typename F> void with_tile_format(int fmt, F&& f) {
  switch (fmt) {
  case A_NV12: f(std::integral_constant<int, A_NV12>()); break;
  case A_YUV420: f(std::integral_constant<int, A_YUV420>()); break;
  case A_YUV444: f(std::integral_constant<int, A_YUV444>()); break;
  case A_RGB: f(std::integral_constant<int, A_RGB>()); break;
  case A_BGR: f(std::integral_constant<int, A_BGR>()); break;
  default: f(std::integral_constant<int, A_RGBP>()); break;
  }
}

// the rules for the frames of a batch; *max_tiles: the tiles of the largest one
int check_frames(const char* who, int n, const vali_surface* frames, int format, int* max_tiles) {
  const int fmt = tile_format(format);
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

} // namespace
} // namespace vali
