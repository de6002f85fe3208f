// Marks on frames (vali_annotate_batch): outlines, translucent fills and pixelation drawn IN PLACE onto a batch of NV12,
// YUV420, YUV444, RGB, BGR or RGB_PLANAR frames of any sizes, from a list of marks that lives in DEVICE memory -- the
// step between a detector's output and PyNvEncoder / the JPEG encoder, without the device-to-host copy and the four
// launches per box and plane of torch slice assignments.
//
// Definition: include/vali_hip.h ("marks on frames"); tests/annotate_model.py restates it in numpy.
//
// Drawing in place is deterministic without any ordering between workgroups because of cell alignment: a workgroup owns
// one 64 x 64 luma tile of one frame, aligned to the frame's origin; pixelation cells (4 .. 32) divide 64 and sit on the
// frame's grid, so every cell lies inside one tile.  The workgroup applies ALL marks that meet its tile, in row order, to
// samples it holds in registers, and stores each 16-byte piece once -- and only if a mark changed it.
//
// Two launches, whatever m and the data:
//   k_annotate_bin   one workgroup per frame: sanitises the rows and leaves, in the workspace, the indices of the rows
//                    that draw on its frame, in row order (a ballot / prefix compaction).  The tiles then scan their
//                    frame's rows, not all m: m * 32 bytes per TILE was the alternative
//   k_annotate<FMT, STAMPS>
//                    grid (tiles of the largest frame, n).  A tile whose frame has no row leaves after two scalar loads;
//                    otherwise it culls the frame's rows against the tile into an LDS hit list (again in order) and, with
//                    no hit, leaves without touching a pixel
// A lane owns the same 16-byte pieces of the tile throughout (one of Y, one of interleaved UV; three of packed RGB; one
// of each plane of the planar formats): loaded and stored as 16-byte vectors at any alignment, byte by byte only where
// the frame's right edge cuts a piece.  Fills and outlines are therefore lane-local and need no barrier; only pixelation
// goes through LDS (integer atomic adds into per-cell sums: the sum does not depend on the order) and is fenced by
// barriers.  Every branch on the mark kind is workgroup-uniform; the mark records are read at a uniform index.
//
// Stamps (vali_annotate_batch_atlas, VALI_MARK_STAMP) blend the mark's colour with a per-pixel weight from a coverage
// atlas: lane-local like FILL (cover_piece over a StampCov), the lane reads the coverage bytes its pieces need straight
// from the atlas, which is small, re-read by many tiles and therefore served by the L2.  k_annotate<FMT, true> holds that
// path; a call without an atlas launches k_annotate<FMT, false>, which is the kernel as it was before stamps existed.
//
// The formats and the frame rules, the tile's pieces, the hit list and the coverage blend are tile_paint.hpp's, shared
// with mask.hip; here are the marks, FILL / BOX, PIXELATE and the atlas reads.
#include "tile_paint.hpp"

namespace vali {
namespace {

constexpr int kMaxMarks = VALI_MAX_MARKS;
constexpr size_t kBinBytes = 16 + (size_t)kMaxMarks * 2;  // per frame: the count, then uint16 row indices in row order
constexpr int kCells = (kTile / 4) * (kTile / 4) * 3;   // cell sums of a tile: 16 x 16 cells of 4, three channels

// A sanitised row: what it paints, clipped to the frame (all values in 0 .. W resp. 0 .. H)
struct Mark {
  int kind;
  int x0, y0, x1, y1;      // the area it touches: rectangle ^ frame (pixelate: grown to the cell grid first)
  int ix0, iy0, ix1, iy1;  // BOX: the inner rectangle that stays as it is (empty: all 0)
  int cell;                // PIXELATE
  u32 colour;
};
// STAMP (kept apart from Mark, which the kernel without stamps resolves too): the pixels that have coverage,
// rectangle ^ atlas ^ frame, NOT snapped on 4:2:0 frames (the Mark's x0 .. y1 are, for culling); frame pixel (px, py)
// reads atlas[py + oy][px + ox]
struct Stamp {
  int rx0, ry0, rx1, ry1;
  int ox, oy;
};

__device__ __forceinline__ void load_mark(const vali_mark* marks, int i, int (&r)[8]) {
  const uint4 a = load16_u((const uint8_t*)(marks + i)), b = load16_u((const uint8_t*)(marks + i) + 16);
  r[0] = (int)a.x, r[1] = (int)a.y, r[2] = (int)a.z, r[3] = (int)a.w;
  r[4] = (int)b.x, r[5] = (int)b.y, r[6] = (int)b.z, r[7] = (int)b.w;
}

// false: the row is skipped (the rules of include/vali_hip.h; the frame index is the caller's to check).  AW x AH: the
// atlas, 0 x 0 without one -- VALI_MARK_STAMP is then an unknown kind
__device__ __forceinline__ bool resolve_mark(const int (&r)[8], int W, int H, bool is420, int AW, int AH, Mark& m) {
  const int kind = r[5], arg = r[6];
  if (kind < VALI_MARK_BOX || kind > (AW > 0 ? VALI_MARK_STAMP : VALI_MARK_PIXELATE) || r[3] < 1 || r[4] < 1)
    return false;
  if (kind == VALI_MARK_BOX && arg < 1)
    return false;
  if (kind == VALI_MARK_PIXELATE && arg != 4 && arg != 8 && arg != 16 && arg != 32)
    return false;
  // 64 bits: x + w and x + t overflow int32
  long long x0 = r[1], y0 = r[2], x1 = x0 + r[3], y1 = y0 + r[4], t = arg;
  if (AW > 0 && kind == VALI_MARK_STAMP) {
    const int u = arg & 0xffff, v = (arg >> 16) & 0xffff;
    if (u >= AW || v >= AH)
      return false;
    // beyond the atlas the coverage is zero: the rectangle ends where the atlas does
    x1 = min(x1, x0 + (AW - u)), y1 = min(y1, y0 + (AH - v));
  }
  if (is420) {
    x0 &= ~1ll, y0 &= ~1ll, x1 = (x1 + 1) & ~1ll, y1 = (y1 + 1) & ~1ll, t = (t + 1) & ~1ll;
  }
  if (x0 >= W || y0 >= H || x1 <= 0 || y1 <= 0)
    return false;
  m.kind = kind;
  m.colour = (u32)r[7];
  m.x0 = clampi(x0, 0, W), m.y0 = clampi(y0, 0, H), m.x1 = clampi(x1, 0, W), m.y1 = clampi(y1, 0, H);
  m.ix0 = m.iy0 = m.ix1 = m.iy1 = 0;
  m.cell = 0;
  if (kind == VALI_MARK_PIXELATE) {
    const int s = arg;
    m.cell = s;
    m.x0 = m.x0 / s * s, m.y0 = m.y0 / s * s;
    m.x1 = min((m.x1 + s - 1) / s * s, W), m.y1 = min((m.y1 + s - 1) / s * s, H);
  } else if (kind == VALI_MARK_BOX) {
    const int ix0 = clampi(x0 + t, 0, W), ix1 = clampi(x1 - t, 0, W);
    const int iy0 = clampi(y0 + t, 0, H), iy1 = clampi(y1 - t, 0, H);
    if (ix0 < ix1 && iy0 < iy1)
      m.ix0 = ix0, m.ix1 = ix1, m.iy0 = iy0, m.iy1 = iy1;
  }
  return true;
}

// a STAMP row that resolve_mark let through
__device__ __forceinline__ void resolve_stamp(const int (&r)[8], int W, int H, int AW, int AH, Stamp& st) {
  const int u = r[6] & 0xffff, v = (r[6] >> 16) & 0xffff;
  // 32 bits do: a rectangle that meets its frame starts above -65535, and the atlas ends it within 65535 pixels
  const int x0 = r[1], y0 = r[2], x1 = x0 + min(r[3], AW - u), y1 = y0 + min(r[4], AH - v);
  st.rx0 = min(max(x0, 0), W), st.ry0 = min(max(y0, 0), H), st.rx1 = min(max(x1, 0), W), st.ry1 = min(max(y1, 0), H);
  st.ox = u - x0, st.oy = v - y0;
}

// does the mark paint inside the tile [tx0, tx0 + 64) x [ty0, ty0 + 64) of a W x H frame
__device__ __forceinline__ bool mark_meets_tile(const Mark& m, int tx0, int ty0, int W, int H) {
  const int tx1 = min(tx0 + kTile, W), ty1 = min(ty0 + kTile, H);
  if (m.x0 >= tx1 || m.x1 <= tx0 || m.y0 >= ty1 || m.y1 <= ty0)
    return false;
  // a tile wholly inside an outline's inner rectangle
  return !(tx0 >= m.ix0 && tx1 <= m.ix1 && ty0 >= m.iy0 && ty1 <= m.iy1);
}

// ---- launch 1: the rows of each frame ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_annotate_bin(const vali_surface* __restrict__ d_frames,
                                                         const vali_mark* __restrict__ marks, int m, int is420,
                                                         int AW, int AH, uint8_t* __restrict__ ws) {
  __shared__ int wtot[kWavesPerBlock];
  const int f = blockIdx.x;
  const int W = d_frames[f].width, H = d_frames[f].height;
  uint8_t* bin = ws + (size_t)f * kBinBytes;
  uint16_t* list = (uint16_t*)(bin + 16);
  int total = 0;
  for (int base = 0; base < m; base += kBlock) {
    const int i = base + (int)threadIdx.x;
    bool flag = false;
    if (i < m) {
      int r[8];
      load_mark(marks, i, r);
      Mark mk;
      flag = r[0] == f && resolve_mark(r, W, H, is420 != 0, AW, AH, mk);
    }
    total = compact_put(flag, i, list, total, wtot);
  }
  if (threadIdx.x == 0)
    *(u32*)bin = (u32)total;
}

// ---- launch 2: the tiles ----------------------------------------------------------------------------------------------
struct AnnArgs {
  const vali_surface* d_frames;
  const vali_mark* marks;
  const uint8_t* ws;
  float m[3][4];  // rgb2yuv rows (YUV formats)
};
// the coverage atlas of a call that has one (k_annotate<FMT, true>): w x h bytes, rows `pitch` apart; without: all 0
struct StampAtlas {
  const uint8_t* p;
  int pitch, w, h;
};

// FILL and BOX on one piece: lane-local
template <int FMT, int S>
__device__ __forceinline__ void blend_piece(const Piece& pc, const Mark& mk, const u32 (&col)[3], u32 alpha, u32 (&w)[4]) {
  constexpr Slot sl = slot_of(FMT, S);
  constexpr int nc = sl.nc, sh = sl.sh;
  if (pc.n <= 0 || pc.y < (mk.y0 >> sh) || pc.y >= (mk.y1 >> sh))
    return;
  const int lo = (mk.x0 >> sh) * nc - pc.bx, hi = (mk.x1 >> sh) * nc - pc.bx;
  if (lo >= 16 || hi <= 0)
    return;
  const bool inner_row = pc.y >= (mk.iy0 >> sh) && pc.y < (mk.iy1 >> sh);
  const int ilo = inner_row ? (mk.ix0 >> sh) * nc - pc.bx : 0, ihi = inner_row ? (mk.ix1 >> sh) * nc - pc.bx : 0;
  u32 c[3];
  piece_colours<FMT, S>(pc.lbx, col, c);
  const u32 ia = 255u - alpha;
#pragma unroll
  for (int b = 0; b < 16; ++b) {
    const bool inside = b >= lo && b < hi && !(b >= ilo && b < ihi);
    const u32 v = (w[b / 4] >> (8 * (b % 4))) & 0xffu;
    const u32 nv = div255(v * ia + c[b % nc] * alpha + 127u);
    if (inside)
      w[b / 4] = (w[b / 4] & ~(0xffu << (8 * (b % 4)))) | (nv << (8 * (b % 4)));
  }
}

// ---- STAMP: lane-local like FILL, the weight of every sample comes from the atlas --------------------------------------
// the n low bytes of a quad word, n clamped to 0 .. 8
__device__ __forceinline__ unsigned long long low_bytes(int n) {
  return n <= 0 ? 0ull : n >= 8 ? ~0ull : (1ull << (8 * n)) - 1ull;
}

// the 16 bytes (lo, hi) moved by d bytes, |d| < 16, towards the higher bytes (d > 0) or the lower; zeros come in
__device__ __forceinline__ void shift_bytes(unsigned long long& lo, unsigned long long& hi, int d) {
  const u32 n = 8u * (u32)(d < 0 ? -d : d);
  if (d > 0) {
    if (n >= 64u)
      hi = lo << (n - 64u), lo = 0ull;
    else
      hi = hi << n | lo >> (64u - n), lo <<= n;
  } else if (d < 0) {
    if (n >= 64u)
      lo = hi >> (n - 64u), hi = 0ull;
    else
      lo = lo >> n | hi << (64u - n), hi >>= n;
  }
}

// The coverage of the N (16, or 6 for a packed RGB piece) frame pixels X .. X + N - 1 of frame row py, a byte each, zero
// where the stamp has none.  ONE vector load of 16 (N = 6: 8) bytes: the window slides into the atlas row where the
// pixels hang over its ends and the bytes are moved back in registers (labels start at the atlas's column 0, so the
// first piece of every stamp row hangs over).  An atlas narrower than the window is read byte by byte.  No byte outside
// the atlas's area is read either way.  (mk.rx0 .. mk.ry1 end with the atlas.)
template <int N>
__device__ __forceinline__ void load_cov(const StampAtlas& t, const Stamp& mk, int X, int py, u32 (&cv)[N == 16 ? 4 : 2]) {
  constexpr int NW = N == 16 ? 4 : 2;
#pragma unroll
  for (int k = 0; k < NW; ++k)
    cv[k] = 0u;
  const int lo = max(mk.rx0 - X, 0), hi = min(mk.rx1 - X, N);
  if (py < mk.ry0 || py >= mk.ry1 || lo >= hi)
    return;
  const int s = X + mk.ox;  // the atlas column under pixel X: in -N + 1 .. aw - 1, as some pixel has coverage
  const uint8_t* row = t.p + (size_t)(py + mk.oy) * (size_t)t.pitch;
  unsigned long long q0 = 0ull, q1 = 0ull;
  if (t.w >= 4 * NW) {
    const int sw = min(max(s, 0), t.w - 4 * NW);
    if constexpr (N == 16) {
      const v4u32 q = gload_u<v4u32>(row + sw);
      q0 = (unsigned long long)q.x | (unsigned long long)q.y << 32, q1 = (unsigned long long)q.z | (unsigned long long)q.w << 32;
    } else {
      const v2u32 q = gload_u<v2u32>(row + sw);
      q0 = (unsigned long long)q.x | (unsigned long long)q.y << 32;
    }
    shift_bytes(q0, q1, sw - s);
  } else {
    for (int k = lo; k < hi; ++k) {  // (rolled: shifts, not an indexed register array)
      const unsigned long long b = gload<uint8_t>(row + (s + k));
      if (k < 8)
        q0 |= b << (8 * k);
      else
        q1 |= b << (8 * (k - 8));
    }
  }
  q0 &= low_bytes(hi) & ~low_bytes(lo);
  cv[0] = (u32)q0, cv[1] = (u32)(q0 >> 32);
  if constexpr (N == 16) {
    q1 &= low_bytes(hi - 8) & ~low_bytes(lo - 8);
    cv[2] = (u32)q1, cv[3] = (u32)(q1 >> 32);
  }
}

// a STAMP and the atlas as cover_piece's coverage source (tile_paint.hpp)
struct StampCov {
  const StampAtlas& t;
  const Stamp& st;
  int rx0, ry0, rx1, ry1;
  template <int N>
  __device__ __forceinline__ void get(int X, int py, u32 (&cv)[N == 16 ? 4 : 2]) const {
    load_cov<N>(t, st, X, py, cv);
  }
};

// PIXELATE on one piece: ADD =the piece's samples go into the cell sums, !ADD = the cell means come back
template <int FMT, int S, bool ADD>
__device__ __forceinline__ void pixelate_piece(const Piece& pc, const Mark& mk, int lcell, u32* sums, u32 (&w)[4]) {
  constexpr Slot sl = slot_of(FMT, S);
  constexpr int nc = sl.nc, sh = sl.sh;
  if (pc.n <= 0 || pc.y < (mk.y0 >> sh) || pc.y >= (mk.y1 >> sh))
    return;
  const int lo = (mk.x0 >> sh) * nc - pc.bx, hi = (mk.x1 >> sh) * nc - pc.bx;
  if (lo >= 16 || hi <= 0)
    return;
  const int lcs = lcell - sh;                                     // log2 of the cell in this plane's samples
  const int rowkey = ((pc.y & ((kTile >> sh) - 1)) >> lcs) * 16;  // the tile starts on a multiple of its side
  const u32 ch0 = nc == 3 ? (u32)pc.lbx % 3u : 0u;
#pragma unroll
  for (int k = 0; k < nc; ++k) {
    const int ch = nc == 3 ? (int)((ch0 + (u32)k) % 3u) : sl.c0 + k;
    int run = -1;  // the cell whose samples `acc` holds
    u32 acc = 0;
#pragma unroll
    for (int b = k; b < 16; b += nc) {
      if (b >= lo && b < hi) {
        const int cx = (int)((u32)(pc.lbx + b) / (u32)nc) >> lcs;
        u32* cell = sums + ((rowkey + cx) * 3 + ch);
        if constexpr (ADD) {
          if (cx != run) {
            if (run >= 0)
              atomicAdd(sums + ((rowkey + run) * 3 + ch), acc);
            run = cx, acc = 0;
          }
          acc += (w[b / 4] >> (8 * (b % 4))) & 0xffu;
        } else {
          w[b / 4] = (w[b / 4] & ~(0xffu << (8 * (b % 4)))) | (*cell << (8 * (b % 4)));
        }
      }
    }
    if constexpr (ADD)
      if (run >= 0)
        atomicAdd(sums + ((rowkey + run) * 3 + ch), acc);
  }
}

// STAMPS: the call has an atlas.  Without one the kernel holds no stamp path and VALI_MARK_STAMP is an unknown kind.
// The waves per SIMD asked of the register allocator: YUV420 with stamps lands one register above the fourth wave (129)
// and fits it when asked; everything else is left at the default of this workgroup size, one
constexpr int min_waves(int f, bool stamps) { return stamps && f == A_YUV420 ? 4 : 1; }
template <int FMT, bool STAMPS>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(min_waves(FMT, STAMPS), 8)))
k_annotate(const AnnArgs a, const StampAtlas t) {
  __shared__ uint16_t hits[kMaxMarks];
  __shared__ u32 sums[kCells];
  __shared__ int wtot[kWavesPerBlock];
  constexpr int NS = nslots(FMT);
  constexpr bool is420 = a_is420(FMT);
  const int AW = STAMPS ? t.w : 0, AH = STAMPS ? t.h : 0;

  const int f = blockIdx.y;
  const vali_surface* d = a.d_frames + f;
  const int W = d->width, H = d->height;
  if constexpr (STAMPS) {
    // (check_frames: the 64-bit forms of W and H that resolve_mark compares with then need no registers for their high
    // halves, which this instantiation has no scalar registers left for)
    __builtin_assume(W >= 1 && W <= 65535 && H >= 1 && H <= 65535);
  }
  const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
  if ((int)blockIdx.x >= tiles_x * tiles_y)
    return;  // the grid is sized for the batch's largest frame
  const uint8_t* bin = a.ws + (size_t)f * kBinBytes;
  const int count = (int)*(const u32*)bin;
  if (count == 0)
    return;  // no row draws on this frame
  const uint16_t* list = (const uint16_t*)(bin + 16);
  const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
  const int tx0 = tx * kTile, ty0 = ty * kTile;
  const int tid = threadIdx.x;

  // the frame's rows that meet this tile, in row order
  int nh = 0;
  for (int base = 0; base < count; base += kBlock) {
    const int i = base + tid;
    bool flag = false;
    int idx = 0;
    if (i < count) {
      idx = list[i];
      int r[8];
      load_mark(a.marks, idx, r);
      Mark mk;
      flag = resolve_mark(r, W, H, is420, AW, AH, mk) && mark_meets_tile(mk, tx0, ty0, W, H);
    }
    nh = compact_put(flag, idx, hits, nh, wtot);
  }
  if (nh == 0)
    return;

  // the lane's pieces
  Piece pc[NS];
  u32 cur[NS][4], orig[NS][4];
#define VALI_SLOT(S) load_piece<FMT, S>(d, tid, tx0, ty0, W, H, pc[S], cur[S], orig[S]);
  VALI_SLOTS(VALI_SLOT)
#undef VALI_SLOT

  for (int h = 0; h < nh; ++h) {
    const int idx = __builtin_amdgcn_readfirstlane((int)hits[h]);
    int r[8];
    load_mark(a.marks, idx, r);
    Mark mk;
    if (!resolve_mark(r, W, H, is420, AW, AH, mk))
      continue;
    if (mk.kind == VALI_MARK_PIXELATE) {
      const int lcell = 31 - __clz(mk.cell);
      for (int j = tid; j < kCells; j += kBlock)
        sums[j] = 0;
      __syncthreads();
#define VALI_SLOT(S) pixelate_piece<FMT, S, true>(pc[S], mk, lcell, sums, cur[S]);
      VALI_SLOTS(VALI_SLOT)
#undef VALI_SLOT
      __syncthreads();
      // sums -> rounded means over (cell ^ frame); entry j = (cell row * 16 + cell column) * 3 + channel
      for (int j = tid; j < kCells; j += kBlock) {
        const u32 sum = sums[j];
        if (sum) {
          const int ch = j % 3, cell = j / 3, cxl = cell & 15, cyl = cell >> 4;
          const int sh = a_is420(FMT) && ch > 0 ? 1 : 0;
          const int cs = mk.cell >> sh;
          const int px0 = (tx0 >> sh) + cxl * cs, py0 = (ty0 >> sh) + cyl * cs;
          const int cw = min(px0 + cs, W >> sh) - px0, chh = min(py0 + cs, H >> sh) - py0;
          const u32 cnt = (u32)(cw * chh);
          sums[j] = (sum + cnt / 2u) / cnt;  // sum > 0: the cell holds a sample of the frame, cnt >= 1
        }
      }
      __syncthreads();
#define VALI_SLOT(S) pixelate_piece<FMT, S, false>(pc[S], mk, lcell, sums, cur[S]);
      VALI_SLOTS(VALI_SLOT)
#undef VALI_SLOT
      __syncthreads();  // the next pixelate mark clears the sums
    } else {
      const u32 alpha = mk.colour >> 24;
      // (spelled out here and in mask.hip, not a function of tile_paint.hpp: as one, the twelve scalars of a.m are loaded
      // before the hit loop and held through it, 8 to 15 more scalar registers in k_mask_paint's YUV forms)
      const u32 cr = (mk.colour >> 16) & 0xffu, cg = (mk.colour >> 8) & 0xffu, cb = mk.colour & 0xffu;
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
      if (STAMPS && mk.kind == VALI_MARK_STAMP) {
        if constexpr (STAMPS) {
          Stamp sp;
          resolve_stamp(r, W, H, AW, AH, sp);
          const StampCov st = {t, sp, sp.rx0, sp.ry0, sp.rx1, sp.ry1};
#define VALI_SLOT(S) cover_piece<FMT, S>(st, pc[S], col, alpha, cur[S]);
          VALI_SLOTS(VALI_SLOT)
#undef VALI_SLOT
        }
      } else {
#define VALI_SLOT(S) blend_piece<FMT, S>(pc[S], mk, col, alpha, cur[S]);
        VALI_SLOTS(VALI_SLOT)
#undef VALI_SLOT
      }
    }
  }

  // only what a mark changed goes back
#define VALI_SLOT(S) store_piece(pc[S], cur[S], orig[S]);
  VALI_SLOTS(VALI_SLOT)
#undef VALI_SLOT
}
#undef VALI_SLOTS

template <int FMT>
void launch_tiles(const dim3& grid, hipStream_t s, const AnnArgs& a, const StampAtlas& t) {
  if (t.p)
    hipLaunchKernelGGL((k_annotate<FMT, true>), grid, dim3(kBlock), 0, s, a, t);
  else
    hipLaunchKernelGGL((k_annotate<FMT, false>), grid, dim3(kBlock), 0, s, a, t);
}

} // namespace
} // namespace vali

using namespace vali;

extern "C" {

int vali_annotate_workspace_size(int n, const vali_surface* frames, size_t* bytes) {
  VALI_REQUIRE(bytes, "null argument");
  VALI_REQUIRE(n >= 0 && n <= 65535, "n outside 0..65535");
  VALI_REQUIRE(frames || n == 0, "null frames");
  if (n > 0) {
    int tiles = 0;
    const int rc = check_frames(__func__, n, frames, frames[0].format, &tiles);
    if (rc != VALI_OK)
      return rc;
  }
  *bytes = (size_t)n * kBinBytes;
  return VALI_OK;
}

int vali_annotate_batch(const vali_surface* frames, const vali_surface* d_frames, int n, int format,
                        const vali_mark* d_marks, int m, const vali_cvt_params* params, void* workspace,
                        size_t ws_bytes, vali_stream_t stream) {
  return vali_annotate_batch_atlas(frames, d_frames, n, format, d_marks, m, nullptr, params, workspace, ws_bytes, stream);
}

int vali_annotate_batch_atlas(const vali_surface* frames, const vali_surface* d_frames, int n, int format,
                              const vali_mark* d_marks, int m, const vali_surface* atlas, const vali_cvt_params* params,
                              void* workspace, size_t ws_bytes, vali_stream_t stream) {
  VALI_REQUIRE(n >= 0 && n <= 65535, "n outside 0..65535");
  VALI_REQUIRE(m >= 0 && m <= kMaxMarks, "m outside 0..4096");
  VALI_REQUIRE((frames && d_frames) || n == 0, "null frames");
  VALI_REQUIRE(d_marks || m == 0, "null marks");
  VALI_REQUIRE(((uintptr_t)d_marks & 3u) == 0, "marks are not 4-byte aligned");
  int tiles = 0;
  const int rc = check_frames(__func__, n, frames, format, &tiles);
  if (rc != VALI_OK)
    return rc;
  const int fmt = tile_format(format);
  VALI_REQUIRE(params || !a_isyuv(fmt), "a YUV format needs params (rgb2yuv)");
  VALI_REQUIRE(workspace || n == 0, "null workspace");
  VALI_REQUIRE(((uintptr_t)workspace & 15u) == 0, "the workspace is not 16-byte aligned");
  VALI_REQUIRE(ws_bytes >= (size_t)n * kBinBytes, "the workspace is smaller than vali_annotate_workspace_size");
  if (atlas) {
    VALI_REQUIRE(atlas->format == VALI_FMT_Y, "the atlas is not a VALI_FMT_Y surface");
    VALI_REQUIRE(atlas->plane[0], "the atlas has a null plane");
    VALI_REQUIRE(atlas->width >= 1 && atlas->height >= 1 && atlas->width <= 65535 && atlas->height <= 65535,
                 "the atlas's size is outside 1..65535");
    VALI_REQUIRE(atlas->pitch[0] >= atlas->width, "the atlas's pitch is shorter than a row");
  }
  if (n == 0 || m == 0)
    return VALI_OK;

  AnnArgs a = {};
  a.d_frames = d_frames;
  a.marks = d_marks;
  a.ws = (const uint8_t*)workspace;
  if (a_isyuv(fmt))
    for (int k = 0; k < 3; ++k)
      for (int j = 0; j < 4; ++j)
        a.m[k][j] = params->rgb2yuv[k][j];
  StampAtlas t = {};
  if (atlas) {
    t.p = (const uint8_t*)atlas->plane[0];
    t.pitch = atlas->pitch[0], t.w = atlas->width, t.h = atlas->height;
  }

  hipStream_t s = as_stream(stream);
  VALI_ENTRY(s);
  hipLaunchKernelGGL(k_annotate_bin, dim3(n), dim3(kBlock), 0, s, d_frames, d_marks, m, a_is420(fmt) ? 1 : 0, t.w, t.h,
                     (uint8_t*)workspace);
  VALI_LAUNCH_CHECK();
  const dim3 grid(tiles, n);
  with_tile_format(fmt, [&](auto f) { launch_tiles<f>(grid, s, a, t); });
  VALI_LAUNCH_CHECK();
  return VALI_OK;
}

} // extern "C"
