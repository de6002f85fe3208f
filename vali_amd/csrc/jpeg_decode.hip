// Baseline sequential JPEG decoder (include/vali_hip.h, "JPEG: baseline sequential decoder").
//
// DEFINITION = libjpeg-turbo's default decompression; tests/jpeg_decode_model.py restates it and
// tests/test_jpeg_decode_host.py pins the restatement to Pillow byte for byte.
// It is the C path (jidctint.c: the dequantised coefficient is an int, the passes run in JLONG).  Pillow runs the SIMD
// path, which keeps dequantised coefficients and their first sums in 16-bit lanes: the two agree while those stay within
// 16 bits (the q50 tables times 3 still do, times 4 no longer: DESIGN.md section 4) and beyond that this decoder follows
// the C path, not the SIMD one -- 16-bit quantisation values wrap as a short, nothing else narrows.
//
// The entropy decode is serial by nature, and most files have no restart markers.  It runs self-synchronising
// (Weissenberger & Schmidt, ICPP 2018): every restart segment is cut into subsequences of kSubBits bits, a lane
// decodes one subsequence from a guessed state and records the state at which it enters the next one; an entry
// that turns out wrong is replaced by the predecessor's exit and the subsequence decoded again, until nothing
// changes.  Segment starts are exact, so the result is the sequential decode for every stream; a stream that
// synchronises slowly only costs more passes.
//
// Launches in stream order (no workgroup ever waits on another workgroup of its own launch):
//   memset         the coefficient blocks (the decoder writes nonzero coefficients only)
//   k_jd_layout    one workgroup: per-image workspace offsets (exclusive scans over the batch), descriptor checks
//   k_jd_unstuff   workgroup = one image: drop the 00 after every FF, find the RSTn markers (per-chunk counts +
//                  prefix sums) -> unstuffed bytes and the bit where every restart segment starts; then the split
//                  of the segments into subsequences (prefix sum over the segments)
//   k_jd_sync      workgroup = 256 consecutive subsequences of one image, lane = one subsequence: decode, take the
//                  predecessor's exit state, decode again while any entry changed
//   k_jd_seams     workgroup = one image: walks the seams between k_jd_sync workgroups in order and re-decodes
//                  from the exact exit of the previous workgroup until the trajectory meets the recorded one; the
//                  number of blocks of its segment in front of each workgroup
//   k_jd_write     as k_jd_sync: block offsets (segmented scan of the counts) and one more decode from the exact
//                  entry states, writing int16 coefficients (natural order, DC as a difference); corrupt data fails
//   k_jd_dc        workgroup = one image: prefix sum of the DC differences per component, reset at every restart
//   k_jd_idct      lane = one 8x8 block: dequantise, islow IDCT, range limit; raw formats write the surface,
//                  RGB formats the MCU-padded component planes in the workspace
//   k_jd_color     RGB formats only: fancy upsampling + ycc_rgb_convert into RGB / BGR / RGB_PLANAR
#include <algorithm>
#include <cstring>

#include "common.hpp"

namespace vali {
namespace {

typedef uint32_t u32;
typedef uint64_t u64;
typedef uint8_t u8;

constexpr int kSubBits = 1024;  // bits per subsequence
constexpr int kGroup = 256;     // subsequences per workgroup of k_jd_sync / k_jd_write
constexpr u64 kMaxData = 1ull << 28;  // bytes of entropy data per file: bit positions stay 32-bit

// natural index of zigzag position k
constexpr int kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
__constant__ u8 d_natural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

__host__ __device__ inline u64 align256(u64 v) { return (v + 255) & ~(u64)255; }

// ---- geometry: one formula for the parser, the host's sizing and the device's checks ----------------------------------
__host__ __device__ inline bool sampling_ok(int H, int V) { return H >= 1 && H <= 2 && V >= 1 && V <= 2; }

// the fields vali_jpeg_parse derives from width, height, components, sampling and restart interval
__host__ __device__ inline bool info_consistent(const vali_jpeg_info& f) {
  if (f.width < 1 || f.height < 1 || f.width > 65535 || f.height > 65535)
    return false;
  if (f.components == 1) {
    if (f.h_samp != 1 || f.v_samp != 1 || f.blocks_per_mcu != 1)
      return false;
  } else if (f.components != 3 || !sampling_ok(f.h_samp, f.v_samp) ||
             f.blocks_per_mcu != f.h_samp * f.v_samp + 2) {
    return false;
  }
  if (f.mcux != (f.width + 8 * f.h_samp - 1) / (8 * f.h_samp) || f.mcuy != (f.height + 8 * f.v_samp - 1) / (8 * f.v_samp))
    return false;
  const long long mcus = (long long)f.mcux * f.mcuy;
  if (f.restart_interval < 0 || f.restart_interval > 65535)
    return false;
  const long long segs = f.restart_interval ? (mcus + f.restart_interval - 1) / f.restart_interval : 1;
  return f.segments == segs && f.data_len < kMaxData;
}

// workspace of one image
struct ImgSize {
  u64 unst;    // unstuffed bytes: a multiple of 16, with 16 spare bytes for the 64-bit bit reader
  u64 blocks;  // coefficient blocks (= bytes of MCU-padded component planes / 64)
  u32 segs;    // segment entries: segments + 1
  u32 subs;    // subsequence slots, a multiple of kGroup
};

__host__ __device__ inline ImgSize img_size(const vali_jpeg_info& f) {
  ImgSize s;
  s.unst = ((u64)f.data_len + 16 + 15) & ~(u64)15;
  s.blocks = (u64)f.mcux * f.mcuy * f.blocks_per_mcu;
  s.segs = (u32)f.segments + 1;
  // sum over segments of max(1, ceil(bits / kSubBits)) <= all bits / kSubBits + segments
  const u64 subs = ((u64)f.data_len * 8 + kSubBits - 1) / kSubBits + (u64)f.segments;
  s.subs = (u32)((subs + kGroup - 1) / kGroup * kGroup);
  return s;
}

struct Totals {
  u64 unst, blocks, segs, subs, gsegs;
};

// per-image offsets, written by k_jd_layout into the workspace
struct Lay {
  u64 unst;  // byte offset of the unstuffed data
  u64 blk;   // first coefficient block (its component planes start at byte blk * 64 of the plane area)
  u32 seg;   // first segment entry
  u32 sub;   // first subsequence slot (a multiple of kGroup)
  u32 gseg;  // first global segment (a check of the totals)
  u32 pad;
};

struct WsMap {
  u64 lay, flag, unst, seg_start, seg_sub, ent_p, ent_ck, ext_p, ext_ck, cnt, head, tail, coef, plane, total;
};

WsMap ws_map(const Totals& t, int n) {
  WsMap m;
  u64 o = 0;
  auto take = [&](u64 bytes) {
    const u64 at = o;
    o += align256(bytes);
    return at;
  };
  m.lay = take((u64)(n > 0 ? n : 1) * sizeof(Lay));
  m.flag = take(4);
  m.unst = take(t.unst);
  m.seg_start = take(t.segs * 4);
  m.seg_sub = take(t.segs * 4);
  m.ent_p = take(t.subs * 4);
  m.ent_ck = take(t.subs * 4);
  m.ext_p = take(t.subs * 4);
  m.ext_ck = take(t.subs * 4);
  m.cnt = take(t.subs * 4);
  m.head = take(t.subs / kGroup * 4);
  m.tail = take(t.subs / kGroup * 4);
  m.coef = take(t.blocks * 128);
  m.plane = take(t.blocks * 64);
  m.total = o;
  return m;
}

// ---- kernel arguments ------------------------------------------------------------------------------------------------------
struct Args {
  const vali_jpeg_info* info;
  const u8* data;
  const vali_surface* dst;
  int32_t* status;
  Lay* lay;
  u32* flag;  // 1: the device infos do not give the host's totals; nothing is decoded
  u8* unst;
  u32 *seg_start, *seg_sub;
  u32 *ent_p, *ent_ck, *ext_p, *ext_ck, *cnt;
  u32 *head, *tail;
  int16_t* coef;
  u8* plane;
  Totals tot;
  int n, format;
};

enum { ST_OK = 0, ST_CORRUPT = 1, ST_BAD_DESC = 2, ST_BAD_INFO = 3 };

// largest i in [0, n) with key(lay[i]) <= v (lay[0] starts at 0)
template <class K>
__device__ inline int find_img(const Lay* lay, int n, u64 v, K key) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (key(lay[mid]) <= v)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// exclusive scan over a workgroup of NW waves; *total = the sum of all lanes
template <int NW, class T>
__device__ inline T wg_excl_scan(T v, T* s_w, T* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = __shfl_up(incl, d, 64);
    if (lane >= d)
      incl += o;
  }
  if (lane == 63)
    s_w[w] = incl;
  __syncthreads();
  T before = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    const T x = s_w[k];
    before += k < w ? x : (T)0;
    tot += x;
  }
  __syncthreads();
  *total = tot;
  return before + incl - v;
}

// ---- k_jd_layout ---------------------------------------------------------------------------------------------------------
__device__ inline bool desc_ok(const vali_surface& d, const vali_jpeg_info& f, int format) {
  if (d.width != f.width || d.height != f.height || d.format != format || !d.plane[0] || d.pitch[0] <= 0)
    return false;
  if (format == VALI_FMT_RGB_PLANAR || format == VALI_FMT_YUV444 || format == VALI_FMT_YUV422 ||
      format == VALI_FMT_YUV420)
    return d.plane[1] && d.plane[2] && d.pitch[1] > 0 && d.pitch[2] > 0;
  if (format == VALI_FMT_NV12)
    return d.plane[1] && d.pitch[1] > 0;
  return true;
}

__global__ void __launch_bounds__(256) k_jd_layout(const Args a) {
  __shared__ u64 s_w[4];
  u64 c_unst = 0, c_blk = 0, c_seg = 0, c_sub = 0, c_gseg = 0;
  for (int i0 = 0; i0 < a.n; i0 += 256) {
    const int i = i0 + (int)threadIdx.x;
    ImgSize s = {0, 0, 0, 0};
    u64 nseg = 0;
    int st = ST_OK;
    if (i < a.n) {
      const vali_jpeg_info& f = a.info[i];
      if (!info_consistent(f)) {
        st = ST_BAD_INFO;  // sizes of 0: the image takes no room and is never decoded
      } else {
        s = img_size(f);
        nseg = (u64)f.segments;
        if (!desc_ok(a.dst[i], f, a.format))
          st = ST_BAD_DESC;
      }
    }
    u64 t_unst, t_blk, t_seg, t_sub, t_gseg;
    const u64 e_unst = wg_excl_scan<4, u64>(s.unst, s_w, &t_unst);
    const u64 e_blk = wg_excl_scan<4, u64>(s.blocks, s_w, &t_blk);
    const u64 e_seg = wg_excl_scan<4, u64>((u64)s.segs, s_w, &t_seg);
    const u64 e_sub = wg_excl_scan<4, u64>((u64)s.subs, s_w, &t_sub);
    const u64 e_gseg = wg_excl_scan<4, u64>(nseg, s_w, &t_gseg);
    if (i < a.n) {
      Lay l;
      l.unst = c_unst + e_unst;
      l.blk = c_blk + e_blk;
      l.seg = (u32)(c_seg + e_seg);
      l.sub = (u32)(c_sub + e_sub);
      l.gseg = (u32)(c_gseg + e_gseg);
      l.pad = 0;
      a.lay[i] = l;
      a.status[i] = st;
    }
    c_unst += t_unst, c_blk += t_blk, c_seg += t_seg, c_sub += t_sub, c_gseg += t_gseg;
  }
  if (threadIdx.x == 0)
    *a.flag = (c_unst != a.tot.unst || c_blk != a.tot.blocks || c_seg != a.tot.segs || c_sub != a.tot.subs ||
               c_gseg != a.tot.gsegs)
                  ? 1u
                  : 0u;
}

// ---- k_jd_unstuff --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) k_jd_unstuff(const Args a) {
  __shared__ u32 s_w[16];
  __shared__ int s_bad;
  const int img = blockIdx.x;
  if (*a.flag || a.status[img] != ST_OK)
    return;
  const vali_jpeg_info& f = a.info[img];
  const Lay L = a.lay[img];
  const u8* src = a.data + f.data_offset;
  const u64 len = f.data_len;
  const int nseg = f.segments;
  u8* out = a.unst + L.unst;
  u32* seg_start = a.seg_start + L.seg;
  if (threadIdx.x == 0)
    s_bad = 0;
  __syncthreads();
  bool bad = false;
  u32 kept_carry = 0, mark_carry = 0;
  for (u64 b0 = 0; b0 < len; b0 += 4096) {
    const u64 i = b0 + 4 * threadIdx.x;
    u32 keep = 0, mark = 0;  // 4-bit masks of this lane's bytes
    u8 byte[4], nxt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const u64 x = i + j;
      byte[j] = nxt[j] = 0;
      if (x >= len)
        continue;
      byte[j] = src[x];
      const bool after_ff = x > 0 && src[x - 1] == 0xFF;  // a stuffed 00 or an RST id: checked at its FF
      if (after_ff)
        continue;
      if (byte[j] != 0xFF) {
        keep |= 1u << j;
        continue;
      }
      if (x + 1 >= len) {
        bad = true;  // FF as the last byte
        continue;
      }
      nxt[j] = src[x + 1];
      if (nxt[j] == 0x00)
        keep |= 1u << j;
      else if (nxt[j] >= 0xD0 && nxt[j] <= 0xD7)
        mark |= 1u << j;
      else
        bad = true;
    }
    const u32 packed = (u32)__popc(keep) | ((u32)__popc(mark) << 16);
    u32 tot;
    const u32 pre = wg_excl_scan<16, u32>(packed, s_w, &tot);
    u32 k = kept_carry + (pre & 0xFFFF), m = mark_carry + (pre >> 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (keep & (1u << j))
        out[k++] = byte[j];
      if (mark & (1u << j)) {
        if ((u32)(nxt[j] & 7) != (m & 7) || (int)m + 1 >= nseg)
          bad = true;  // out of order, or more markers than segments
        else
          seg_start[m + 1] = k * 8;
        ++m;
      }
    }
    kept_carry += tot & 0xFFFF;
    mark_carry += tot >> 16;
  }
  if (bad)
    s_bad = 1;
  // 16 zero bytes after the data: the bit reader's last word
  if (threadIdx.x < 16)
    out[kept_carry + threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    seg_start[0] = 0;
    seg_start[nseg] = kept_carry * 8;
  }
  __syncthreads();
  if (s_bad || mark_carry != (u32)(nseg - 1)) {
    if (threadIdx.x == 0)
      a.status[img] = ST_CORRUPT;
    return;
  }
  // subsequences of every segment: max(1, ceil(bits / kSubBits)), prefix-summed
  u32* seg_sub = a.seg_sub + L.seg;
  u32 carry = 0;
  for (int s0 = 0; s0 < nseg; s0 += 1024) {
    const int s = s0 + (int)threadIdx.x;
    u32 cnt = 0;
    if (s < nseg) {
      const u32 bits = seg_start[s + 1] - seg_start[s];
      cnt = bits ? (bits + kSubBits - 1) / kSubBits : 1u;
    }
    u32 tot;
    const u32 pre = wg_excl_scan<16, u32>(cnt, s_w, &tot);
    if (s < nseg)
      seg_sub[s] = carry + pre;
    carry += tot;
  }
  if (threadIdx.x == 0)
    seg_sub[nseg] = carry;
}

// ---- entropy decoding ------------------------------------------------------------------------------------------------------
// Words of the unstuffed stream a decode of one subsequence can touch: it starts at a code word at or after the
// subsequence's first bit, and its last code word starts before the end and reads at most 32 bits.
constexpr int kWin = kSubBits / 32 + 2;

// the kWin words from word `first` on, as peek32 reads them (indices clamped to the image's slot), into LDS
__device__ inline void load_window(const u32* words, u32 last_word, u32 first, u32* win, int lane, int lanes) {
  for (int k = lane; k < kWin; k += lanes)
    win[k] = words[min(first + (u32)k, last_word)];
}

// 32 bits of the unstuffed stream from bit p (big-endian).  Word reads are clamped to the image's slot; `words`
// holds the stream from word `first` on, and reads are clamped to its kWin words when `windowed`
__device__ inline u32 peek32(const u32* words, u32 last_word, u32 first, bool windowed, u32 p) {
  u32 wi = min(p >> 5, last_word - 1);
  if (windowed)
    wi = min(max(wi, first), first + (u32)kWin - 2) - first;
  const u64 x = ((u64)__builtin_bswap32(words[wi]) << 32) | __builtin_bswap32(words[wi + 1]);
  return (u32)((x << (p & 31)) >> 32);
}

// one Huffman symbol from the top bits of w: its length (0 = no code matches) and *sym
__device__ inline int huff_sym(const vali_jpeg_huff& t, u32 w, int* sym) {
  const u32 e = t.look[w >> 23];
  if (e) {
    *sym = (int)(e & 255);
    return (int)(e >> 8);
  }
  for (int l = 10; l <= 16; ++l) {
    const int code = (int)(w >> (32 - l));
    if (code <= t.maxcode[l]) {
      *sym = t.vals[(code + t.valoff[l]) & 255];
      return l;
    }
  }
  return 0;
}

struct Dec {
  const u32* words;  // the image's unstuffed words, or an LDS window of them from word `first` on
  u32 last_word;
  u32 first;
  bool windowed;
  const vali_jpeg_huff* tab;  // dc[0..2], ac[0..2]
  int HV, bpm;
};

// Decodes the code words that start in [p, end): WRITE = false for synchronisation (nothing written, corrupt data
// resolved deterministically); WRITE = true from an exact state: nonzero coefficients of block `blk` onward into
// coef, stops after block segblocks - 1, sets *err on corrupt data.  Returns the blocks completed.
template <bool WRITE>
__device__ int decode_run(const Dec& d, u32& p, int& c, int& k, u32 end, int16_t* coef, int blk, int segblocks,
                          u32 seg_end, bool* err) {
  int done = 0;
  while (p < end) {
    if (WRITE && blk >= segblocks)
      break;
    const u32 w = peek32(d.words, d.last_word, d.first, d.windowed, p);
    const int comp = c < d.HV ? 0 : c - d.HV + 1;
    int sym = 0;
    int len = huff_sym(d.tab[k == 0 ? comp : 3 + comp], w, &sym);
    bool bad = len == 0;
    if (bad)
      len = 16, sym = 0;  // synchronisation: a DC difference of 0, or an EOB
    const int r = k == 0 ? 0 : sym >> 4;
    const int sz = k == 0 ? sym : sym & 15;
    int v = 0;
    if (sz) {
      const u32 e = (w << len) >> (32 - sz);
      v = e < (1u << (sz - 1)) ? (int)e - (1 << sz) + 1 : (int)e;
    }
    int nk;
    if (k == 0) {
      if (WRITE && !bad)
        coef[(size_t)blk * 64] = (int16_t)v;
      nk = 1;
    } else if (sz) {
      if (k + r > 63) {
        bad = true;
        nk = 64;
      } else {
        if (WRITE && !bad)
          coef[(size_t)blk * 64 + d_natural[k + r]] = (int16_t)v;
        nk = k + r + 1;
      }
    } else if (r == 15) {
      if (k + 16 > 64)
        bad = true;
      nk = min(k + 16, 64);
    } else {
      nk = 64;  // EOB
    }
    const u32 used = (u32)(len + sz);
    if (WRITE && (bad || p + used > seg_end)) {
      *err = true;
      break;
    }
    p += used;
    k = nk;
    if (k == 64) {
      k = 0;
      c = c + 1 == d.bpm ? 0 : c + 1;
      ++done;
      ++blk;
    }
  }
  return done;
}

// where subsequence js (image-local) of an image lies
struct Sub {
  int s;         // segment
  u32 t;         // index in the segment
  u32 start, end, seg_end;
};

__device__ inline Sub locate(const u32* seg_start, const u32* seg_sub, int nseg, u32 js) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg_sub[mid] <= js)
      lo = mid;
    else
      hi = mid - 1;
  }
  Sub r;
  r.s = lo;
  r.t = js - seg_sub[lo];
  r.seg_end = seg_start[lo + 1];
  r.start = seg_start[lo] + r.t * kSubBits;
  r.end = min(r.start + kSubBits, r.seg_end);
  return r;
}

// shared set-up of k_jd_sync / k_jd_write: the image of this workgroup and its tables in LDS
struct GroupCtx {
  int img;
  Lay L;
  int nseg;
  u32 nsub;
  Dec d;
};

__device__ inline bool group_setup(const Args& a, vali_jpeg_huff* s_tab, GroupCtx* g) {
  const u32 first = blockIdx.x * kGroup;
  g->img = find_img(a.lay, a.n, first, [](const Lay& l) { return (u64)l.sub; });
  if (*a.flag || a.status[g->img] != ST_OK)
    return false;
  const vali_jpeg_info& f = a.info[g->img];
  g->L = a.lay[g->img];
  g->nseg = f.segments;
  g->nsub = a.seg_sub[g->L.seg + g->nseg];
  if (first - g->L.sub >= g->nsub)
    return false;
  const u32* src = (const u32*)&f.dc[0];
  u32* dst = (u32*)s_tab;
  for (int i = threadIdx.x; i < (int)(6 * sizeof(vali_jpeg_huff) / 4); i += blockDim.x)
    dst[i] = src[i];
  g->d.words = (const u32*)(a.unst + g->L.unst);
  g->d.last_word = (u32)(img_size(f).unst / 4 - 1);
  g->d.first = 0;
  g->d.windowed = false;
  g->d.tab = s_tab;
  g->d.HV = f.components == 1 ? 1 : f.h_samp * f.v_samp;
  g->d.bpm = f.blocks_per_mcu;
  __syncthreads();
  return true;
}

__global__ void __launch_bounds__(256) k_jd_sync(const Args a) {
  __shared__ vali_jpeg_huff s_tab[6];
  __shared__ u32 s_p[kGroup], s_ck[kGroup], s_tail;
  __shared__ u32 s_win[kGroup * kWin];
  __shared__ int s_last;
  GroupCtx g;
  if (!group_setup(a, s_tab, &g))
    return;
  const int tid = threadIdx.x;
  const u32 js = blockIdx.x * kGroup - g.L.sub + tid;
  const bool act = js < g.nsub;
  const u32* seg_start = a.seg_start + g.L.seg;
  const u32* seg_sub = a.seg_sub + g.L.seg;
  Sub sb = {};
  if (act) {
    sb = locate(seg_start, seg_sub, g.nseg, js);
    load_window(g.d.words, g.d.last_word, sb.start >> 5, s_win + tid * kWin, 0, 1);
    g.d.words = s_win + tid * kWin;
    g.d.first = sb.start >> 5;
    g.d.windowed = true;
  }
  u32 ep = sb.start, eck = 0;  // entry state: a segment start is exact, anything else a guess
  u32 p = ep;
  int c = 0, k = 0, cnt = 0;
  if (act)
    cnt = decode_run<false>(g.d, p, c, k, sb.end, nullptr, 0, 0, 0, nullptr);
  for (;;) {
    s_p[tid] = p;
    s_ck[tid] = ((u32)c << 8) | (u32)k;
    __syncthreads();
    bool changed = false;
    if (act && sb.t > 0 && tid > 0) {
      const u32 np = s_p[tid - 1], nck = s_ck[tid - 1];
      if (np != ep || nck != eck) {
        ep = np, eck = nck;
        p = ep, c = (int)(eck >> 8), k = (int)(eck & 255);
        cnt = decode_run<false>(g.d, p, c, k, sb.end, nullptr, 0, 0, 0, nullptr);
        changed = true;
      }
    }
    if (!__syncthreads_or(changed))
      break;
  }
  const size_t j = (size_t)blockIdx.x * kGroup + tid;
  if (act) {
    a.ent_p[j] = ep, a.ent_ck[j] = eck;
    a.ext_p[j] = p, a.ext_ck[j] = ((u32)c << 8) | (u32)k;
    a.cnt[j] = (u32)cnt;
  }
  // blocks completed by the last segment of this workgroup (k_jd_seams continues from them)
  if (tid == 0) {
    s_tail = 0;
    s_last = locate(seg_start, seg_sub, g.nseg, min(g.nsub, blockIdx.x * kGroup - g.L.sub + kGroup) - 1).s;
  }
  __syncthreads();
  if (act && sb.s == s_last)
    atomicAdd(&s_tail, (u32)cnt);
  __syncthreads();
  if (tid == 0) {
    a.tail[blockIdx.x] = s_tail;
    a.head[blockIdx.x] = 0;
  }
}

// ---- k_jd_seams ------------------------------------------------------------------------------------------------------------
// Workgroup = one image.  Its seams (the first subsequence of a k_jd_sync workgroup that does not start a segment)
// are resolved in order: lane 0 re-decodes from the exact exit of the previous subsequence until the trajectory
// meets the recorded entry of the next one; the other lanes stage each subsequence's words in LDS.  A seam's
// result is final before the next seam reads it, so the walk is exact however slowly a stream synchronises.
__global__ void __launch_bounds__(64) k_jd_seams(const Args a) {
  __shared__ vali_jpeg_huff s_tab[6];
  __shared__ u32 s_win[kWin];
  __shared__ u32 s_first;
  __shared__ int s_go;
  const int img = blockIdx.x, lane = threadIdx.x;
  if (*a.flag || a.status[img] != ST_OK)
    return;
  const vali_jpeg_info& f = a.info[img];
  const Lay L = a.lay[img];
  const u32* seg_start = a.seg_start + L.seg;
  const u32* seg_sub = a.seg_sub + L.seg;
  const int nseg = f.segments;
  const u32 nsub = seg_sub[nseg];
  const u32 ngroups = (nsub + kGroup - 1) / kGroup;
  {
    const u32* src = (const u32*)&f.dc[0];
    u32* dst = (u32*)s_tab;
    for (int i = lane; i < (int)(6 * sizeof(vali_jpeg_huff) / 4); i += 64)
      dst[i] = src[i];
  }
  const u32* gwords = (const u32*)(a.unst + L.unst);
  Dec d;
  d.words = s_win;
  d.last_word = (u32)(img_size(f).unst / 4 - 1);
  d.first = 0;
  d.windowed = true;
  d.tab = s_tab;
  d.HV = f.components == 1 ? 1 : f.h_samp * f.v_samp;
  d.bpm = f.blocks_per_mcu;
  __syncthreads();
  // lane 0's state across the walk
  u32 xp = 0, xck = 0, j = 0, jend = 0, end = 0;
  int delta = 0, s = 0;
  bool tail_is_s = false;
  for (u32 gw = 1; gw < ngroups; ++gw) {
    const u32 w = L.sub / kGroup + gw;  // global workgroup index of k_jd_sync
    if (lane == 0) {
      const u32 jl = gw * kGroup;
      const Sub sb = locate(seg_start, seg_sub, nseg, jl);
      s_go = sb.t > 0;
      if (sb.t > 0) {
        s = sb.s;
        const int s_prev = locate(seg_start, seg_sub, nseg, jl - kGroup).s;
        a.head[w] = (s_prev == s ? a.head[w - 1] : 0u) + a.tail[w - 1];
        xp = a.ext_p[L.sub + jl - 1], xck = a.ext_ck[L.sub + jl - 1];
        j = jl;
        jend = min(min(seg_sub[s + 1], nsub), jl + kGroup) - 1;
        tail_is_s = locate(seg_start, seg_sub, nseg, min(nsub, jl + kGroup) - 1).s == s;
        delta = 0;
      }
    }
    __syncthreads();
    while (s_go) {
      if (lane == 0) {
        if (j > jend || (a.ent_p[L.sub + j] == xp && a.ent_ck[L.sub + j] == xck)) {
          s_go = 0;  // the trajectory meets the recorded one: the rest of the workgroup is exact
          if (tail_is_s)
            a.tail[w] = (u32)((int)a.tail[w] + delta);
        } else {
          const u32 start = seg_start[s] + (j - seg_sub[s]) * kSubBits;
          end = min(start + kSubBits, seg_start[s + 1]);
          s_first = start >> 5;
        }
      }
      __syncthreads();
      if (!s_go)
        break;
      load_window(gwords, d.last_word, s_first, s_win, lane, 64);
      __syncthreads();
      if (lane == 0) {
        d.first = s_first;
        const size_t g = L.sub + j;
        a.ent_p[g] = xp, a.ent_ck[g] = xck;
        u32 p = xp;
        int c = (int)(xck >> 8), k = (int)(xck & 255);
        const int cnt = decode_run<false>(d, p, c, k, end, nullptr, 0, 0, 0, nullptr);
        delta += cnt - (int)a.cnt[g];
        a.cnt[g] = (u32)cnt;
        xp = p, xck = ((u32)c << 8) | (u32)k;
        a.ext_p[g] = xp, a.ext_ck[g] = xck;
        ++j;
      }
      __syncthreads();
    }
  }
}

// ---- k_jd_write ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_jd_write(const Args a) {
  __shared__ vali_jpeg_huff s_tab[6];
  __shared__ u32 s_sum[kGroup], s_run[kGroup];
  __shared__ u32 s_win[kGroup * kWin];
  __shared__ int s_err;
  GroupCtx g;
  if (!group_setup(a, s_tab, &g))
    return;
  const int tid = threadIdx.x;
  const u32 js = blockIdx.x * kGroup - g.L.sub + tid;
  const bool act = js < g.nsub;
  const u32* seg_start = a.seg_start + g.L.seg;
  const u32* seg_sub = a.seg_sub + g.L.seg;
  Sub sb = {};
  sb.s = -1 - tid;  // inactive lanes: a segment of their own
  if (act) {
    sb = locate(seg_start, seg_sub, g.nseg, js);
    load_window(g.d.words, g.d.last_word, sb.start >> 5, s_win + tid * kWin, 0, 1);
    g.d.words = s_win + tid * kWin;
    g.d.first = sb.start >> 5;
    g.d.windowed = true;
  }
  const size_t j = (size_t)blockIdx.x * kGroup + tid;
  const u32 mine = act ? a.cnt[j] : 0u;
  // segmented exclusive scan of the block counts: lanes of one segment are contiguous
  s_run[tid] = (u32)sb.s;
  if (tid == 0)
    s_err = 0;
  __syncthreads();
  const bool head_lane = tid == 0 || s_run[tid - 1] != (u32)sb.s;
  const int seg0 = (int)s_run[0];
  __syncthreads();
  s_sum[tid] = mine;
  s_run[tid] = head_lane ? (u32)tid : 0u;
  __syncthreads();
  for (int dd = 1; dd < kGroup; dd <<= 1) {
    const u32 o = tid >= dd ? s_sum[tid - dd] : 0u;
    const u32 r = tid >= dd ? s_run[tid - dd] : 0u;
    __syncthreads();
    s_sum[tid] += o;
    s_run[tid] = max(s_run[tid], r);
    __syncthreads();
  }
  const u32 run0 = s_run[tid];
  const u32 pre = s_sum[tid] - mine - (run0 > 0 ? s_sum[run0 - 1] : 0u);
  if (act) {
    const vali_jpeg_info& f = a.info[g.img];
    const long long mcus = (long long)f.mcux * f.mcuy;
    const int R = f.restart_interval ? f.restart_interval : (int)mcus;
    const long long segcap = (long long)R * f.blocks_per_mcu;
    const long long nblocks = mcus * f.blocks_per_mcu;
    const int segblocks = (int)min(segcap, nblocks - segcap * sb.s);
    const int blk0 = (int)(pre + (sb.s == seg0 ? a.head[blockIdx.x] : 0u));
    int16_t* coef = a.coef + (g.L.blk + (u64)(segcap * sb.s)) * 64;
    u32 p = a.ent_p[j];
    const u32 eck = a.ent_ck[j];
    int c = (int)(eck >> 8), k = (int)(eck & 255);
    bool err = false;
    int blk = blk0;
    if (blk < segblocks) {
      blk += decode_run<true>(g.d, p, c, k, sb.end, coef, blk, segblocks, sb.seg_end, &err);
      // the last subsequence of a segment must have completed its last block
      if (!err && js + 1 == seg_sub[sb.s + 1] && blk < segblocks)
        err = true;
    }
    if (err)
      s_err = 1;
  }
  __syncthreads();
  if (tid == 0 && s_err)
    a.status[g.img] = ST_CORRUPT;
}

// ---- k_jd_dc -------------------------------------------------------------------------------------------------------------
// inclusive segmented scan over the workgroup: a set flag starts a new sum at its lane
__device__ inline int seg_scan(int v, bool f, int* s_v, int* s_f, bool* any) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int fi = f ? 1 : 0;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int ov = __shfl_up(v, d, 64), of = __shfl_up(fi, d, 64);
    if (lane >= d) {
      if (!fi)
        v += ov;
      fi |= of;
    }
  }
  if (lane == 63)
    s_v[w] = v, s_f[w] = fi;
  __syncthreads();
  int pv = 0, pf = 0;
  for (int k = 0; k < w; ++k) {
    pv = s_f[k] ? s_v[k] : pv + s_v[k];
    pf |= s_f[k];
  }
  __syncthreads();
  if (!fi)
    v += pv;
  *any = (fi | pf) != 0;
  return v;
}

__global__ void __launch_bounds__(1024) k_jd_dc(const Args a) {
  __shared__ int s_v[16], s_f[16], s_carry[3];
  const int img = blockIdx.x;
  if (*a.flag || a.status[img] != ST_OK)
    return;
  const vali_jpeg_info& f = a.info[img];
  const Lay L = a.lay[img];
  const long long mcus = (long long)f.mcux * f.mcuy;
  const long long segcap = (long long)(f.restart_interval ? f.restart_interval : mcus) * f.blocks_per_mcu;
  const long long nblocks = mcus * f.blocks_per_mcu;
  const int HV = f.components == 1 ? 1 : f.h_samp * f.v_samp, bpm = f.blocks_per_mcu;
  int16_t* coef = a.coef + L.blk * 64;
  int carry[3] = {0, 0, 0};
  for (long long b0 = 0; b0 < nblocks; b0 += 1024) {
    const long long b = b0 + threadIdx.x;
    const bool act = b < nblocks;
    const int pos = (int)(b % bpm);
    const int comp = pos < HV ? 0 : pos - HV + 1;
    const int diff = act ? coef[b * 64] : 0;
    const bool reset = act && b % segcap == 0;
    int mine = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      bool any;
      int v = seg_scan(act && comp == c ? diff : 0, reset, s_v, s_f, &any);
      if (!any)
        v += carry[c];
      if (comp == c)
        mine = v;
      if (threadIdx.x == 1023)
        s_carry[c] = v;
    }
    if (act)
      coef[b * 64] = (int16_t)mine;  // libjpeg keeps the int predictor and stores the JCOEF cast
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c)
      carry[c] = s_carry[c];
    __syncthreads();
  }
}

// ---- k_jd_idct -----------------------------------------------------------------------------------------------------------
// jidctint with JLONG arithmetic; pass 1 (columns) keeps PASS1_BITS = 2 extra bits in an int workspace
constexpr long long F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633,
                    F1501 = 12299, F1847 = 15137, F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;

template <int SH>
__device__ inline void idct_1d(const long long* in, long long* out) {
  long long z2 = in[2], z3 = in[6];
  long long z1 = (z2 + z3) * F0541;
  const long long tmp2 = z1 + z3 * -F1847, tmp3 = z1 + z2 * F0765;
  const long long tmp0 = (in[0] + in[4]) << 13, tmp1 = (in[0] - in[4]) << 13;
  const long long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  long long t0 = in[7], t1 = in[5], t2 = in[3], t3 = in[1];
  z1 = t0 + t3;
  z2 = t1 + t2;
  z3 = t0 + t2;
  long long z4 = t1 + t3;
  const long long z5 = (z3 + z4) * F1175;
  t0 *= F0298, t1 *= F2053, t2 *= F3072, t3 *= F1501;
  z1 *= -F0899, z2 *= -F2562, z3 *= -F1961, z4 *= -F0390;
  z3 += z5, z4 += z5;
  t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
  constexpr long long half = 1ll << (SH - 1);
  out[0] = (tmp10 + t3 + half) >> SH;
  out[7] = (tmp10 - t3 + half) >> SH;
  out[1] = (tmp11 + t2 + half) >> SH;
  out[6] = (tmp11 - t2 + half) >> SH;
  out[2] = (tmp12 + t1 + half) >> SH;
  out[5] = (tmp12 - t1 + half) >> SH;
  out[3] = (tmp13 + t0 + half) >> SH;
  out[4] = (tmp13 - t0 + half) >> SH;
}

// jdmaster's post-IDCT range-limit table, indexed by (x & 1023)
__device__ inline u8 range_limit(int x) {
  const int u = x & 1023;
  return (u8)(u < 128 ? u + 128 : u < 512 ? 255 : u < 896 ? 0 : u - 896);
}

__global__ void __launch_bounds__(256) k_jd_idct(const Args a) {
  const u64 gb = (u64)blockIdx.x * 256 + threadIdx.x;
  if (gb >= a.tot.blocks || *a.flag)
    return;
  const int img = find_img(a.lay, a.n, gb, [](const Lay& l) { return l.blk; });
  if (a.status[img] != ST_OK)
    return;
  const vali_jpeg_info& f = a.info[img];
  const Lay L = a.lay[img];
  const u64 b = gb - L.blk;
  const int bpm = f.blocks_per_mcu;
  const int H = f.h_samp, V = f.v_samp, HV = f.components == 1 ? 1 : H * V;
  const u64 m = b / bpm;
  const int pos = (int)(b - m * bpm);
  const int mx = (int)(m % f.mcux), my = (int)(m / f.mcux);
  const int comp = pos < HV ? 0 : pos - HV + 1;
  const int hs = comp ? 1 : H, vs = comp ? 1 : V;
  const int bx = comp ? mx : mx * H + pos % H, by = comp ? my : my * V + pos / H;
  const int cw = (f.width * hs + H - 1) / H, ch = (f.height * vs + V - 1) / V;
  const int fmt = a.format;
  const bool raw = fmt == VALI_FMT_Y || fmt == VALI_FMT_YUV444 || fmt == VALI_FMT_YUV422 || fmt == VALI_FMT_YUV420 ||
                   fmt == VALI_FMT_NV12;
  if (raw && (comp > 0 && fmt == VALI_FMT_Y))
    return;
  if (raw && (bx * 8 >= cw || by * 8 >= ch))
    return;

  const int16_t* src = a.coef + gb * 64;
  int ws[64];  // dequantised coefficients, then jidctint's int workspace
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint4 q = ((const uint4*)src)[i];
    const u32 wv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n0 = 8 * i + 2 * e;
      // ISLOW_MULT_TYPE is a short in libjpeg-turbo: 16-bit quantisation values above 32767 wrap
      ws[n0] = (int)(int16_t)(wv[e] & 0xFFFF) * (int)(int16_t)f.qtable[comp][n0];
      ws[n0 + 1] = (int)(int16_t)(wv[e] >> 16) * (int)(int16_t)f.qtable[comp][n0 + 1];
    }
  }
  // pass 1: columns -> int workspace
#pragma unroll
  for (int col = 0; col < 8; ++col) {
    long long in[8], out[8];
#pragma unroll
    for (int r = 0; r < 8; ++r)
      in[r] = ws[8 * r + col];
    idct_1d<11>(in, out);
#pragma unroll
    for (int r = 0; r < 8; ++r)
      ws[8 * r + col] = (int)out[r];
  }
  // pass 2: rows -> samples
  u32 rows[8][2];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    long long in[8], out[8];
#pragma unroll
    for (int x = 0; x < 8; ++x)
      in[x] = ws[8 * r + x];
    idct_1d<18>(in, out);
    u32 lo = 0, hi = 0;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      lo |= (u32)range_limit((int)out[x]) << (8 * x);
      hi |= (u32)range_limit((int)out[x + 4]) << (8 * x);
    }
    rows[r][0] = lo, rows[r][1] = hi;
  }

  if (!raw) {
    // MCU-padded component planes: plane c is (mcux * hs * 8) x (mcuy * vs * 8), one after the other
    const u64 pw0 = (u64)f.mcux * H * 8, ph0 = (u64)f.mcuy * V * 8;
    const u64 pwc = (u64)f.mcux * 8, phc = (u64)f.mcuy * 8;
    u8* base = a.plane + L.blk * 64 + (comp == 0 ? 0 : pw0 * ph0 + (u64)(comp - 1) * pwc * phc);
    const u64 pitch = comp ? pwc : pw0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      uint2* o = (uint2*)(base + (u64)(by * 8 + r) * pitch + bx * 8);
      *o = make_uint2(rows[r][0], rows[r][1]);
    }
    return;
  }
  const vali_surface dsc = a.dst[img];
  const int nx = min(8, cw - bx * 8), ny = min(8, ch - by * 8);
  const bool nv12_c = fmt == VALI_FMT_NV12 && comp > 0;
  u8* plane = (u8*)(nv12_c ? dsc.plane[1] : dsc.plane[comp]);
  const int pitch = nv12_c ? dsc.pitch[1] : dsc.pitch[comp];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    if (r >= ny)
      break;
    u8* row = plane + (size_t)(by * 8 + r) * pitch;
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      if (x < nx) {
        const u8 v = (u8)(rows[r][x >> 2] >> (8 * (x & 3)));
        if (nv12_c)
          row[2 * (bx * 8 + x) + comp - 1] = v;
        else
          row[bx * 8 + x] = v;
      }
    }
  }
}

// ---- k_jd_color ----------------------------------------------------------------------------------------------------------
__device__ inline int clampu8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// chroma sample of output pixel (x, y): jdsample's fancy upsampling (or replication) of a plane of cw x ch samples
__device__ inline int upsample(const u8* pl, u64 pitch, int x, int y, int H, int V, int cw, int ch) {
  if (H == 1 && V == 1)
    return pl[(u64)y * pitch + x];
  if (H == 2 && V == 1) {
    const u8* row = pl + (u64)y * pitch;
    const int i = x >> 1;
    if (cw <= 2)
      return row[i];
    return (x & 1) ? (3 * row[i] + row[min(i + 1, cw - 1)] + 2) >> 2 : (3 * row[i] + row[max(i - 1, 0)] + 1) >> 2;
  }
  if (H == 1 && V == 2) {
    const int r = y >> 1;
    const int nr = (y & 1) ? min(r + 1, ch - 1) : max(r - 1, 0);
    return (3 * pl[(u64)r * pitch + x] + pl[(u64)nr * pitch + x] + ((y & 1) ? 2 : 1)) >> 2;
  }
  const int r = y >> 1, i = x >> 1;
  if (cw <= 2)
    return pl[(u64)r * pitch + i];
  const int nr = (y & 1) ? min(r + 1, ch - 1) : max(r - 1, 0);
  const u8* r0 = pl + (u64)r * pitch;
  const u8* r1 = pl + (u64)nr * pitch;
  const int ni = (x & 1) ? min(i + 1, cw - 1) : max(i - 1, 0);
  const int cs = 3 * r0[i] + r1[i], ns = 3 * r0[ni] + r1[ni];
  return (x & 1) ? (3 * cs + ns + 7) >> 4 : (3 * cs + ns + 8) >> 4;
}

__global__ void __launch_bounds__(256) k_jd_color(const Args a) {
  const int img = blockIdx.y;
  if (*a.flag || a.status[img] != ST_OK)
    return;
  const vali_jpeg_info& f = a.info[img];
  const u64 px = (u64)blockIdx.x * 256 + threadIdx.x;
  if (px >= (u64)f.width * f.height)
    return;
  const int x = (int)(px % f.width), y = (int)(px / f.width);
  const Lay L = a.lay[img];
  const int H = f.h_samp, V = f.v_samp;
  const u64 pw0 = (u64)f.mcux * H * 8, ph0 = (u64)f.mcuy * V * 8, pwc = (u64)f.mcux * 8, phc = (u64)f.mcuy * 8;
  const u8* p0 = a.plane + L.blk * 64;
  const int Y = p0[(u64)y * pw0 + x];
  int R = Y, G = Y, B = Y;
  if (f.components == 3) {
    const int cw = (f.width + H - 1) / H, ch = (f.height + V - 1) / V;
    const int cb = upsample(p0 + pw0 * ph0, pwc, x, y, H, V, cw, ch) - 128;
    const int cr = upsample(p0 + pw0 * ph0 + pwc * phc, pwc, x, y, H, V, cw, ch) - 128;
    // jdcolor ycc_rgb_convert tables: FIX(1.40200), FIX(1.77200), -FIX(0.71414), -FIX(0.34414), SCALEBITS = 16
    R = clampu8(Y + ((91881 * cr + 32768) >> 16));
    G = clampu8(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    B = clampu8(Y + ((116130 * cb + 32768) >> 16));
  }
  const vali_surface d = a.dst[img];
  if (a.format == VALI_FMT_RGB_PLANAR) {
    ((u8*)d.plane[0])[(size_t)y * d.pitch[0] + x] = (u8)R;
    ((u8*)d.plane[1])[(size_t)y * d.pitch[1] + x] = (u8)G;
    ((u8*)d.plane[2])[(size_t)y * d.pitch[2] + x] = (u8)B;
  } else {
    u8* o = (u8*)d.plane[0] + (size_t)y * d.pitch[0] + 3 * (size_t)x;
    const bool bgr = a.format == VALI_FMT_BGR;
    o[0] = (u8)(bgr ? B : R);
    o[1] = (u8)G;
    o[2] = (u8)(bgr ? R : B);
  }
}

// ---- host: marker parser ---------------------------------------------------------------------------------------------------
struct HuffSpec {
  bool have = false;
  u8 bits[16];
  u8 vals[256];
  int n = 0;
};

int build_huff(const char* fn, const HuffSpec& s, bool dc, vali_jpeg_huff* t) {
  memset(t, 0, sizeof(*t));
  if (!s.have)
    return fail(VALI_ERR_INVALID_ARG, "%s: a scan component uses an undefined Huffman table", fn);
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int nl = s.bits[l - 1];
    t->maxcode[l] = -1;
    if (nl) {
      t->valoff[l] = k - code;
      for (int i = 0; i < nl; ++i, ++k, ++code) {
        if (code >= (1 << l))
          return fail(VALI_ERR_INVALID_ARG, "%s: oversubscribed Huffman table", fn);
        if (code == (1 << l) - 1)
          return fail(VALI_ERR_INVALID_ARG, "%s: Huffman table holds the all-ones code", fn);
        const int sym = s.vals[k];
        if (dc && sym > 15)
          return fail(VALI_ERR_INVALID_ARG, "%s: DC Huffman symbol %d above 15", fn, sym);
        if (l <= 9)
          for (int e = code << (9 - l); e < (code + 1) << (9 - l); ++e)
            t->look[e] = (uint16_t)((l << 8) | sym);
      }
      t->maxcode[l] = code - 1;
    }
    code <<= 1;
  }
  t->maxcode[17] = 0x7FFFFFFF;
  memcpy(t->vals, s.vals, 256);
  return VALI_OK;
}

int parse(const char* fn, const u8* d, size_t len, vali_jpeg_info* out) {
  if (len < 4 || d[0] != 0xFF || d[1] != 0xD8)
    return fail(VALI_ERR_INVALID_ARG, "%s: no SOI marker", fn);
  bool have_q[4] = {false, false, false, false};
  uint16_t qt[4][64];
  HuffSpec ht[2][4];
  int ri = 0, adobe = -1;
  bool jfif = false, sof = false;
  int W = 0, Hh = 0, nc = 0, cid[3] = {0, 0, 0}, csamp[3] = {0, 0, 0}, ctq[3] = {0, 0, 0};
  size_t i = 2;
  for (;;) {
    if (i >= len || d[i] != 0xFF)
      return fail(VALI_ERR_INVALID_ARG, "%s: marker expected at byte %zu", fn, i);
    while (i < len && d[i] == 0xFF)
      ++i;  // fill bytes
    if (i >= len)
      return fail(VALI_ERR_INVALID_ARG, "%s: truncated header", fn);
    const int mk = d[i++];
    if (mk == 0xD8 || mk == 0xD9 || (mk >= 0xD0 && mk <= 0xD7) || mk == 0x01 || mk == 0x00)
      return fail(VALI_ERR_INVALID_ARG, "%s: marker 0x%02X before the scan", fn, mk);
    if (i + 2 > len)
      return fail(VALI_ERR_INVALID_ARG, "%s: truncated header", fn);
    const size_t L = ((size_t)d[i] << 8) | d[i + 1];
    if (L < 2 || i + L > len)
      return fail(VALI_ERR_INVALID_ARG, "%s: truncated header", fn);
    const u8* p = d + i + 2;
    const size_t n = L - 2;
    switch (mk) {
    case 0xC0:
    case 0xC1: {
      if (sof)
        return fail(VALI_ERR_INVALID_ARG, "%s: two frame headers", fn);
      sof = true;
      if (n < 6)
        return fail(VALI_ERR_INVALID_ARG, "%s: short SOF", fn);
      if (p[0] != 8)
        return fail(VALI_ERR_UNSUPPORTED, "%s: %d-bit samples (8-bit only)", fn, p[0]);
      Hh = (p[1] << 8) | p[2];
      W = (p[3] << 8) | p[4];
      nc = p[5];
      if (Hh == 0)
        return fail(VALI_ERR_UNSUPPORTED, "%s: height defined by DNL", fn);
      if (W == 0)
        return fail(VALI_ERR_INVALID_ARG, "%s: width 0", fn);
      if (nc != 1 && nc != 3)
        return fail(VALI_ERR_UNSUPPORTED, "%s: %d components (1 or 3 only)", fn, nc);
      if (n != 6 + 3 * (size_t)nc)
        return fail(VALI_ERR_INVALID_ARG, "%s: bad SOF length", fn);
      for (int c = 0; c < nc; ++c) {
        cid[c] = p[6 + 3 * c];
        csamp[c] = p[7 + 3 * c];
        ctq[c] = p[8 + 3 * c];
        if (ctq[c] > 3 || (csamp[c] >> 4) < 1 || (csamp[c] >> 4) > 4 || (csamp[c] & 15) < 1 || (csamp[c] & 15) > 4)
          return fail(VALI_ERR_INVALID_ARG, "%s: bad component %d", fn, c);
      }
      break;
    }
    case 0xC2: case 0xC6: case 0xCA: case 0xCE:
      return fail(VALI_ERR_UNSUPPORTED, "%s: progressive JPEG", fn);
    case 0xC3: case 0xC7: case 0xCB: case 0xCF:
      return fail(VALI_ERR_UNSUPPORTED, "%s: lossless JPEG", fn);
    case 0xC5:
      return fail(VALI_ERR_UNSUPPORTED, "%s: hierarchical JPEG", fn);
    case 0xC9: case 0xCD: case 0xCC:
      return fail(VALI_ERR_UNSUPPORTED, "%s: arithmetic coding", fn);
    case 0xDC:
      return fail(VALI_ERR_UNSUPPORTED, "%s: DNL marker", fn);
    case 0xC4: {
      size_t o = 0;
      while (o < n) {
        if (o + 17 > n)
          return fail(VALI_ERR_INVALID_ARG, "%s: short DHT", fn);
        const int tc = p[o] >> 4, th = p[o] & 15;
        if (tc > 1 || th > 3)
          return fail(VALI_ERR_INVALID_ARG, "%s: bad DHT class / id", fn);
        HuffSpec& h = ht[tc][th];
        int total = 0;
        for (int l = 0; l < 16; ++l)
          total += (h.bits[l] = p[o + 1 + l]);
        if (total > 256 || o + 17 + total > n)
          return fail(VALI_ERR_INVALID_ARG, "%s: bad DHT length", fn);
        memset(h.vals, 0, 256);
        memcpy(h.vals, p + o + 17, total);
        h.n = total;
        h.have = true;
        o += 17 + total;
      }
      break;
    }
    case 0xDB: {
      size_t o = 0;
      while (o < n) {
        const int pq = p[o] >> 4, tq = p[o] & 15;
        if (pq > 1 || tq > 3 || o + 1 + 64 * (pq + 1) > n)
          return fail(VALI_ERR_INVALID_ARG, "%s: bad DQT", fn);
        for (int k = 0; k < 64; ++k)
          qt[tq][kNatural[k]] = pq ? (uint16_t)((p[o + 1 + 2 * k] << 8) | p[o + 2 + 2 * k]) : p[o + 1 + k];
        have_q[tq] = true;
        o += 1 + 64 * (pq + 1);
      }
      break;
    }
    case 0xDD:
      if (n != 2)
        return fail(VALI_ERR_INVALID_ARG, "%s: bad DRI length", fn);
      ri = (p[0] << 8) | p[1];
      break;
    case 0xE0:
      if (n >= 5 && memcmp(p, "JFIF\0", 5) == 0)
        jfif = true;
      break;
    case 0xEE:
      if (n >= 12 && memcmp(p, "Adobe", 5) == 0)
        adobe = p[11];
      break;
    case 0xDA: {
      if (!sof)
        return fail(VALI_ERR_INVALID_ARG, "%s: scan before the frame header", fn);
      const int ns = n ? p[0] : 0;
      if (ns != nc)
        return fail(VALI_ERR_UNSUPPORTED, "%s: a scan of %d of %d components (multiple scans)", fn, ns, nc);
      if (n != 1 + 2 * (size_t)ns + 3)
        return fail(VALI_ERR_INVALID_ARG, "%s: bad SOS length", fn);
      const u8* e = p + 1 + 2 * ns;
      if (e[0] != 0 || e[1] != 63 || e[2] != 0)
        return fail(VALI_ERR_UNSUPPORTED, "%s: spectral selection / successive approximation", fn);
      if (nc == 3 && adobe == 0)
        return fail(VALI_ERR_UNSUPPORTED, "%s: Adobe transform 0 (RGB / CMYK colour space)", fn);
      if (nc == 3 && !jfif && adobe < 0 && cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B')
        return fail(VALI_ERR_UNSUPPORTED, "%s: RGB colour space", fn);
      memset(out, 0, sizeof(*out));
      int H = 1, V = 1;
      if (nc == 3) {
        H = csamp[0] >> 4, V = csamp[0] & 15;
        if (!sampling_ok(H, V) || csamp[1] != 0x11 || csamp[2] != 0x11)
          return fail(VALI_ERR_UNSUPPORTED, "%s: sampling %dx%d,%dx%d,%dx%d", fn, csamp[0] >> 4, csamp[0] & 15,
                      csamp[1] >> 4, csamp[1] & 15, csamp[2] >> 4, csamp[2] & 15);
      }
      for (int c = 0; c < nc; ++c) {
        if (p[1 + 2 * c] != cid[c])
          return fail(VALI_ERR_UNSUPPORTED, "%s: scan components not in frame order", fn);
        const int td = p[2 + 2 * c] >> 4, ta = p[2 + 2 * c] & 15;
        if (td > 3 || ta > 3)
          return fail(VALI_ERR_INVALID_ARG, "%s: bad table id in SOS", fn);
        int rc = build_huff(fn, ht[0][td], true, &out->dc[c]);
        if (rc == VALI_OK)
          rc = build_huff(fn, ht[1][ta], false, &out->ac[c]);
        if (rc != VALI_OK)
          return rc;
        if (!have_q[ctq[c]])
          return fail(VALI_ERR_INVALID_ARG, "%s: undefined quantisation table %d", fn, ctq[c]);
        memcpy(out->qtable[c], qt[ctq[c]], sizeof(qt[0]));
      }
      out->width = W, out->height = Hh, out->components = nc, out->h_samp = H, out->v_samp = V;
      out->restart_interval = ri;
      out->mcux = (W + 8 * H - 1) / (8 * H);
      out->mcuy = (Hh + 8 * V - 1) / (8 * V);
      out->blocks_per_mcu = nc == 1 ? 1 : H * V + 2;
      const long long mcus = (long long)out->mcux * out->mcuy;
      out->segments = (int)(ri ? (mcus + ri - 1) / ri : 1);
      // entropy data: up to the first FF that starts no stuffed byte and no RSTn
      const size_t start = i + L;
      size_t end = len;
      for (size_t x = start; x + 1 < len; ++x) {
        const u8* q = (const u8*)memchr(d + x, 0xFF, len - 1 - x);
        if (!q)
          break;
        x = (size_t)(q - d);
        const u8 nx = d[x + 1];
        if (nx != 0x00 && (nx < 0xD0 || nx > 0xD7)) {
          end = x;
          break;
        }
      }
      if (end < len) {
        size_t y = end;
        while (y < len && d[y] == 0xFF)
          ++y;
        const int after = y < len ? d[y] : 0xD9;
        if (after == 0xDC)
          return fail(VALI_ERR_UNSUPPORTED, "%s: DNL marker", fn);
        if (after != 0xD9)
          return fail(VALI_ERR_UNSUPPORTED, "%s: marker 0x%02X after the scan (multiple scans)", fn, after);
      }
      out->data_offset = start;
      out->data_len = end - start;
      if (out->data_len >= kMaxData)
        return fail(VALI_ERR_UNSUPPORTED, "%s: entropy-coded data of %llu bytes", fn,
                    (unsigned long long)out->data_len);
      return VALI_OK;
    }
    default:
      break;  // APPn, COM, ...
    }
    i += L;
  }
}

int totals(const char* fn, const vali_jpeg_info* infos, int n, Totals* t) {
  VALI_REQUIRE(infos || n == 0, "null infos");
  if (n < 0 || n > 65535)
    return fail(VALI_ERR_INVALID_ARG, "%s: batch size out of range (0..65535)", fn);
  *t = Totals{0, 0, 0, 0, 0};
  for (int i = 0; i < n; ++i) {
    if (!info_consistent(infos[i]))
      return fail(VALI_ERR_INVALID_ARG, "%s: info %d is not one vali_jpeg_parse made", fn, i);
    const ImgSize s = img_size(infos[i]);
    t->unst += s.unst, t->blocks += s.blocks, t->segs += s.segs, t->subs += s.subs;
    t->gsegs += (u64)infos[i].segments;
  }
  if (t->subs >= (1ull << 31) || t->segs >= (1ull << 31) || t->gsegs >= (1ull << 31) || t->blocks >= (1ull << 40))
    return fail(VALI_ERR_INVALID_ARG, "%s: batch too large for one call", fn);
  return VALI_OK;
}

bool format_fits(int format, const vali_jpeg_info& f) {
  switch (format) {
  case VALI_FMT_RGB: case VALI_FMT_BGR: case VALI_FMT_RGB_PLANAR: case VALI_FMT_Y:
    return true;
  case VALI_FMT_YUV444:
    return f.components == 3 && f.h_samp == 1 && f.v_samp == 1;
  case VALI_FMT_YUV422:
    return f.components == 3 && f.h_samp == 2 && f.v_samp == 1 && subsampled_sizes_ok(format, f.width, f.height);
  case VALI_FMT_YUV420: case VALI_FMT_NV12:
    return f.components == 3 && f.h_samp == 2 && f.v_samp == 2 && subsampled_sizes_ok(format, f.width, f.height);
  default:
    return false;
  }
}

} // namespace
} // namespace vali

using namespace vali;

extern "C" {

int vali_jpeg_parse(const uint8_t* data, size_t len, vali_jpeg_info* out) {
  VALI_REQUIRE(data && out, "null argument");
  vali_jpeg_info tmp;
  const int rc = parse(__func__, data, len, &tmp);
  if (rc == VALI_OK)
    *out = tmp;
  return rc;
}

int vali_jpeg_decode_workspace_size(const vali_jpeg_info* infos, int n, size_t* bytes) {
  VALI_REQUIRE(bytes, "null output");
  Totals t;
  const int rc = totals(__func__, infos, n, &t);
  if (rc != VALI_OK)
    return rc;
  *bytes = (size_t)ws_map(t, n).total;
  return VALI_OK;
}

int vali_jpeg_decode_batch(const vali_jpeg_info* infos, const vali_jpeg_info* d_infos, int n, const uint8_t* d_data,
                           int format, const vali_surface* d_dst, void* workspace, size_t ws_bytes, int32_t* d_status,
                           vali_stream_t stream) {
  Totals t;
  int rc = totals(__func__, infos, n, &t);
  if (rc != VALI_OK)
    return rc;
  if (n == 0)
    return VALI_OK;
  VALI_REQUIRE(d_infos && d_data && d_dst && workspace && d_status, "null argument");
  for (int i = 0; i < n; ++i)
    if (!format_fits(format, infos[i]))
      return fail(VALI_ERR_UNSUPPORTED, "%s: file %d (%d components, %dx%d sampling, %d x %d) cannot be decoded to "
                  "format %d", __func__, i, infos[i].components, infos[i].h_samp, infos[i].v_samp, infos[i].width,
                  infos[i].height, format);
  VALI_REQUIRE((((uintptr_t)workspace) & 255) == 0, "workspace not 256-byte aligned");
  const WsMap m = ws_map(t, n);
  VALI_REQUIRE(ws_bytes >= m.total, "workspace below vali_jpeg_decode_workspace_size");
  u8* ws = (u8*)workspace;
  Args a;
  a.info = d_infos;
  a.data = d_data;
  a.dst = d_dst;
  a.status = d_status;
  a.lay = (Lay*)(ws + m.lay);
  a.flag = (u32*)(ws + m.flag);
  a.unst = ws + m.unst;
  a.seg_start = (u32*)(ws + m.seg_start);
  a.seg_sub = (u32*)(ws + m.seg_sub);
  a.ent_p = (u32*)(ws + m.ent_p);
  a.ent_ck = (u32*)(ws + m.ent_ck);
  a.ext_p = (u32*)(ws + m.ext_p);
  a.ext_ck = (u32*)(ws + m.ext_ck);
  a.cnt = (u32*)(ws + m.cnt);
  a.head = (u32*)(ws + m.head);
  a.tail = (u32*)(ws + m.tail);
  a.coef = (int16_t*)(ws + m.coef);
  a.plane = ws + m.plane;
  a.tot = t;
  a.n = n;
  a.format = format;
  u64 maxpix = 1;
  for (int i = 0; i < n; ++i)
    maxpix = std::max(maxpix, (u64)infos[i].width * infos[i].height);

  hipStream_t s = as_stream(stream);
  VALI_ENTRY(s);
  VALI_HIP_CHECK(hipMemsetAsync(a.coef, 0, t.blocks * 128, s));
  hipLaunchKernelGGL(k_jd_layout, dim3(1), dim3(256), 0, s, a);
  VALI_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_jd_unstuff, dim3(n), dim3(1024), 0, s, a);
  VALI_LAUNCH_CHECK();
  const u32 groups = (u32)(t.subs / kGroup);
  hipLaunchKernelGGL(k_jd_sync, dim3(groups), dim3(kGroup), 0, s, a);
  VALI_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_jd_seams, dim3(n), dim3(64), 0, s, a);
  VALI_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_jd_write, dim3(groups), dim3(kGroup), 0, s, a);
  VALI_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_jd_dc, dim3(n), dim3(1024), 0, s, a);
  VALI_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_jd_idct, dim3((u32)((t.blocks + 255) / 256)), dim3(256), 0, s, a);
  VALI_LAUNCH_CHECK();
  if (format == VALI_FMT_RGB || format == VALI_FMT_BGR || format == VALI_FMT_RGB_PLANAR) {
    hipLaunchKernelGGL(k_jd_color, dim3((u32)((maxpix + 255) / 256), n), dim3(256), 0, s, a);
    VALI_LAUNCH_CHECK();
  }
  return VALI_OK;
}

} // extern "C"
