// Baseline sequential JFIF encoder: the reference's PyNvJpegEncoder (src/TC/src/TaskNvJpegEncode.cpp, nvJPEG).
//
// DEFINITION = libjpeg's encoder with the Annex K Huffman tables (include/vali_hip.h, "JPEG"); tests/jpeg_model.py
// restates it and tests/test_jpeg_host.py pins the restatement to Pillow's libjpeg byte for byte.
//
// Four launches in stream order; none hands data to another workgroup of the same launch:
//   k_jpeg_fdct      lane = one 8x8 block of one component, in MCU-interleaved scan order: load (edge replication,
//                    rgb_ycc for RGB sources), islow FDCT, quantise, zigzag -> 128 B of int16 in the workspace.
//                    The pixels come from 8-bit surfaces, or from one float32 / float16 / bfloat16 / uint8 tensor
//                    whose elements are scaled, rounded and clamped to 0..255 in registers (vali_jpeg_encode_tensor).
//                    A dummy block of a partial MCU computes the block whose DC it copies and keeps only that DC.
//                    RGB sources coded 4:2:2 / 4:2:0: a luma lane also averages the chroma of its 8x8 pixels (jcsample)
//                    and hands it to the MCU's chroma lanes through LDS (fdct_subsampled).
//   k_jpeg_huff      wave = one restart segment (<= 64 blocks), lane = one block: count the bits of each block,
//                    prefix-sum them into bit offsets, OR the codes into an LDS bit buffer (ds_or_b32), pad with
//                    1-bits, then stuff a 0x00 after every 0xFF (per-chunk counts + prefix sum) into the segment's
//                    worst-case slot; its length goes to the length array.
//   k_jpeg_offsets   workgroup = one image: exclusive scan of (segment length + 2 bytes of RST) -> offsets, size.
//   k_jpeg_assemble  workgroup = one segment: copy it and its RST marker to the image's output slot.
//
// optimize = 1 (per-image Huffman tables, libjpeg's jpeg_gen_optimal_table; tests/jpeg_optimize_model.py restates it):
// a memset of the histograms and two more launches between k_jpeg_fdct and k_jpeg_huff,
//   k_jpeg_hist      walks the coefficients as k_jpeg_huff does (wave = segment, lane = block, code_block in its
//                    counting mode) and counts every symbol into an LDS histogram (ds_add_u32); the non-zero bins
//                    of a workgroup then go to the image's four 256-bin histograms with global atomic adds.
//   k_jpeg_tables    wave = one table of one image: the merges of the Huffman construction with the 257 counts in
//                    registers (the two smallest by a wave reduction that carries the index), code lengths, the
//                    16-bit limit of Annex K.2, HUFFVAL order and the Annex C codes -> the table k_jpeg_huff codes
//                    with, and the table's bytes of the DHT segment.
// k_jpeg_huff then codes with the image's tables, k_jpeg_offsets starts every image after its DHT + DRI + SOS, and
// k_jpeg_assemble writes those in front of the entropy data.
//
// Regions of surfaces of any sizes (vali_jpeg_encode_rois): the same launches, each as a one-dimensional grid over the
// sum of the images' workgroups.  vali_jpeg_plan_rois lays the images out on the host, one vali_jpeg_item each: its
// geometry, where its coefficients, segments and output start, and its first workgroup in every launch.  A workgroup
// of k_jpeg_fdct_roi / _hist_roi / _huff_roi / _assemble_roi finds its item by a binary search of that field with
// blockIdx.x, which is scalar work, and then runs the body it shares with the uniform kernel; k_jpeg_offsets_roi and
// k_jpeg_tables are per image anyway.  The loader starts at the rectangle's origin and counts, and replicates, rows and
// columns in the rectangle (SurfIn::item_at).
#include <cmath>
#include <cstring>
#include <type_traits>

#include "common.hpp"
#include "tensor_in.hpp"

namespace vali {
namespace {

typedef uint32_t u32;
typedef uint8_t u8;

// ---- Annex K (ITU T.81): the one copy of the tables, for the header writer and the kernels ---------------------------
constexpr u8 kLumaQ[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57,
                           69, 56, 14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64,
                           81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr u8 kChromaQ[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                             99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                             99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// natural index of zigzag position k
constexpr int kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffSpec {
  u8 bits[16];   // BITS: number of codes of length 1..16
  u8 vals[162];  // HUFFVAL
  int nvals;
};

// DHT order: DC luma, AC luma, DC chroma, AC chroma (table class << 4 | id = 0x00, 0x10, 0x01, 0x11)
constexpr HuffSpec kHuff[4] = {
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12},
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
     {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
      0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
      0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
      0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
      0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
      0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
      0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
      0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
      0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
     162},
    {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12},
    {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
     {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
      0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
      0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
      0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
      0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
      0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
      0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
      0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
      0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
     162}};

// symbol -> (code << 8) | length (Annex C); length 0 = no such symbol
struct CodeTable {
  u32 e[256];
};

constexpr CodeTable build_codes(const HuffSpec& s) {
  CodeTable t{};
  u32 code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < s.bits[len - 1]; ++i)
      t.e[s.vals[k++]] = (code++ << 8) | (u32)len;
    code <<= 1;
  }
  return t;
}

// device copy, built at compile time from kHuff: DC luma, AC luma, DC chroma, AC chroma
__constant__ CodeTable d_codes[4] = {build_codes(kHuff[0]), build_codes(kHuff[1]), build_codes(kHuff[2]),
                                     build_codes(kHuff[3])};

// Worst case of one block: DC 11 + 11 bits (chroma), 63 AC of 16 + 10 bits: 1660 bits < 208 bytes.  A segment's
// stuffed bytes at most double that.
constexpr int kBlockBytes = 208;
constexpr int kSegBlocks = 64;
constexpr int kHuffWords = kSegBlocks * kBlockBytes / 4 + 2;  // LDS bit buffer (+ padding word, + spill word)

// optimize = 1: what the device writes in front of an image's entropy data, at most: DHT (marker, length, four tables
// of class byte + BITS + at most 12 / 162 values: DC sizes 0..11, AC runs 0..15 x sizes 1..10 + ZRL + EOB), DRI, SOS
constexpr int kDriSosBytes = 6 + 14;
constexpr int kPrefixMax = 4 + 4 * 17 + 12 + 12 + 162 + 162 + kDriSosBytes;
constexpr int kDhtSlot = 288;       // workspace bytes of one table's part of the DHT: 17 + 256 values, rounded up
constexpr int kHistWaves = 4;       // waves of a k_jpeg_hist workgroup
constexpr int kHistSegsPerWave = 4; // restart segments each of them counts (profiles/jpeg_optimize.md)

// ---- geometry ------------------------------------------------------------------------------------------------------------
struct JpegGeom {
  int H, V, bpm, R, bps;          // luma sampling, blocks per MCU, MCUs / blocks per segment
  int mcux, mcuy, nblocks, nseg;  // per image
  int cw[3], ch[3], bw[3], bh[3]; // component size in samples / real blocks
  size_t slot;                    // bytes of one segment slot
  size_t coef_bytes, len_at, off_at, slot_at;  // workspace layout of a batch
  int optimize;                                // per-image Huffman tables:
  size_t prefix;                               //   worst case of DHT + DRI + SOS in front of the entropy data
  size_t hist_at, codes_at, dht_at, dhtlen_at; //   histograms, code tables, DHT parts and their lengths
  size_t ws_bytes;
};

// one image's output slot: every segment's worst case and its RST marker, after the worst case of the prefix
inline size_t jpeg_capacity(const JpegGeom& g) { return g.prefix + (size_t)g.nseg * (g.slot + 2); }

int jpeg_sampling(int format, int* H, int* V) {
  switch (format) {
  case VALI_FMT_RGB: case VALI_FMT_BGR: case VALI_FMT_RGB_PLANAR: case VALI_FMT_YUV444:
    *H = 1, *V = 1;
    return 1;
  case VALI_FMT_YUV422:
    *H = 2, *V = 1;
    return 1;
  case VALI_FMT_YUV420:
    *H = 2, *V = 2;
    return 1;
  default:
    return 0;
  }
}

bool jpeg_is_rgb(int format) {
  return format == VALI_FMT_RGB || format == VALI_FMT_BGR || format == VALI_FMT_RGB_PLANAR;
}

// the luma samplings a format can be coded with: its own; RGB sources also 2x1 and 2x2 (chroma is downsampled)
bool jpeg_sampling_ok(int format, int h_samp, int v_samp) {
  int H, V;
  if (!jpeg_sampling(format, &H, &V))
    return false;
  if (h_samp == H && v_samp == V)
    return true;
  return jpeg_is_rgb(format) && h_samp == 2 && (v_samp == 1 || v_samp == 2);
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// what of g depends on the image's size; H, V, bpm and R are set
void jpeg_image_geom(int w, int h, JpegGeom* g) {
  const int H = g->H, V = g->V;
  g->mcux = (w + 8 * H - 1) / (8 * H);
  g->mcuy = (h + 8 * V - 1) / (8 * V);
  const long long nmcu = (long long)g->mcux * g->mcuy;
  g->nblocks = (int)(nmcu * g->bpm);
  g->nseg = (int)((nmcu + g->R - 1) / g->R);
  for (int c = 0; c < 3; ++c) {
    const int hs = c ? 1 : H, vs = c ? 1 : V;
    g->cw[c] = (w * hs + H - 1) / H;
    g->ch[c] = (h * vs + V - 1) / V;
    g->bw[c] = (g->cw[c] + 7) / 8;
    g->bh[c] = (g->ch[c] + 7) / 8;
  }
}

// the workspace of n images that hold `blocks` blocks and `segs` segments together
void jpeg_layout(size_t n, size_t blocks, size_t segs, JpegGeom* g) {
  g->coef_bytes = align256(blocks * 128);
  g->len_at = g->coef_bytes;
  g->off_at = g->len_at + align256(segs * 4);
  g->slot_at = g->off_at + align256(segs * 4);
  g->ws_bytes = g->slot_at + segs * g->slot;
  if (g->optimize) {
    g->hist_at = align256(g->ws_bytes);
    g->codes_at = g->hist_at + n * 4 * 256 * sizeof(u32);
    g->dht_at = g->codes_at + n * 4 * 256 * sizeof(u32);
    g->dhtlen_at = g->dht_at + align256(n * 4 * kDhtSlot);
    g->ws_bytes = g->dhtlen_at + align256(n * 4 * sizeof(u32));
  }
}

// checks params and sizes; fills g (workspace layout for a batch of n)
int jpeg_geom(const char* fn, int n, int w, int h, const vali_jpeg_params* p, JpegGeom* g) {
  if (!p)
    return fail(VALI_ERR_INVALID_ARG, "%s: null params", fn);
  if (w < 1 || h < 1 || w > 65535 || h > 65535)
    return fail(VALI_ERR_INVALID_ARG, "%s: size %d x %d outside 1..65535", fn, w, h);
  int H, V;
  if (!jpeg_sampling(p->format, &H, &V))
    return fail(VALI_ERR_UNSUPPORTED, "%s: format %d cannot be encoded", fn, p->format);
  if (!jpeg_sampling_ok(p->format, p->h_samp, p->v_samp))
    return fail(VALI_ERR_INVALID_ARG, "%s: sampling %dx%d does not match format %d", fn, p->h_samp, p->v_samp,
                p->format);
  H = p->h_samp, V = p->v_samp;
  if (!subsampled_sizes_ok(p->format, w, h))
    return fail(VALI_ERR_INVALID_ARG, "%s: %d x %d: 4:2:0 needs an even width and height, 4:2:2 an even width", fn,
                w, h);
  const int bpm = H * V + 2;
  if (p->optimize != 0 && p->optimize != 1)
    return fail(VALI_ERR_INVALID_ARG, "%s: optimize must be 0 or 1, not %d", fn, p->optimize);
  if (p->restart_interval < 1 || p->restart_interval * bpm > kSegBlocks)
    return fail(VALI_ERR_INVALID_ARG, "%s: restart interval %d outside 1..%d", fn, p->restart_interval,
                kSegBlocks / bpm);
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 64; ++k)
      if (p->qtable[t][k] == 0)
        return fail(VALI_ERR_INVALID_ARG, "%s: quantisation table %d holds 0", fn, t);
  if (n < 0 || n > 65535)
    return fail(VALI_ERR_INVALID_ARG, "%s: batch size out of range (0..65535)", fn);
  g->H = H, g->V = V, g->bpm = bpm, g->R = p->restart_interval, g->bps = g->R * bpm;
  jpeg_image_geom(w, h, g);
  g->slot = (size_t)2 * g->bps * kBlockBytes;
  g->optimize = p->optimize;
  g->prefix = p->optimize ? kPrefixMax : 0;
  // one image's output slot must stay addressable with 32-bit offsets
  if (jpeg_capacity(*g) > 0xFFFFFFFFull)
    return fail(VALI_ERR_INVALID_ARG, "%s: %d x %d is too large for one output slot", fn, w, h);
  const size_t nn = (size_t)(n > 0 ? n : 1);
  jpeg_layout(nn, nn * g->nblocks, nn * g->nseg, g);
  return VALI_OK;
}

// ---- regions of surfaces of any sizes: the plan -----------------------------------------------------------------------
// what the items before item i add up to: where item i starts in every area and every flattened grid
struct RoiTotals {
  uint64_t blocks, segs, out, wg_fdct, wg_hist;
};

// blocks of one k_jpeg_fdct workgroup: 256, or the whole MCUs of a subsampled RGB source
int fdct_blocks_per_wg(const vali_jpeg_params* p, const JpegGeom& g) {
  return jpeg_is_rgb(p->format) && g.H * g.V > 1 ? 256 / g.bpm * g.bpm : 256;
}

// what of params a plan depends on, beyond what the records themselves hold
u32 roi_check(const vali_jpeg_params* p) {
  return 0x4A524F49u ^ (u32)p->format ^ (u32)p->h_samp << 8 ^ (u32)p->v_samp << 12 ^ (u32)p->optimize << 16 ^
         (u32)p->restart_interval << 20;
}

// The record of rectangle r (1..65535 on a side), the next after the items that add up to *t; g holds the params'
// part.  False when its output slot or a flattened grid would pass what 32 bits address.
bool roi_item(const vali_jpeg_roi& r, const vali_jpeg_params* p, JpegGeom* g, RoiTotals* t, vali_jpeg_item* it) {
  jpeg_image_geom(r.width, r.height, g);
  if (jpeg_capacity(*g) > 0xFFFFFFFFull)
    return false;
  memset(it, 0, sizeof(*it));
  it->x = r.x, it->y = r.y, it->width = r.width, it->height = r.height;
  it->mcux = g->mcux, it->mcuy = g->mcuy, it->nblocks = g->nblocks, it->nseg = g->nseg;
  for (int c = 0; c < 3; ++c)
    it->cw[c] = g->cw[c], it->ch[c] = g->ch[c], it->bw[c] = g->bw[c], it->bh[c] = g->bh[c];
  it->wg_fdct = (u32)t->wg_fdct, it->wg_hist = (u32)t->wg_hist, it->wg_seg = (u32)t->segs;
  it->check = roi_check(p);
  it->block_first = t->blocks, it->seg_first = t->segs, it->out_offset = t->out;
  const int per_wg = fdct_blocks_per_wg(p, *g), per_hist = kHistWaves * kHistSegsPerWave;
  t->blocks += (uint64_t)g->nblocks;
  t->segs += (uint64_t)g->nseg;
  t->out += jpeg_capacity(*g);
  t->wg_fdct += (uint64_t)((g->nblocks + per_wg - 1) / per_wg);
  t->wg_hist += (uint64_t)((g->nseg + per_hist - 1) / per_hist);
  return t->wg_fdct <= 0x7FFFFFFFull && t->segs <= 0x7FFFFFFFull;
}

// ---- k_jpeg_fdct -----------------------------------------------------------------------------------------------------
struct FdctArgs {
  int16_t* coef;  // image i: coef + i * nblocks * 64
  int H, V, HV, bpm, mcux, nblocks;
  int cw[3], ch[3], bw[3], bh[3];
  u32 recip[2][64];       // jcdctmgr reciprocal of 8 q (natural order)
  u32 corr_shift[2][64];  // correction | shift << 16
};

// 8-bit surfaces; from SRC_TENSOR on one (N, 3, H, W) tensor: SRC_TENSOR | dtype << 2 | channels last << 1 | YUV
// (a named type: k_jpeg_fdct's signature spells `SRC >= SRC_TENSOR` out, and an unnamed enum is numbered differently in
// the host and the device pass, so the host looked for a kernel symbol the code object does not have)
enum JpegSrc { SRC_YUV = 0, SRC_RGB = 1, SRC_BGR = 2, SRC_RGB_PLANAR = 3, SRC_TENSOR = 16 };

constexpr int tensor_src(int dtype, bool packed, bool yuv) {
  return SRC_TENSOR | dtype << 2 | (packed ? 2 : 0) | (yuv ? 1 : 0);
}

constexpr int fix16(double x) { return (int)(x * 65536 + 0.5); }

// 8 samples of one row, columns x0.. clamped to the last column cw - 1
__device__ __forceinline__ void load_row_u8(const u8* row, int x0, int cw, int v[8]) {
  const u8* p = row + x0;
  if (x0 + 8 <= cw && (((uintptr_t)p) & 3) == 0) {
    const u32 a = *(const u32*)p, b = *(const u32*)(p + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = (a >> (8 * i)) & 0xFF;
      v[4 + i] = (b >> (8 * i)) & 0xFF;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      v[i] = row[min(x0 + i, cw - 1)];
  }
}

__device__ __forceinline__ void load_row_rgb(const u8* row, int x0, int cw, int r[8], int g[8], int b[8]) {
  const u8* p = row + 3 * x0;
  if (x0 + 8 <= cw && (((uintptr_t)p) & 3) == 0) {
    u32 w[6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
      w[i] = ((const u32*)p)[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = 3 * i;
      r[i] = (w[k / 4] >> (8 * (k % 4))) & 0xFF;
      g[i] = (w[(k + 1) / 4] >> (8 * ((k + 1) % 4))) & 0xFF;
      b[i] = (w[(k + 2) / 4] >> (8 * ((k + 2) % 4))) & 0xFF;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const u8* q = row + 3 * min(x0 + i, cw - 1);
      r[i] = q[0], g[i] = q[1], b[i] = q[2];
    }
  }
}

// ---- where k_jpeg_fdct takes its pixels from ---------------------------------------------------------------------------
// A source hands out rows of 8 pixels, columns x0.. clamped to the last column cw - 1, as ints 0..255: rgb_row the
// three colours by name, comp_row component c as it is (kYuv sources).  Everything after the load is the same code.
// Args travel as a kernel argument; Item is what a lane keeps of its image.  The functions are static and the Item a
// local of the kernel: held as a member of an object, a vali_surface stayed in memory and was promoted to LDS.

// 8-bit surfaces
template <int SRC>
struct SurfIn {
  static constexpr bool kYuv = SRC == SRC_YUV;
  struct Args {
    const vali_surface* d_src;
  };
  typedef vali_surface Item;  // what a lane keeps of its image
  static __device__ __forceinline__ Item item(const Args& a, int i) { return a.d_src[i]; }
  // The image as a rectangle with its origin at pixel (x0, y0) sees it (vali_jpeg_encode_rois): every plane starts at
  // the origin, a subsampled chroma plane (H x V, kYuv sources) at the origin over its sampling.  Rows and columns are
  // then counted, and replicated, in the rectangle; an origin off a dword falls to the byte path of load_row_*.
  static __device__ __forceinline__ Item item_at(const Args& a, int i, int x0, int y0, int H, int V) {
    Item s = a.d_src[i];
    const int bpp = SRC == SRC_RGB || SRC == SRC_BGR ? 3 : 1;
    const void *p0 = s.plane[0], *p1 = s.plane[1], *p2 = s.plane[2];
    s.plane[0] = (void*)((const u8*)p0 + (size_t)y0 * s.pitch[0] + bpp * x0);
    if (SRC == SRC_RGB_PLANAR || SRC == SRC_YUV) {
      const int cx = kYuv ? x0 / H : x0, cy = kYuv ? y0 / V : y0;
      s.plane[1] = (void*)((const u8*)p1 + (size_t)cy * s.pitch[1] + cx);
      s.plane[2] = (void*)((const u8*)p2 + (size_t)cy * s.pitch[2] + cx);
    }
    return s;
  }
  static __device__ __forceinline__ void rgb_row(const Args&, const Item& s, int y, int x0, int cw, int R[8], int G[8],
                                                 int B[8]) {
    if (SRC == SRC_RGB_PLANAR) {
      load_row_u8((const u8*)s.plane[0] + (size_t)y * s.pitch[0], x0, cw, R);
      load_row_u8((const u8*)s.plane[1] + (size_t)y * s.pitch[1], x0, cw, G);
      load_row_u8((const u8*)s.plane[2] + (size_t)y * s.pitch[2], x0, cw, B);
    } else if (SRC == SRC_RGB) {
      load_row_rgb((const u8*)s.plane[0] + (size_t)y * s.pitch[0], x0, cw, R, G, B);
    } else {
      load_row_rgb((const u8*)s.plane[0] + (size_t)y * s.pitch[0], x0, cw, B, G, R);
    }
  }
  static __device__ __forceinline__ void comp_row(const Args&, const Item& s, int c, int y, int x0, int cw, int v[8]) {
    // values first, then the choice: a choice between the members themselves is a choice of addresses, and kept s
    // in memory
    const void *p0 = s.plane[0], *p1 = s.plane[1], *p2 = s.plane[2];
    const int q0 = s.pitch[0], q1 = s.pitch[1], q2 = s.pitch[2];
    const u8* plane = (const u8*)(c == 0 ? p0 : c == 1 ? p1 : p2);
    const int pitch = c == 0 ? q0 : c == 1 ? q1 : q2;
    load_row_u8(plane + (size_t)y * pitch, x0, cw, v);
  }
};

// One (N, 3, H, W) tensor (vali_jpeg_encode_tensor): TensorArgs, TensorElem and TensorIn of tensor_in.hpp, shared with
// tensor_to_surface.hip.

template <int SRC>
using SourceOf = std::conditional_t<(SRC >= SRC_TENSOR), TensorIn<(SRC >> 2) & 3, (SRC & 2) != 0, (SRC & 1) != 0>,
                                    SurfIn<SRC>>;

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of libjpeg's jfdctint over d[0], d[S], ..., d[7 S]; ROWS = pass 1 (keeps PASS1_BITS = 2 extra bits)
template <bool ROWS, int S>
__device__ __forceinline__ void fdct_pass(int* d) {
  constexpr int sh = ROWS ? 13 - 2 : 13 + 2;
  const int tmp0 = d[0] + d[7 * S], tmp7 = d[0] - d[7 * S];
  const int tmp1 = d[S] + d[6 * S], tmp6 = d[S] - d[6 * S];
  const int tmp2 = d[2 * S] + d[5 * S], tmp5 = d[2 * S] - d[5 * S];
  const int tmp3 = d[3 * S] + d[4 * S], tmp4 = d[3 * S] - d[4 * S];
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  if (ROWS) {
    d[0] = (tmp10 + tmp11) * 4;
    d[4 * S] = (tmp10 - tmp11) * 4;
  } else {
    d[0] = descale(tmp10 + tmp11, 2);
    d[4 * S] = descale(tmp10 - tmp11, 2);
  }
  int z1 = (tmp12 + tmp13) * 4433;
  d[2 * S] = descale(z1 + tmp13 * 6270, sh);
  d[6 * S] = descale(z1 - tmp12 * 15137, sh);
  z1 = tmp4 + tmp7;
  int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int z5 = (z3 + z4) * 9633;
  const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d[7 * S] = descale(t4 + z1 + z3, sh);
  d[5 * S] = descale(t5 + z2 + z4, sh);
  d[3 * S] = descale(t6 + z2 + z3, sh);
  d[S] = descale(t7 + z1 + z4, sh);
}

// CS: chroma sampling of an RGB source, 0 = 1x1 (4:4:4), 1 = 2x1 (4:2:2), 2 = 2x2 (4:2:0)
template <int CS>
struct SubGeom {
  static constexpr int V = CS == 2 ? 2 : 1, HV = 2 * V, BPM = HV + 2;
  static constexpr int MPW = 256 / BPM;  // whole MCUs of one workgroup: 64 (all 256 lanes) / 42 (252 lanes)
  static constexpr int NQ = 8 / V;       // dwords of one component of one quadrant: its rows of 4 chroma samples
  static constexpr int STRIDE = 2 * HV * NQ + 1;  // dwords of one MCU in LDS: 32, + 1 so that MCUs start on different banks
};

// One 8x8 quadrant of an MCU of a subsampled RGB source, pixel columns x0.. (replicated at column w - 1) and rows y0..:
// LUMA: d = Y - 128.  CHROMA: cq[0 / 1][k] = row k of the quadrant's 4 wide Cb / Cr samples, one byte each: jccolor on
// every pixel, truncated to 8 bits, then jcsample's h2v1 / h2v2 average with its alternating bias (0, 1 / 1, 2; the
// quadrant starts on an even chroma column).  Rows are replicated as the component wants them: luma at row h - 1;
// chroma (CROWS) at 4:2:0 in pairs, row 2 y' + (Y & 1) of y' = min(Y / 2, ch - 1) -- the same row wherever Y < h.
template <class IN, int CS, bool LUMA, bool CHROMA, bool CROWS>
__device__ __forceinline__ void load_quadrant(const typename IN::Args& src, const typename IN::Item& s, int x0,
                                              int y0, int w, int h, int ch, int* d, u32 (*cq)[SubGeom<CS>::NQ]) {
  int even[2][4];  // 4:2:0: the horizontal sums of the even row
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int Y = y0 + r;
    const int y = CROWS && CS == 2 ? min(2 * min(Y >> 1, ch - 1) + (Y & 1), h - 1) : min(Y, h - 1);
    int R[8], G[8], B[8];
    IN::rgb_row(src, s, y, x0, w, R, G, B);
    if (LUMA) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        d[8 * r + i] = ((fix16(0.299) * R[i] + fix16(0.587) * G[i] + fix16(0.114) * B[i] + (1 << 15)) >> 16) - 128;
    }
    if (CHROMA) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int kr = k == 0 ? -fix16(0.16874) : fix16(0.5);
        const int kg = k == 0 ? -fix16(0.33126) : -fix16(0.41869);
        const int kb = k == 0 ? fix16(0.5) : -fix16(0.08131);
        constexpr int off = (128 << 16) + (1 << 15) - 1;
        u32 packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int sum = ((kr * R[2 * j] + kg * G[2 * j] + kb * B[2 * j] + off) >> 16) +
                          ((kr * R[2 * j + 1] + kg * G[2 * j + 1] + kb * B[2 * j + 1] + off) >> 16);
          if (CS == 1)
            packed |= (u32)((sum + (j & 1)) >> 1) << (8 * j);
          else if ((r & 1) == 0)
            even[k][j] = sum;
          else
            packed |= (u32)((even[k][j] + sum + 1 + (j & 1)) >> 2) << (8 * j);
        }
        if (CS == 1)
          cq[k][r] = packed;
        else if (r & 1)
          cq[k][r / 2] = packed;
      }
    }
  }
}

// CS != 0, a subsampled RGB source: the lane of a luma block loads its 8x8 pixels once, keeps Y and hands the 4 wide Cb
// and Cr samples of its quadrant of the MCU to the MCU's two chroma lanes through LDS; a chroma lane that loaded its own
// 16 x 8 or 16 x 16 pixels would do so while the luma lanes of its wave wait.  A workgroup holds whole MCUs (the last
// 256 % BPM lanes idle); the order of the blocks in the workspace stays the MCU-interleaved scan order.
// The source's own arguments travel beside FdctArgs: nothing takes the address of `a`, so its tables are read where they
// are used (fdct_args below).
//
// k_jpeg_fdct_roi (vali_jpeg_encode_rois): the grid is one-dimensional over the workgroups of images of any sizes, and a
// workgroup reads what it works on from the record of the item that blockIdx.x falls in, into FdctWork: scalars, not
// the record, since whatever stays live across the 64 ints of the block must sit in SGPRs.  In k_jpeg_fdct the image is
// blockIdx.y and its geometry the launch's, and FdctWork only names what the kernel arguments hold.  The two kernels
// share fdct_block.
struct FdctWork {
  int img;        // the image's descriptor / tensor item
  int wg;         // the workgroup's place among the image's
  int16_t* coef;  // the image's coefficients
  int mcux, nblocks, cw0, cw1, ch0, ch1, bw0, bw1, bh0, bh1;
};

// the lane's image: as it is, or as the item's rectangle sees it
template <class IN, bool ROI>
__device__ __forceinline__ typename IN::Item fdct_item(const typename IN::Args& src, int img, int x0, int y0, int H,
                                                       int V) {
  if constexpr (ROI)
    return IN::item_at(src, img, x0, y0, H, V);
  else
    return IN::item(src, img);
}

// The item whose workgroups hold workgroup `wg`: the last one whose first workgroup (field FIRST, ascending, [0] = 0) is
// <= wg.  wg is blockIdx.x, the same for every lane, so the search and everything read from the record stay scalar.
template <u32 vali_jpeg_item::*FIRST>
__device__ __forceinline__ int find_item(const vali_jpeg_item* __restrict__ items, int n, u32 wg) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (items[mid].*FIRST <= wg)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// The kernel's FdctArgs where the dispatch put them: FdctArgs is the FIRST argument of k_jpeg_fdct and k_jpeg_fdct_roi, so
// it starts the kernel argument segment, and fdct_block reads it there, each field and table entry where it is used,
// as a kernel does with an argument that nothing takes the address of.  Handed `a` by reference or by value, fdct_block
// had all 256 table entries loaded up front, and every instantiation spilled 220..380 SGPRs.
typedef const FdctArgs __attribute__((address_space(4))) * FdctArgsPtr;
__device__ __forceinline__ FdctArgsPtr fdct_args() { return (FdctArgsPtr)__builtin_amdgcn_kernarg_segment_ptr(); }

// One block of workgroup g.wg of the image g names: load, FDCT, quantisation, zigzag.  (rx, ry): ROI, the rectangle's
// origin in its surface.
template <int SRC, int CS, bool ROI>
__device__ __forceinline__ void fdct_block(FdctArgsPtr a, const typename SourceOf<SRC>::Args& src, const FdctWork& g,
                                           int rx, int ry) {
  using IN = SourceOf<SRC>;
  static_assert(CS == 0 || !IN::kYuv, "YUV sources bring their own chroma");
  int d[64];
  int gb, c;
  bool dummy;
  if constexpr (CS != 0) {
    using SG = SubGeom<CS>;
    __shared__ u32 s_c[SG::MPW * SG::STRIDE];
    const int ml = threadIdx.x / SG::BPM, p = threadIdx.x - ml * SG::BPM;
    gb = g.wg * (SG::MPW * SG::BPM) + threadIdx.x;
    const bool act = ml < SG::MPW && gb < g.nblocks;
    const int mcu = g.wg * SG::MPW + ml;
    const int mx = mcu % g.mcux, my = mcu / g.mcux;
    c = p < SG::HV ? 0 : p - SG::HV + 1;
    dummy = false;  // a chroma block of an MCU is always real: mcux = bw[1], mcuy = bh[1]
    if (act && c == 0) {
      const typename IN::Item s = fdct_item<IN, ROI>(src, g.img, rx, ry, a->H, a->V);
      const int w = g.cw0, h = g.ch0;
      const int bx = mx * 2 + (p & 1), by = my * SG::V + (p >> 1);
      dummy = bx >= g.bw0 || by >= g.bh0;
      u32 cq[2][SG::NQ];
      // A dummy block codes the block whose DC it copies (jccoefct: the block to its left, for a dummy row the last block
      // of the row above in this MCU) but still owns the chroma of its own quadrant, and at 4:2:0 the bottom blocks
      // replicate rows for chroma in another way than for luma: those few take their chroma from a pass of its own.
      // It comes first, while d is not live yet.
      const bool own = dummy || (CS == 2 && by * 8 + 8 > h);
      u32 cown[2][SG::NQ] = {};
      if (own)
        load_quadrant<IN, CS, false, true, true>(src, s, bx * 8, by * 8, w, h, g.ch1, d, cown);
      int lx = bx, ly = by;
      if (by >= g.bh0) {
        lx = mx * 2 + 1;
        ly = g.bh0 - 1;
      }
      lx = min(lx, g.bw0 - 1);
      load_quadrant<IN, CS, true, true, false>(src, s, lx * 8, ly * 8, w, h, g.ch1, d, cq);
      u32* o = s_c + ml * SG::STRIDE + p * SG::NQ;
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int i = 0; i < SG::NQ; ++i)
          o[k * SG::HV * SG::NQ + i] = own ? cown[k][i] : cq[k][i];
    }
    __syncthreads();
    if (!act)
      return;
    if (c) {
      const u32* in = s_c + ml * SG::STRIDE + (c - 1) * SG::HV * SG::NQ;
#pragma unroll
      for (int q = 0; q < SG::HV; ++q)
#pragma unroll
        for (int i = 0; i < SG::NQ; ++i) {
          const u32 v = in[q * SG::NQ + i];
#pragma unroll
          for (int j = 0; j < 4; ++j)
            d[8 * (SG::NQ * (q >> 1) + i) + 4 * (q & 1) + j] = (int)((v >> (8 * j)) & 0xFF) - 128;
        }
    }
  } else {
    gb = g.wg * 256 + threadIdx.x;
    if (gb >= g.nblocks)
      return;
    const typename IN::Item s = fdct_item<IN, ROI>(src, g.img, rx, ry, a->H, a->V);
    const int mcu = gb / a->bpm, p = gb - mcu * a->bpm;
    const int mx = mcu % g.mcux, my = mcu / g.mcux;
    c = p < a->HV ? 0 : p - a->HV + 1;
    int bx = c ? mx : mx * a->H + p % a->H;
    int by = c ? my : my * a->V + p / a->H;
    const int bw = c ? g.bw1 : g.bw0, bh = c ? g.bh1 : g.bh0;
    const int cw = c ? g.cw1 : g.cw0, ch = c ? g.ch1 : g.ch0;
    // a dummy block of a partial MCU computes the block whose DC it copies (jccoefct): the block to its left, for a
    // dummy row the last block of the row above in this MCU -- always a real block after clamping
    dummy = bx >= bw || by >= bh;
    if (by >= bh) {
      bx = c ? mx : mx * a->H + a->H - 1;
      by = bh - 1;
    }
    bx = min(bx, bw - 1);

    const int x0 = bx * 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int y = min(by * 8 + r, ch - 1);
      int* v = d + 8 * r;
      if (IN::kYuv) {
        IN::comp_row(src, s, c, y, x0, cw, v);
      } else {
        int R[8], G[8], B[8];
        IN::rgb_row(src, s, y, x0, cw, R, G, B);
        // jccolor rgb_ycc_convert: this lane's component only
        const int kr = c == 0 ? fix16(0.299) : c == 1 ? -fix16(0.16874) : fix16(0.5);
        const int kg = c == 0 ? fix16(0.587) : c == 1 ? -fix16(0.33126) : -fix16(0.41869);
        const int kb = c == 0 ? fix16(0.114) : c == 1 ? fix16(0.5) : -fix16(0.08131);
        const int off = c == 0 ? (1 << 15) : (128 << 16) + (1 << 15) - 1;
#pragma unroll
        for (int i = 0; i < 8; ++i)
          v[i] = (kr * R[i] + kg * G[i] + kb * B[i] + off) >> 16;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i)
        v[i] -= 128;
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r)
    fdct_pass<true, 1>(d + 8 * r);
#pragma unroll
  for (int col = 0; col < 8; ++col)
    fdct_pass<false, 8>(d + col);

  // quantise: (|x| + corr) * recip >> shift == round_half_away(|x| / 8q) for every |x| < 2^15 (test_jpeg_host)
  const int t = c ? 1 : 0;
  u32 out[32];
#pragma unroll
  for (int k = 0; k < 64; ++k) {
    const int x = d[kZigzag[k]];
    const u32 recip = t ? a->recip[1][kZigzag[k]] : a->recip[0][kZigzag[k]];
    const u32 cs = t ? a->corr_shift[1][kZigzag[k]] : a->corr_shift[0][kZigzag[k]];
    const u32 m = (u32)abs(x);
    const int q = (int)(((m + (cs & 0xFFFF)) * recip) >> (cs >> 16));
    int v = x < 0 ? -q : q;
    if (dummy && k)
      v = 0;
    if (k & 1)
      out[k / 2] |= (u32)(v & 0xFFFF) << 16;
    else
      out[k / 2] = (u32)(v & 0xFFFF);
  }
  uint4* dst = (uint4*)(g.coef + (size_t)gb * 64);
#pragma unroll
  for (int i = 0; i < 8; ++i)
    dst[i] = make_uint4(out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]);
}


template <int SRC, int CS>
__global__ void __launch_bounds__(256) k_jpeg_fdct(const FdctArgs a, const typename SourceOf<SRC>::Args src) {
  const FdctWork g = {(int)blockIdx.y, (int)blockIdx.x, a.coef + (size_t)blockIdx.y * a.nblocks * 64, a.mcux, a.nblocks,
                      a.cw[0], a.cw[1], a.ch[0], a.ch[1], a.bw[0], a.bw[1], a.bh[0], a.bh[1]};
  fdct_block<SRC, CS, false>(fdct_args(), src, g, 0, 0);
}

template <int SRC, int CS>
__global__ void __launch_bounds__(256) k_jpeg_fdct_roi(const FdctArgs a, const typename SurfIn<SRC>::Args src,
                                                       const vali_jpeg_item* __restrict__ items, int n) {
  const int i = find_item<&vali_jpeg_item::wg_fdct>(items, n, blockIdx.x);
  const vali_jpeg_item* it = items + i;
  const FdctWork g = {i, (int)(blockIdx.x - it->wg_fdct), a.coef + it->block_first * 64, it->mcux, it->nblocks,
                      it->cw[0], it->cw[1], it->ch[0], it->ch[1], it->bw[0], it->bw[1], it->bh[0], it->bh[1]};
  fdct_block<SRC, CS, true>(fdct_args(), src, g, it->x, it->y);
}

// ---- entropy coding: what k_jpeg_hist and k_jpeg_huff share -------------------------------------------------------------
__device__ __forceinline__ int nbits(int v) { return v ? 32 - __clz(abs(v)) : 0; }

// OR `len` (1..32) bits of `code` into the big-endian bit stream at bit `pos`: one or two ds_or_b32
__device__ __forceinline__ void put_bits(u32* buf, u32 pos, u32 code, int len) {
  const u32 w = pos >> 5, off = pos & 31;
  const uint64_t x = (uint64_t)code << (64 - off - len);
  atomicOr(&buf[w], (u32)(x >> 32));
  if ((u32)x)
    atomicOr(&buf[w + 1], (u32)x);
}

__device__ __forceinline__ u32 wave_incl_scan(u32 v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u32 o = __shfl_up(v, d, 64);
    if (lane >= d)
      v += o;
  }
  return v;
}

// What code_block does with the symbols of a block: BLOCK_BITS returns their bits, BLOCK_EMIT writes them at bit `pos`,
// BLOCK_COUNT counts them (dc and ac are then the histograms of the block's tables, and nothing is read from them)
enum BlockMode { BLOCK_BITS = 0, BLOCK_EMIT = 1, BLOCK_COUNT = 2 };

// the table entry of `sym`; BLOCK_COUNT: one more of it, and no entry
template <int MODE>
__device__ __forceinline__ u32 symbol(u32* table, int sym) {
  if (MODE == BLOCK_COUNT) {
    atomicAdd(&table[sym], 1u);
    return 0;
  }
  return table[sym];
}

template <int MODE>
__device__ __forceinline__ u32 code_block(const int* z, int diff, u32* dc, u32* ac, u32* buf, u32 pos) {
  constexpr bool EMIT = MODE == BLOCK_EMIT;
  u32 n = 0;
  {
    const int s = nbits(diff);
    const u32 e = symbol<MODE>(dc, s);
    const int len = (int)(e & 0xFF) + s;
    if (EMIT)
      put_bits(buf, pos, ((e >> 8) << s) | ((u32)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1)), len);
    n += len;
  }
  int last = 0;
#pragma unroll
  for (int k = 1; k < 64; ++k) {
    const int v = z[k];
    if (v) {
      int run = k - last - 1;
      for (; run > 15; run -= 16) {
        const u32 e = symbol<MODE>(ac, 0xF0);
        if (EMIT)
          put_bits(buf, pos + n, e >> 8, (int)(e & 0xFF));
        n += e & 0xFF;
      }
      const int s = nbits(v);
      const u32 e = symbol<MODE>(ac, (run << 4) | s);
      const int len = (int)(e & 0xFF) + s;
      if (EMIT)
        put_bits(buf, pos + n, ((e >> 8) << s) | ((u32)(v < 0 ? v - 1 : v) & ((1u << s) - 1)), len);
      n += len;
      last = k;
    }
  }
  if (last < 63) {
    const u32 e = symbol<MODE>(ac, 0);
    if (EMIT)
      put_bits(buf, pos + n, e >> 8, (int)(e & 0xFF));
    n += e & 0xFF;
  }
  return n;
}

// lane's block of a restart segment that starts at block `base` of image `img`: its 64 coefficients (zero when the
// lane is past the segment's `nb` blocks) and its DC difference.  DC prediction comes from the previous block of the
// same component and restarts with the segment.  Returns whether the block is a chroma block.
__device__ __forceinline__ bool segment_block(const int16_t* coef, size_t img, int nblocks, int base, int nb, int bpm,
                                              int HV, int lane, int* z, int* diff) {
  if (lane < nb) {
    const uint4* src = (const uint4*)(coef + (img * nblocks + base + lane) * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint4 q = src[i];
      const u32 w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        z[8 * i + 2 * j] = (int)(int16_t)(w[j] & 0xFFFF);
        z[8 * i + 2 * j + 1] = (int)(int16_t)(w[j] >> 16);
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 64; ++k)
      z[k] = 0;
  }
  const int p = lane % bpm;  // segments start on an MCU
  const bool chroma = p >= HV;
  const int prev = lane - (chroma ? bpm : p > 0 ? 1 : bpm - HV + 1);
  const int pdc = __shfl(z[0], prev < 0 ? lane : prev, 64);
  *diff = z[0] - (prev < 0 ? 0 : pdc);
  return chroma;
}

// ---- k_jpeg_hist -----------------------------------------------------------------------------------------------------
struct HistArgs {
  const int16_t* coef;
  u32* hist;  // image i, table t (DHT order), symbol v: [(i * 4 + t) * 256 + v], zero before the launch
  int nblocks, nseg, bpm, HV, bps;
};

// Counts fit 32 bits: an image's output slot is addressed with 32 bits (jpeg_geom), a segment slot takes 416 bytes a
// block, and a block has at most 64 symbols of one table.
// workgroup `wg` of an image of nseg segments / nblocks blocks whose coefficients are image `img` of `coef` (images
// nblocks blocks apart); g: the image's four histograms
__device__ __forceinline__ void hist_segments(const HistArgs& a, const int16_t* coef, size_t img, int nblocks, int nseg,
                                              int wg, u32* g) {
  __shared__ u32 s_hist[4][256];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  for (int i = tid; i < 4 * 256; i += 64 * kHistWaves)
    s_hist[i >> 8][i & 255] = 0;
  __syncthreads();
  const int seg0 = (wg * kHistWaves + wid) * kHistSegsPerWave;
  const int seg1 = min(seg0 + kHistSegsPerWave, nseg);
  for (int seg = seg0; seg < seg1; ++seg) {  // wave-uniform
    const int base = seg * a.bps;
    const int nb = min(a.bps, nblocks - base);
    int z[64], diff;
    const bool chroma = segment_block(coef, img, nblocks, base, nb, a.bpm, a.HV, lane, z, &diff);
    if (lane < nb)
      code_block<BLOCK_COUNT>(z, diff, s_hist[chroma ? 2 : 0], s_hist[chroma ? 3 : 1], nullptr, 0);
  }
  __syncthreads();
  for (int i = tid; i < 4 * 256; i += 64 * kHistWaves) {
    const u32 c = s_hist[i >> 8][i & 255];
    if (c)
      atomicAdd(&g[i], c);  // integer adds: the sum does not depend on their order
  }
}

__global__ void __launch_bounds__(64 * kHistWaves) k_jpeg_hist(const HistArgs a) {
  const size_t img = blockIdx.y;
  hist_segments(a, a.coef, img, a.nblocks, a.nseg, blockIdx.x, a.hist + img * (4 * 256));
}

// a.nblocks and a.nseg are not read: they are the item's
__global__ void __launch_bounds__(64 * kHistWaves) k_jpeg_hist_roi(const HistArgs a,
                                                                   const vali_jpeg_item* __restrict__ items, int n) {
  const int i = find_item<&vali_jpeg_item::wg_hist>(items, n, blockIdx.x);
  const vali_jpeg_item* it = items + i;
  hist_segments(a, a.coef + it->block_first * 64, 0, it->nblocks, it->nseg, (int)(blockIdx.x - it->wg_hist),
                a.hist + (size_t)i * (4 * 256));
}

// ---- k_jpeg_tables ---------------------------------------------------------------------------------------------------
struct TablesArgs {
  const u32* hist;
  u32* codes;   // symbol -> (code << 8) | length, 0 for a symbol the image does not have: what k_jpeg_huff reads
  u8* dht;      // table (i * 4 + t): kDhtSlot bytes: class << 4 | id, BITS, HUFFVAL
  u32* dhtlen;  // and how many of them: 17 + number of values
};

// libjpeg's jpeg_gen_optimal_table.  Symbol v lives in lane v % 64, register v / 64; symbol 256, in lane 0, is the
// pseudo-symbol of count 1 that keeps the all-ones code free.  Each merge joins the two least frequent live entries:
// c1 is the largest index among the minima, c2 the largest among the minima of the rest, which is the order of the key
// (count << 9 | 511 - index); the sum stays at c1.  Every symbol remembers the entry its subtree is summed in, so that
// a merge deepens all symbols of both subtrees at once: the code length is the depth in the merge tree.
__global__ void __launch_bounds__(64) k_jpeg_tables(const TablesArgs a) {
  constexpr int kMaxLen = 257;  // no code of 257 symbols is deeper than 256
  __shared__ u32 s_len[kMaxLen + 1];          // codes of each length
  __shared__ u32 s_first[18], s_start[18];    // Annex C: first code of a length, and its place in HUFFVAL
  const int lane = threadIdx.x;
  const int t = blockIdx.x;
  const size_t tab = (size_t)blockIdx.y * 4 + t;
  const u32* h = a.hist + tab * 256;
  constexpr uint64_t kNone = ~0ull;

  u32 f[5];
  int grp[5], len[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    f[j] = j < 4 ? h[lane + 64 * j] : lane == 0 ? 1u : 0u;
    grp[j] = lane + 64 * j;
    len[j] = 0;
  }
  for (int i = lane; i <= kMaxLen; i += 64)
    s_len[i] = 0;

  for (;;) {
    // the two smallest keys of the lane, then of the wave
    uint64_t k1 = kNone, k2 = kNone;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const uint64_t key = f[j] ? ((uint64_t)f[j] << 9) | (u32)(511 - (lane + 64 * j)) : kNone;
      k2 = min(k2, max(k1, key));
      k1 = min(k1, key);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t o1 = __shfl_xor(k1, d, 64), o2 = __shfl_xor(k2, d, 64);
      k2 = min(max(k1, o1), min(k2, o2));
      k1 = min(k1, o1);
    }
    if (k2 == kNone)  // one entry left: wave-uniform
      break;
    const int c1 = 511 - (int)(k1 & 511), c2 = 511 - (int)(k2 & 511);
    const u32 v2 = (u32)(k2 >> 9);
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int idx = lane + 64 * j;
      f[j] = idx == c1 ? f[j] + v2 : idx == c2 ? 0u : f[j];
      if (grp[j] == c1 || grp[j] == c2) {
        grp[j] = c1;
        ++len[j];
      }
    }
  }

  // BITS before limiting (the pseudo-symbol included) and the place of every symbol in HUFFVAL: by length, then by
  // value.  A length's symbols are found by ballots, register by register: that is their order by value.
  int maxlen = 0;
#pragma unroll
  for (int j = 0; j < 5; ++j)
    maxlen = max(maxlen, len[j]);
#pragma unroll
  for (int d = 1; d < 64; d <<= 1)
    maxlen = max(maxlen, __shfl_xor(maxlen, d, 64));
  const int pseudo = __shfl(len[4], 0, 64);
  const uint64_t below = (1ull << lane) - 1;
  int pos[4] = {0, 0, 0, 0};
  u32 nvals = 0;
  for (int l = 1; l <= maxlen; ++l) {
    u32 n = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint64_t m = __ballot(len[j] == l);
      if (len[j] == l)
        pos[j] = (int)(nvals + n) + __popcll(m & below);
      n += (u32)__popcll(m);
    }
    if (lane == 0)
      s_len[l] = n + (pseudo == l ? 1u : 0u);
    nvals += n;
  }
  __syncthreads();

  if (lane == 0) {
    // Annex K.2, figure K.3 (jchuff): no code longer than 16 bits
    for (int i = maxlen; i > 16; --i) {
      while (s_len[i] > 0) {
        int j = i - 2;
        while (j > 0 && s_len[j] == 0)
          --j;
        s_len[i] -= 2;
        s_len[i - 1] += 1;
        s_len[j + 1] += 2;
        s_len[j] -= 1;
      }
    }
    int i = min(maxlen, 16);
    while (i > 0 && s_len[i] == 0)
      --i;
    if (i > 0)
      s_len[i] -= 1;  // the pseudo-symbol's code
    u32 code = 0, start = 0;
    for (int l = 1; l <= 16; ++l) {
      s_first[l] = code;
      s_start[l] = start;
      code = (code + s_len[l]) << 1;
      start += s_len[l];
    }
    s_start[17] = start;
  }
  __syncthreads();

  u8* dht = a.dht + tab * kDhtSlot;
  u32* codes = a.codes + tab * 256;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    u32 e = 0;
    if (len[j] > 0) {
      const u32 p = (u32)pos[j];
      for (int l = 1; l <= 16; ++l)
        if (p >= s_start[l] && p < s_start[l + 1])
          e = ((s_first[l] + p - s_start[l]) << 8) | (u32)l;
      dht[17 + p] = (u8)(lane + 64 * j);
    }
    codes[lane + 64 * j] = e;
  }
  if (lane == 0) {
    dht[0] = (u8)(((t & 1) << 4) | (t >> 1));  // DHT order: 0x00, 0x10, 0x01, 0x11
    a.dhtlen[tab] = 17 + nvals;
  } else if (lane <= 16) {
    dht[lane] = (u8)s_len[lane];
  }
}

// ---- k_jpeg_huff -----------------------------------------------------------------------------------------------------
struct HuffArgs {
  const int16_t* coef;
  const u32* codes;  // image i, table t (DHT order): [(i * 4 + t) * 256]; null: Annex K
  u32* seglen;  // image i, segment s: [i * nseg + s]
  u8* slots;    // slot bytes per segment, same order
  int nblocks, nseg, bpm, HV, bps;
  u32 slot;
};

// segment `seg` of an image of nblocks blocks whose coefficients are image `img` of `coef` (images nblocks blocks apart),
// with the tables `codes` (null: Annex K), into the slot `out`; its length goes to *seglen
__device__ __forceinline__ void huff_segment(const HuffArgs& a, const int16_t* coef, size_t img, int nblocks, int seg,
                                             const u32* codes, u8* out, u32* seglen) {
  __shared__ u32 s_codes[4][256];
  __shared__ u32 s_bits[kHuffWords];
  const int lane = threadIdx.x;
  if (codes) {  // the image's own tables (optimize = 1)
    for (int i = lane; i < 4 * 256; i += 64)
      s_codes[i >> 8][i & 255] = codes[i];
  } else {
    for (int i = lane; i < 4 * 256; i += 64)
      s_codes[i >> 8][i & 255] = d_codes[i >> 8].e[i & 255];
  }

  const int base = seg * a.bps;
  const int nb = min(a.bps, nblocks - base);
  const bool act = lane < nb;
  int z[64], diff;
  const bool chroma = segment_block(coef, img, nblocks, base, nb, a.bpm, a.HV, lane, z, &diff);
  __syncthreads();  // code tables

  u32* dc = s_codes[chroma ? 2 : 0];
  u32* ac = s_codes[chroma ? 3 : 1];
  const u32 mine = act ? code_block<BLOCK_BITS>(z, diff, dc, ac, nullptr, 0) : 0;
  const u32 incl = wave_incl_scan(mine, lane);
  const u32 total = __shfl(incl, 63, 64);
  const int nwords = (int)((total + 7) >> 5) + 2;
  for (int i = lane; i < nwords; i += 64)
    s_bits[i] = 0;
  __syncthreads();
  if (act)
    code_block<BLOCK_EMIT>(z, diff, dc, ac, s_bits, incl - mine);
  const u32 pad = (8 - (total & 7)) & 7;
  if (lane == 0 && pad)
    put_bits(s_bits, total, (1u << pad) - 1, (int)pad);
  __syncthreads();

  // byte stuffing: 4 bytes per lane per step, 0xFF counts prefix-summed across the wave
  const u32 nbytes = (total + pad) >> 3;
  u32 opos = 0;
  for (u32 b0 = 0; b0 < nbytes; b0 += 256) {
    const u32 bi = b0 + 4 * lane;
    const u32 word = bi < nbytes ? s_bits[bi >> 2] : 0u;
    const int nv = bi < nbytes ? (int)min(4u, nbytes - bi) : 0;
    u32 ff = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      ff += (k < nv && ((word >> (24 - 8 * k)) & 0xFF) == 0xFF) ? 1u : 0u;
    const u32 fincl = wave_incl_scan(ff, lane);
    const u32 ftot = __shfl(fincl, 63, 64);
    u8* o = out + opos + 4 * lane + (fincl - ff);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < nv) {
        const u32 byte = (word >> (24 - 8 * k)) & 0xFF;
        *o++ = (u8)byte;
        if (byte == 0xFF)
          *o++ = 0;
      }
    }
    opos += min(256u, nbytes - b0) + ftot;
  }
  if (lane == 0)
    *seglen = opos;
}

__global__ void __launch_bounds__(64) k_jpeg_huff(const HuffArgs a) {
  const int seg = blockIdx.x;
  const size_t img = blockIdx.y;
  const size_t k = img * a.nseg + seg;
  huff_segment(a, a.coef, img, a.nblocks, seg, a.codes ? a.codes + img * (4 * 256) : nullptr, a.slots + k * a.slot,
               a.seglen + k);
}

// one workgroup per segment of every item: blockIdx.x is the segment's place in the length and slot areas as well
// (wg_seg = seg_first).  a.nblocks and a.nseg are not read: they are the item's
__global__ void __launch_bounds__(64) k_jpeg_huff_roi(const HuffArgs a, const vali_jpeg_item* __restrict__ items,
                                                      int n) {
  const int i = find_item<&vali_jpeg_item::wg_seg>(items, n, blockIdx.x);
  const vali_jpeg_item* it = items + i;
  const size_t k = blockIdx.x;
  huff_segment(a, a.coef + it->block_first * 64, 0, it->nblocks, (int)(blockIdx.x - it->wg_seg),
               a.codes ? a.codes + (size_t)i * (4 * 256) : nullptr, a.slots + k * a.slot, a.seglen + k);
}

// ---- k_jpeg_offsets ----------------------------------------------------------------------------------------------------
// the bytes in front of an image's entropy data when its tables are its own: DHT (marker, length, four parts), DRI, SOS
__device__ __forceinline__ u32 dht_bytes(const u32* dhtlen, size_t img) {
  const uint4 l = *(const uint4*)(dhtlen + img * 4);
  return 4 + l.x + l.y + l.z + l.w;
}

// one image: seglen and segoff are its entries, `carry` the bytes in front of its entropy data
__device__ __forceinline__ void image_offsets(const u32* seglen, u32* segoff, u32* size, int nseg, u32 carry) {
  __shared__ u32 s_wave[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  for (int s0 = 0; s0 < nseg; s0 += 256) {
    const int s = s0 + tid;
    const u32 v = s < nseg ? seglen[s] + 2u : 0u;  // + RST marker
    const u32 incl = wave_incl_scan(v, lane);
    if (lane == 63)
      s_wave[wid] = incl;
    __syncthreads();
    u32 before = 0, chunk = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      before += w < wid ? s_wave[w] : 0u;
      chunk += s_wave[w];
    }
    if (s < nseg)
      segoff[s] = carry + before + incl - v;
    carry += chunk;
    __syncthreads();
  }
  if (tid == 0)
    *size = carry - 2u;  // no marker after the last segment
}

__global__ void __launch_bounds__(256) k_jpeg_offsets(const u32* seglen, u32* segoff, u32* sizes, int nseg,
                                                      const u32* dhtlen) {
  const size_t img = blockIdx.x;
  image_offsets(seglen + img * nseg, segoff + img * nseg, sizes + img, nseg,
                dhtlen ? dht_bytes(dhtlen, img) + kDriSosBytes : 0u);
}

__global__ void __launch_bounds__(256) k_jpeg_offsets_roi(const u32* seglen, u32* segoff, u32* sizes,
                                                          const vali_jpeg_item* __restrict__ items,
                                                          const u32* dhtlen) {
  const size_t img = blockIdx.x;
  const vali_jpeg_item* it = items + img;
  image_offsets(seglen + it->seg_first, segoff + it->seg_first, sizes + img, it->nseg,
                dhtlen ? dht_bytes(dhtlen, img) + kDriSosBytes : 0u);
}

// ---- k_jpeg_assemble ---------------------------------------------------------------------------------------------------
struct AsmArgs {
  const u32* seglen;
  const u32* segoff;
  const u8* slots;
  u8* out;
  size_t out_stride;
  int nseg;
  u32 slot;
  const u8* dht;      // optimize = 1: the parts of the image's DHT and their lengths (k_jpeg_tables); else null
  const u32* dhtlen;
  int restart_interval;
};

// segment `seg` of the nseg of image `img`, entry k of the length, offset and slot areas, into the image's bytes at `o`
__device__ __forceinline__ void assemble_segment(const AsmArgs& a, size_t img, int seg, int nseg, size_t k, u8* o) {
  const u32 len = a.seglen[k];
  const u8* src = a.slots + k * a.slot;
  u8* dst = o + a.segoff[k];
  for (u32 i = 4 * threadIdx.x; i < len; i += 4 * 256) {
    const u32 v = *(const u32*)(src + i);  // slots are 16-byte aligned and a multiple of 16 long
    const u32 n = min(4u, len - i);
#pragma unroll
    for (u32 j = 0; j < 4; ++j)
      if (j < n)
        dst[i + j] = (u8)(v >> (8 * j));
  }
  if (threadIdx.x == 0 && seg + 1 < nseg) {
    dst[len] = 0xFF;
    dst[len + 1] = (u8)(0xD0 + (seg & 7));
  }
  if (a.dht && seg == 0) {  // the image's own DHT, then DRI and SOS as write_header lays them out
    u32 at = 4;
    for (int t = 0; t < 4; ++t) {
      const u32 n = a.dhtlen[img * 4 + t];
      const u8* part = a.dht + (img * 4 + t) * kDhtSlot;
      for (u32 i = threadIdx.x; i < n; i += 256)
        o[at + i] = part[i];
      at += n;
    }
    if (threadIdx.x == 0) {
      o[0] = 0xFF, o[1] = 0xC4, o[2] = (u8)((at - 2) >> 8), o[3] = (u8)(at - 2);
      o += at;
      o[0] = 0xFF, o[1] = 0xDD, o[2] = 0, o[3] = 4;
      o[4] = (u8)(a.restart_interval >> 8), o[5] = (u8)a.restart_interval;
      o[6] = 0xFF, o[7] = 0xDA, o[8] = 0, o[9] = 12;
      o[10] = 3, o[11] = 1, o[12] = 0x00, o[13] = 2, o[14] = 0x11, o[15] = 3, o[16] = 0x11;
      o[17] = 0, o[18] = 63, o[19] = 0;
    }
  }
}

__global__ void __launch_bounds__(256) k_jpeg_assemble(const AsmArgs a) {
  const int seg = blockIdx.x;
  const size_t img = blockIdx.y;
  assemble_segment(a, img, seg, a.nseg, img * a.nseg + seg, a.out + img * a.out_stride);
}

// as k_jpeg_huff_roi: blockIdx.x is the segment's entry.  a.nseg and a.out_stride are not read
__global__ void __launch_bounds__(256) k_jpeg_assemble_roi(const AsmArgs a, const vali_jpeg_item* __restrict__ items,
                                                           int n) {
  const int i = find_item<&vali_jpeg_item::wg_seg>(items, n, blockIdx.x);
  const vali_jpeg_item* it = items + i;
  assemble_segment(a, (size_t)i, (int)(blockIdx.x - it->wg_seg), it->nseg, blockIdx.x, a.out + it->out_offset);
}

// ---- host ----------------------------------------------------------------------------------------------------------------
void put16(u8* p, int v) {
  p[0] = (u8)(v >> 8);
  p[1] = (u8)v;
}

size_t write_header(int w, int h, const vali_jpeg_params* p, u8* o) {
  size_t n = 0;
  auto seg = [&](int marker, int payload) {
    o[n] = 0xFF, o[n + 1] = (u8)marker;
    put16(o + n + 2, payload + 2);
    n += 4;
  };
  o[n++] = 0xFF, o[n++] = 0xD8;
  static const u8 jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  seg(0xE0, 14);
  memcpy(o + n, jfif, 14), n += 14;
  seg(0xDB, 2 * 65);
  for (int t = 0; t < 2; ++t) {
    o[n++] = (u8)t;
    for (int k = 0; k < 64; ++k)
      o[n++] = p->qtable[t][kZigzag[k]];
  }
  seg(0xC0, 15);
  o[n++] = 8;
  put16(o + n, h), n += 2;
  put16(o + n, w), n += 2;
  const u8 comps[10] = {3, 1, (u8)((p->h_samp << 4) | p->v_samp), 0, 2, 0x11, 1, 3, 0x11, 1};
  memcpy(o + n, comps, 10), n += 10;
  if (p->optimize)  // DHT, DRI and SOS come from the device, with the image's own tables
    return n;
  int dht = 0;
  for (int t = 0; t < 4; ++t)
    dht += 17 + kHuff[t].nvals;
  seg(0xC4, dht);
  static const u8 cls_id[4] = {0x00, 0x10, 0x01, 0x11};
  for (int t = 0; t < 4; ++t) {
    o[n++] = cls_id[t];
    memcpy(o + n, kHuff[t].bits, 16), n += 16;
    memcpy(o + n, kHuff[t].vals, kHuff[t].nvals), n += kHuff[t].nvals;
  }
  seg(0xDD, 2);
  put16(o + n, p->restart_interval), n += 2;
  seg(0xDA, 10);
  const u8 sos[10] = {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
  memcpy(o + n, sos, 10), n += 10;
  return n;
}

constexpr size_t kHeaderMax = 1024;

// jcdctmgr compute_reciprocal of the divisor 8 q
void reciprocal(int q, u32* recip, u32* corr_shift) {
  const u32 d = 8u * (u32)q;
  int b = 31 - __builtin_clz(d);
  int r = 16 + b;
  u32 fq = (u32)((1ull << r) / d), fr = (u32)((1ull << r) % d), c = d / 2;
  if (fr == 0) {
    fq >>= 1;
    --r;
  } else if (fr <= d / 2) {
    ++c;
  } else {
    ++fq;
  }
  *recip = fq;
  *corr_shift = c | ((u32)r << 16);
}

// an RGB source with chroma sampling cs: 0 = 1x1, 1 = 2x1, 2 = 2x2
template <int SRC>
void launch_fdct(int cs, dim3 grid, hipStream_t s, const FdctArgs& f, const typename SourceOf<SRC>::Args& src) {
  if (cs == 0)
    hipLaunchKernelGGL((k_jpeg_fdct<SRC, 0>), grid, dim3(256), 0, s, f, src);
  else if (cs == 1)
    hipLaunchKernelGGL((k_jpeg_fdct<SRC, 1>), grid, dim3(256), 0, s, f, src);
  else
    hipLaunchKernelGGL((k_jpeg_fdct<SRC, 2>), grid, dim3(256), 0, s, f, src);
}

// a tensor source: the channels are colours (coded with chroma sampling cs) or Y, Cb, Cr as they are
template <int DT, bool PACKED>
void launch_fdct_tensor(bool yuv, int cs, dim3 grid, hipStream_t s, const FdctArgs& f, const TensorArgs& src) {
  if (yuv)
    hipLaunchKernelGGL((k_jpeg_fdct<tensor_src(DT, PACKED, true), 0>), grid, dim3(256), 0, s, f, src);
  else
    launch_fdct<tensor_src(DT, PACKED, false)>(cs, grid, s, f, src);
}

template <int DT>
void launch_fdct_tensor(bool packed, bool yuv, int cs, dim3 grid, hipStream_t s, const FdctArgs& f,
                        const TensorArgs& src) {
  if (packed)
    launch_fdct_tensor<DT, true>(yuv, cs, grid, s, f, src);
  else
    launch_fdct_tensor<DT, false>(yuv, cs, grid, s, f, src);
}

// what the surface and the tensor entry points share: everything but the arguments' checks and the first launch
struct JpegLaunch {
  FdctArgs f;
  HistArgs hi;   // optimize = 1 only, as tb
  TablesArgs tb;
  HuffArgs hf;
  AsmArgs as;
  int cs;      // chroma sampling of an RGB source: 0 = 1x1, 1 = 2x1, 2 = 2x2
  dim3 fgrid;
};

int jpeg_launch_prepare(const char* fn, int n, const JpegGeom& g, const vali_jpeg_params* params, void* workspace,
                        size_t ws_bytes, uint8_t* d_out, size_t out_stride, JpegLaunch* l) {
  if ((((uintptr_t)workspace) & 255) != 0)
    return fail(VALI_ERR_INVALID_ARG, "%s: workspace not 256-byte aligned", fn);
  if (ws_bytes < g.ws_bytes)
    return fail(VALI_ERR_INVALID_ARG, "%s: workspace below vali_jpeg_workspace_size", fn);
  if (out_stride < jpeg_capacity(g))
    return fail(VALI_ERR_INVALID_ARG, "%s: out_stride below vali_jpeg_stream_capacity", fn);
  u8* ws = (u8*)workspace;
  FdctArgs& f = l->f;
  f = {};
  f.coef = (int16_t*)ws;
  f.H = g.H, f.V = g.V, f.HV = g.H * g.V, f.bpm = g.bpm, f.mcux = g.mcux, f.nblocks = g.nblocks;
  for (int c = 0; c < 3; ++c)
    f.cw[c] = g.cw[c], f.ch[c] = g.ch[c], f.bw[c] = g.bw[c], f.bh[c] = g.bh[c];
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 64; ++k)
      reciprocal(params->qtable[t][k], &f.recip[t][k], &f.corr_shift[t][k]);
  const bool opt = g.optimize != 0;
  u32* codes = opt ? (u32*)(ws + g.codes_at) : nullptr;
  u8* dht = opt ? ws + g.dht_at : nullptr;
  u32* dhtlen = opt ? (u32*)(ws + g.dhtlen_at) : nullptr;
  l->hi = {(const int16_t*)ws, opt ? (u32*)(ws + g.hist_at) : nullptr, g.nblocks, g.nseg, g.bpm, g.H * g.V, g.bps};
  l->tb = {l->hi.hist, codes, dht, dhtlen};
  l->hf = {(const int16_t*)ws, codes, (u32*)(ws + g.len_at), ws + g.slot_at, g.nblocks, g.nseg, g.bpm, g.H * g.V,
           g.bps, (u32)g.slot};
  l->as = {(const u32*)(ws + g.len_at), (const u32*)(ws + g.off_at), ws + g.slot_at, d_out, out_stride, g.nseg,
           (u32)g.slot, dht, dhtlen, g.R};
  // a subsampled RGB source: workgroups of whole MCUs (fdct_subsampled)
  l->cs = jpeg_is_rgb(params->format) ? g.H * g.V / 2 : 0;
  const int per_wg = l->cs ? 256 / g.bpm * g.bpm : 256;
  l->fgrid = dim3((g.nblocks + per_wg - 1) / per_wg, n);
  return VALI_OK;
}

// k_jpeg_huff, k_jpeg_offsets, k_jpeg_assemble, after the source's k_jpeg_fdct; with the image's own tables the
// histograms are zeroed and k_jpeg_hist and k_jpeg_tables run first
int jpeg_launch_rest(const char* fn, int n, const JpegLaunch& l, uint32_t* d_sizes, hipStream_t s) {
  // VALI_LAUNCH_CHECK's message under the entry point's name
  hipError_t e;
  if (l.hi.hist) {
    if ((e = hipMemsetAsync(l.hi.hist, 0, (size_t)n * 4 * 256 * sizeof(u32), s)) != hipSuccess)
      return fail(VALI_ERR_RUNTIME, "%s: clearing the histograms failed: %s", fn, hipGetErrorString(e));
    const int per_wg = kHistWaves * kHistSegsPerWave;
    hipLaunchKernelGGL(k_jpeg_hist, dim3((l.hi.nseg + per_wg - 1) / per_wg, n), dim3(64 * kHistWaves), 0, s, l.hi);
    if ((e = hipGetLastError()) != hipSuccess)
      return fail(VALI_ERR_RUNTIME, "%s: kernel launch failed: %s", fn, hipGetErrorString(e));
    hipLaunchKernelGGL(k_jpeg_tables, dim3(4, n), dim3(64), 0, s, l.tb);
    if ((e = hipGetLastError()) != hipSuccess)
      return fail(VALI_ERR_RUNTIME, "%s: kernel launch failed: %s", fn, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(k_jpeg_huff, dim3(l.hf.nseg, n), dim3(64), 0, s, l.hf);
  if ((e = hipGetLastError()) != hipSuccess)
    return fail(VALI_ERR_RUNTIME, "%s: kernel launch failed: %s", fn, hipGetErrorString(e));
  hipLaunchKernelGGL(k_jpeg_offsets, dim3(n), dim3(256), 0, s, l.as.seglen, (u32*)l.as.segoff, (u32*)d_sizes,
                     l.hf.nseg, l.as.dhtlen);
  if ((e = hipGetLastError()) != hipSuccess)
    return fail(VALI_ERR_RUNTIME, "%s: kernel launch failed: %s", fn, hipGetErrorString(e));
  hipLaunchKernelGGL(k_jpeg_assemble, dim3(l.hf.nseg, n), dim3(256), 0, s, l.as);
  if ((e = hipGetLastError()) != hipSuccess)
    return fail(VALI_ERR_RUNTIME, "%s: kernel launch failed: %s", fn, hipGetErrorString(e));
  return VALI_OK;
}

// vali_jpeg_encode_rois: the same launches over flattened grids; every workgroup looks its image up in d_items
template <int SRC>
void launch_fdct_roi(int cs, u32 grid, hipStream_t s, const FdctArgs& f, const vali_surface* d_src,
                     const vali_jpeg_item* d_items, int n) {
  const typename SurfIn<SRC>::Args src = {d_src};
  if (cs == 0)
    hipLaunchKernelGGL((k_jpeg_fdct_roi<SRC, 0>), dim3(grid), dim3(256), 0, s, f, src, d_items, n);
  else if (cs == 1)
    hipLaunchKernelGGL((k_jpeg_fdct_roi<SRC, 1>), dim3(grid), dim3(256), 0, s, f, src, d_items, n);
  else
    hipLaunchKernelGGL((k_jpeg_fdct_roi<SRC, 2>), dim3(grid), dim3(256), 0, s, f, src, d_items, n);
}

int jpeg_launch_rest_roi(const char* fn, int n, const JpegLaunch& l, const RoiTotals& t, const vali_jpeg_item* d_items,
                         uint32_t* d_sizes, hipStream_t s) {
  hipError_t e;
  if (l.hi.hist) {
    if ((e = hipMemsetAsync(l.hi.hist, 0, (size_t)n * 4 * 256 * sizeof(u32), s)) != hipSuccess)
      return fail(VALI_ERR_RUNTIME, "%s: clearing the histograms failed: %s", fn, hipGetErrorString(e));
    hipLaunchKernelGGL(k_jpeg_hist_roi, dim3((u32)t.wg_hist), dim3(64 * kHistWaves), 0, s, l.hi, d_items, n);
    if ((e = hipGetLastError()) != hipSuccess)
      return fail(VALI_ERR_RUNTIME, "%s: kernel launch failed: %s", fn, hipGetErrorString(e));
    hipLaunchKernelGGL(k_jpeg_tables, dim3(4, n), dim3(64), 0, s, l.tb);
    if ((e = hipGetLastError()) != hipSuccess)
      return fail(VALI_ERR_RUNTIME, "%s: kernel launch failed: %s", fn, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(k_jpeg_huff_roi, dim3((u32)t.segs), dim3(64), 0, s, l.hf, d_items, n);
  if ((e = hipGetLastError()) != hipSuccess)
    return fail(VALI_ERR_RUNTIME, "%s: kernel launch failed: %s", fn, hipGetErrorString(e));
  hipLaunchKernelGGL(k_jpeg_offsets_roi, dim3(n), dim3(256), 0, s, l.as.seglen, (u32*)l.as.segoff, (u32*)d_sizes,
                     d_items, l.as.dhtlen);
  if ((e = hipGetLastError()) != hipSuccess)
    return fail(VALI_ERR_RUNTIME, "%s: kernel launch failed: %s", fn, hipGetErrorString(e));
  hipLaunchKernelGGL(k_jpeg_assemble_roi, dim3((u32)t.segs), dim3(256), 0, s, l.as, d_items, n);
  if ((e = hipGetLastError()) != hipSuccess)
    return fail(VALI_ERR_RUNTIME, "%s: kernel launch failed: %s", fn, hipGetErrorString(e));
  return VALI_OK;
}

} // namespace
} // namespace vali

using namespace vali;

extern "C" {

int vali_jpeg_params_init(int quality, int format, vali_jpeg_params* out) {
  VALI_REQUIRE(out, "null output");
  int H, V;
  if (!jpeg_sampling(format, &H, &V))
    return fail(VALI_ERR_UNSUPPORTED, "%s: format %d cannot be encoded", __func__, format);
  return vali_jpeg_params_init_sampled(quality, format, H, V, out);
}

int vali_jpeg_params_init_sampled(int quality, int format, int h_samp, int v_samp, vali_jpeg_params* out) {
  VALI_REQUIRE(out, "null output");
  int H, V;
  if (!jpeg_sampling(format, &H, &V))
    return fail(VALI_ERR_UNSUPPORTED, "%s: format %d cannot be encoded", __func__, format);
  if (!jpeg_sampling_ok(format, h_samp, v_samp))
    return fail(VALI_ERR_INVALID_ARG, "%s: sampling %dx%d does not fit format %d", __func__, h_samp, v_samp, format);
  H = h_samp, V = v_samp;
  memset(out, 0, sizeof(*out));
  const int q = quality < 1 ? 1 : quality > 100 ? 100 : quality;
  const int scale = q < 50 ? 5000 / q : 200 - 2 * q;  // jpeg_quality_scaling
  for (int k = 0; k < 64; ++k) {
    const int l = (kLumaQ[k] * scale + 50) / 100, c = (kChromaQ[k] * scale + 50) / 100;
    out->qtable[0][k] = (uint8_t)(l < 1 ? 1 : l > 255 ? 255 : l);  // force_baseline
    out->qtable[1][k] = (uint8_t)(c < 1 ? 1 : c > 255 ? 255 : c);
  }
  out->quality = q;
  out->format = format;
  out->h_samp = H;
  out->v_samp = V;
  out->restart_interval = kSegBlocks / (H * V + 2);
  return VALI_OK;
}

int vali_jpeg_header(int width, int height, const vali_jpeg_params* params, uint8_t* out, size_t cap, size_t* len) {
  VALI_REQUIRE(len, "null length");
  JpegGeom g;
  const int rc = jpeg_geom(__func__, 1, width, height, params, &g);
  if (rc != VALI_OK)
    return rc;
  u8 buf[kHeaderMax];
  const size_t n = write_header(width, height, params, buf);
  *len = n;
  if (!out)
    return VALI_OK;
  VALI_REQUIRE(cap >= n, "capacity below the header length");
  memcpy(out, buf, n);
  return VALI_OK;
}

int vali_jpeg_workspace_size(int n, int width, int height, const vali_jpeg_params* params, size_t* bytes) {
  VALI_REQUIRE(bytes, "null output");
  JpegGeom g;
  const int rc = jpeg_geom(__func__, n, width, height, params, &g);
  if (rc != VALI_OK)
    return rc;
  *bytes = g.ws_bytes;
  return VALI_OK;
}

int vali_jpeg_stream_capacity(int width, int height, const vali_jpeg_params* params, size_t* bytes) {
  VALI_REQUIRE(bytes, "null output");
  JpegGeom g;
  const int rc = jpeg_geom(__func__, 1, width, height, params, &g);
  if (rc != VALI_OK)
    return rc;
  *bytes = jpeg_capacity(g);
  return VALI_OK;
}

int vali_jpeg_encode_batch(const vali_surface* d_src, int n, int width, int height, int format,
                           const vali_jpeg_params* params, void* workspace, size_t ws_bytes, uint8_t* d_out,
                           size_t out_stride, uint32_t* d_sizes, vali_stream_t stream) {
  VALI_REQUIRE(d_src && params && workspace && d_out && d_sizes, "null argument");
  VALI_REQUIRE(params->format == format, "params were made for another format");
  JpegGeom g;
  int rc = jpeg_geom(__func__, n, width, height, params, &g);
  if (rc != VALI_OK)
    return rc;
  JpegLaunch l;
  rc = jpeg_launch_prepare(__func__, n, g, params, workspace, ws_bytes, d_out, out_stride, &l);
  if (rc != VALI_OK)
    return rc;
  if (n == 0)
    return VALI_OK;

  hipStream_t s = as_stream(stream);
  VALI_ENTRY(s);
  switch (format) {
  case VALI_FMT_RGB:
    launch_fdct<SRC_RGB>(l.cs, l.fgrid, s, l.f, {d_src});
    break;
  case VALI_FMT_BGR:
    launch_fdct<SRC_BGR>(l.cs, l.fgrid, s, l.f, {d_src});
    break;
  case VALI_FMT_RGB_PLANAR:
    launch_fdct<SRC_RGB_PLANAR>(l.cs, l.fgrid, s, l.f, {d_src});
    break;
  default:
    hipLaunchKernelGGL((k_jpeg_fdct<SRC_YUV, 0>), l.fgrid, dim3(256), 0, s, l.f, SurfIn<SRC_YUV>::Args{d_src});
    break;
  }
  VALI_LAUNCH_CHECK();
  return jpeg_launch_rest(__func__, n, l, d_sizes, s);
}

int vali_jpeg_plan_rois(const vali_jpeg_roi* rois, const int32_t* src_w, const int32_t* src_h, int n,
                        const vali_jpeg_params* params, vali_jpeg_item* items, size_t* ws_bytes, size_t* out_bytes) {
  VALI_REQUIRE(ws_bytes && out_bytes, "null output");
  JpegGeom g;
  const int rc = jpeg_geom(__func__, n, 2, 2, params, &g);  // params and n; every format takes 2 x 2
  if (rc != VALI_OK)
    return rc;
  *ws_bytes = *out_bytes = 0;
  if (n == 0)
    return VALI_OK;
  VALI_REQUIRE(rois && src_w && src_h && items, "null argument");
  int fh = 1, fv = 1;  // the sampling of the SOURCE's chroma planes: a rectangle starts and ends on their samples
  jpeg_sampling(params->format, &fh, &fv);
  RoiTotals t = {};
  for (int i = 0; i < n; ++i) {
    const vali_jpeg_roi& r = rois[i];
    if (r.width < 1 || r.height < 1 || r.width > 65535 || r.height > 65535)
      return fail(VALI_ERR_INVALID_ARG, "%s: item %d: rectangle of %d x %d: a side must be 1..65535", __func__, i,
                  r.width, r.height);
    if (r.x < 0 || r.y < 0 || (long long)r.x + r.width > src_w[i] || (long long)r.y + r.height > src_h[i])
      return fail(VALI_ERR_INVALID_ARG, "%s: item %d: rectangle (%d, %d, %d, %d) does not lie inside its %d x %d surface",
                  __func__, i, r.x, r.y, r.width, r.height, src_w[i], src_h[i]);
    if ((fh == 2 && ((r.x | r.width) & 1)) || (fv == 2 && ((r.y | r.height) & 1)))
      return fail(VALI_ERR_INVALID_ARG,
                  "%s: item %d: rectangle (%d, %d, %d, %d): YUV420 needs even x, y, width and height, YUV422 an even x "
                  "and width",
                  __func__, i, r.x, r.y, r.width, r.height);
    if (!roi_item(r, params, &g, &t, &items[i]))
      return fail(VALI_ERR_INVALID_ARG,
                  "%s: item %d: %d x %d is too large for one output slot, or the batch for one launch", __func__, i,
                  r.width, r.height);
  }
  jpeg_layout((size_t)n, t.blocks, t.segs, &g);
  *ws_bytes = g.ws_bytes;
  *out_bytes = t.out;
  return VALI_OK;
}

int vali_jpeg_encode_rois(const vali_surface* d_src, const vali_jpeg_item* items, const vali_jpeg_item* d_items, int n,
                          const vali_jpeg_params* params, void* workspace, size_t ws_bytes, uint8_t* d_out,
                          size_t out_bytes, uint32_t* d_sizes, vali_stream_t stream) {
  VALI_REQUIRE(d_src && items && d_items && params && workspace && d_out && d_sizes, "null argument");
  JpegGeom g;
  int rc = jpeg_geom(__func__, n, 2, 2, params, &g);
  if (rc != VALI_OK)
    return rc;
  if (n == 0)
    return VALI_OK;
  // the records are the plan's: made again from their rectangles, they come out as they are
  RoiTotals t = {};
  for (int i = 0; i < n; ++i) {
    const vali_jpeg_item& it = items[i];
    const vali_jpeg_roi r = {it.x, it.y, it.width, it.height};
    vali_jpeg_item again;
    if (r.x < 0 || r.y < 0 || r.width < 1 || r.height < 1 || r.width > 65535 || r.height > 65535 ||
        !roi_item(r, params, &g, &t, &again) || memcmp(&again, &it, sizeof(it)) != 0)
      return fail(VALI_ERR_INVALID_ARG, "%s: item %d is not what vali_jpeg_plan_rois makes for these params", __func__,
                  i);
  }
  jpeg_layout((size_t)n, t.blocks, t.segs, &g);
  if ((((uintptr_t)workspace) & 255) != 0)
    return fail(VALI_ERR_INVALID_ARG, "%s: workspace not 256-byte aligned", __func__);
  if (ws_bytes < g.ws_bytes)
    return fail(VALI_ERR_INVALID_ARG, "%s: workspace below the plan's ws_bytes", __func__);
  if (out_bytes < t.out)
    return fail(VALI_ERR_INVALID_ARG, "%s: output below the plan's out_bytes", __func__);
  JpegLaunch l;  // the areas of the workspace and the tables; what it holds of one image's geometry is not read
  rc = jpeg_launch_prepare(__func__, n, g, params, workspace, ws_bytes, d_out, out_bytes, &l);
  if (rc != VALI_OK)
    return rc;

  hipStream_t s = as_stream(stream);
  VALI_ENTRY(s);
  const u32 grid = (u32)t.wg_fdct;
  switch (params->format) {
  case VALI_FMT_RGB:
    launch_fdct_roi<SRC_RGB>(l.cs, grid, s, l.f, d_src, d_items, n);
    break;
  case VALI_FMT_BGR:
    launch_fdct_roi<SRC_BGR>(l.cs, grid, s, l.f, d_src, d_items, n);
    break;
  case VALI_FMT_RGB_PLANAR:
    launch_fdct_roi<SRC_RGB_PLANAR>(l.cs, grid, s, l.f, d_src, d_items, n);
    break;
  default:
    hipLaunchKernelGGL((k_jpeg_fdct_roi<SRC_YUV, 0>), dim3(grid), dim3(256), 0, s, l.f, SurfIn<SRC_YUV>::Args{d_src},
                       d_items, n);
    break;
  }
  VALI_LAUNCH_CHECK();
  return jpeg_launch_rest_roi(__func__, n, l, t, d_items, d_sizes, s);
}

int vali_jpeg_encode_tensor(const vali_tensor_src* src, const float scale[3], const float offset[3],
                            const vali_jpeg_params* params, void* workspace, size_t ws_bytes, uint8_t* d_out,
                            size_t out_stride, uint32_t* d_sizes, vali_stream_t stream) {
  VALI_REQUIRE(src && scale && offset && params && workspace && d_out && d_sizes, "null argument");
  int rc = check_tensor_src(__func__, src, scale, offset);
  if (rc != VALI_OK)
    return rc;
  // the channels are colours, or Y, Cb, Cr as they are: a tensor has no subsampled planes
  if (!jpeg_is_rgb(params->format) && params->format != VALI_FMT_YUV444)
    return fail(VALI_ERR_UNSUPPORTED, "%s: format %d cannot name the channels of a tensor", __func__, params->format);
  const int n = src->n;
  JpegGeom g;
  rc = jpeg_geom(__func__, n, src->width, src->height, params, &g);
  if (rc != VALI_OK)
    return rc;
  JpegLaunch l;
  rc = jpeg_launch_prepare(__func__, n, g, params, workspace, ws_bytes, d_out, out_stride, &l);
  if (rc != VALI_OK)
    return rc;
  TensorArgs ta = {};
  ta.t = *src;
  for (int c = 0; c < 3; ++c)
    ta.scale[c] = scale[c], ta.offset[c] = offset[c];
  ta.swap_rb = params->format == VALI_FMT_BGR;
  const bool yuv = params->format == VALI_FMT_YUV444, packed = src->packed != 0;

  hipStream_t s = as_stream(stream);
  VALI_ENTRY(s);
  with_src_dtype(src->dtype, [&](auto dt) { launch_fdct_tensor<dt>(packed, yuv, l.cs, l.fgrid, s, l.f, ta); });
  VALI_LAUNCH_CHECK();
  return jpeg_launch_rest(__func__, n, l, d_sizes, s);
}

} // extern "C"
