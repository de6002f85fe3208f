// vali_detect_select: a detector's raw head -> GPU-held detections in frame pixels (include/vali_hip.h, "detections").
// Four launches whatever the data, nothing allocated, nothing synchronised:
//   k_det_score   reads the N*K*C scores once; per candidate one ordered 32-bit key (0: not a candidate) and its class
//   k_det_select  one workgroup per frame: the survivors into LDS (a radix select of the T-th (key, k) pair when more
//                 than T pass), each placed by the number of survivors above it
//   k_det_iou     the suppression bit matrix, four waves per 64 x 64 tile of the lower triangle below the candidate count
//   k_det_reduce  one wave per frame walks the candidates 64 at a time from registers and writes dets, counts, rois, marks
// tests/detect_model.py restates the definition in numpy; tests/test_gpu_detect_select.py compares bit for bit.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "common.hpp"
#include "mark_rows.hpp"
#include "tensor_in.hpp"

#pragma clang fp contract(off)

namespace vali {
namespace {

typedef uint64_t u64;
typedef uint16_t u16;

constexpr int kMaxN = 1024, kMaxK = 1 << 20, kMaxC = 4096, kMaxT = 1024;

struct DetTensor {
  const void* p;
  int dtype;
  long long sn, sk, sc;  // element strides
};

struct DetArgs {
  DetTensor boxes, scores;
  int n, k, c, T, D;
  float score_thr, iou_thr;
  int agnostic, cxcywh;
  const vali_roi* rects;
  // the workspace
  u32* keys;      // n x KS: the ordered key of a candidate, 0 when it is none
  u16* cls;       // n x KS
  u32* cnt;       // n: candidates that went on, <= T
  float4* sbox;   // n x T: x1, y1, x2, y2, sorted
  uint4* smeta;   // n x T: class, k, score bits, 0
  u64* mask;      // n x T x W: bit i of row j: i < j suppresses j
  int KS, W;
};

struct DetOut {
  int32_t *dets, *counts, *rois;
  MarkStyle ms;  // marks: mark_rows.hpp
  int crop[4];
};

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

struct FrameRec {
  float dx, dy, dx2, dy2;
  bool ok;
};

__device__ __forceinline__ FrameRec frame_rec(const vali_roi& r) {
  FrameRec fr;
  fr.ok = r.src_w >= 1 && r.src_h >= 1 && r.dst_w >= 1 && r.dst_h >= 1;
  fr.dx = (float)r.dst_x, fr.dy = (float)r.dst_y;
  fr.dx2 = (float)((long long)r.dst_x + (long long)r.dst_w), fr.dy2 = (float)((long long)r.dst_y + (long long)r.dst_h);
  return fr;
}

// step 3 of the definition: the box of candidate k in network coordinates, clipped to the placement
__device__ __forceinline__ bool det_box(const DetArgs& a, int f, int k, const FrameRec& fr, float4& o) {
  const long long base = (long long)f * a.boxes.sn + (long long)k * a.boxes.sk;
  const float b0 = tensor_elem_f(a.boxes.p, a.boxes.dtype, base);
  const float b1 = tensor_elem_f(a.boxes.p, a.boxes.dtype, base + a.boxes.sc);
  const float b2 = tensor_elem_f(a.boxes.p, a.boxes.dtype, base + 2 * a.boxes.sc);
  const float b3 = tensor_elem_f(a.boxes.p, a.boxes.dtype, base + 3 * a.boxes.sc);
  float x1 = b0, y1 = b1, x2 = b2, y2 = b3;
  if (a.cxcywh) {
    const float hw = __fmul_rn(b2, 0.5f), hh = __fmul_rn(b3, 0.5f);
    x1 = __fsub_rn(b0, hw), x2 = __fadd_rn(b0, hw);
    y1 = __fsub_rn(b1, hh), y2 = __fadd_rn(b1, hh);
  }
  // the edge replaces the coordinate only when the comparison holds: a NaN stays a NaN
  x1 = fr.dx > x1 ? fr.dx : x1, y1 = fr.dy > y1 ? fr.dy : y1;
  x2 = fr.dx2 < x2 ? fr.dx2 : x2, y2 = fr.dy2 < y2 ? fr.dy2 : y2;
  o = make_float4(x1, y1, x2, y2);
  return finite_f(x1) && finite_f(y1) && finite_f(x2) && finite_f(y2) && x2 > x1 && y2 > y1;
}

// floats in their order as unsigned integers; -0.0 is 0.0; no float gives 0
__device__ __forceinline__ u32 score_key(float s) {
  u32 b = __float_as_uint(s);
  b = b == 0x80000000u ? 0u : b;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ u32 key_score_bits(u32 key) { return (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key; }

// (key, k) as one number: key descending, then k ascending, is this number descending
__device__ __forceinline__ u64 comp56(u32 key, int k) { return ((u64)key << 24) | ((u64)(0xFFFFFu - (u32)k) << 4); }

__device__ __forceinline__ void finish_candidate(const DetArgs& a, int f, int k, float s, int cls, const FrameRec& fr) {
  u32 key = 0;
  if (fr.ok && s > a.score_thr) {
    float4 b;
    if (det_box(a, f, k, fr, b))
      key = score_key(s);
  }
  const size_t at = (size_t)f * a.KS + k;
  a.keys[at] = key;
  a.cls[at] = (u16)cls;
}

// ---- k_det_score ---------------------------------------------------------------------------------------------------
// any strides: a lane per candidate walks its classes; coalesced when k is the contiguous dimension
template <int DT>
__global__ __launch_bounds__(256) void k_det_score(DetArgs a) {
  typedef TensorElem<DT> E;
  typedef typename E::Bits Bits;
  const int f = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
  if (k >= a.k)
    return;
  const FrameRec fr = frame_rec(a.rects[f]);
  const Bits* p = (const Bits*)a.scores.p + (long long)f * a.scores.sn + (long long)k * a.scores.sk;
  float s = -INFINITY;
  int cls = 0;
#pragma unroll 4
  for (int c = 0; c < a.c; ++c) {
    const float v = E::f(p[(long long)c * a.scores.sc]);
    if (v > s)
      s = v, cls = c;
  }
  finish_candidate(a, f, k, s, cls, fr);
}

// classes contiguous, rows 16-byte aligned: eight lanes share a candidate, 16 bytes per lane and load
template <int DT>
__global__ __launch_bounds__(256) void k_det_score_c(DetArgs a) {
  typedef TensorElem<DT> E;
  typedef typename E::Bits Bits;
  constexpr int ES = sizeof(Bits), EPC = 16 / ES;
  const int f = blockIdx.y, sub = threadIdx.x & 7, cand = blockIdx.x * 32 + (threadIdx.x >> 3);
  const int k = min(cand, a.k - 1);
  const FrameRec fr = frame_rec(a.rects[f]);
  const Bits* row = (const Bits*)a.scores.p + (long long)f * a.scores.sn + (long long)k * a.scores.sk;
  float s = -INFINITY;
  int cls = 0;
  const int nfull = a.c / EPC;
  for (int ch = sub; ch < nfull; ch += 8) {
    u32 w[4];
    load_elems<ES, EPC>(row + ch * EPC, w);
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      const float v = E::f(elem_bits<ES>(w, e));
      if (v > s)
        s = v, cls = ch * EPC + e;
    }
  }
  for (int c = nfull * EPC + sub; c < a.c; c += 8) {
    const float v = E::f(row[c]);
    if (v > s)
      s = v, cls = c;
  }
#pragma unroll
  for (int m = 1; m < 8; m <<= 1) {
    const float os = __shfl_xor(s, m);
    const int oc = __shfl_xor(cls, m);
    if (os > s || (os == s && oc < cls))
      s = os, cls = oc;
  }
  if (sub == 0 && cand < a.k)
    finish_candidate(a, f, k, s, cls, fr);
}

// candidates contiguous (a transposed head), planes 16-byte aligned: a lane owns 16 bytes of consecutive candidates, the
// eight waves of a block split the classes, so that a wave has its few loads in flight together, and meet in LDS
constexpr int kScoreWaves = 8;
template <int DT>
__global__ __launch_bounds__(64 * kScoreWaves) void k_det_score_k(DetArgs a) {
  typedef TensorElem<DT> E;
  typedef typename E::Bits Bits;
  constexpr int ES = sizeof(Bits), EPC = 16 / ES;
  __shared__ float ss[kScoreWaves][EPC][64];
  __shared__ u16 sc[kScoreWaves][EPC][64];
  const int f = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k0 = (blockIdx.x * 64 + lane) * EPC;
  const FrameRec fr = frame_rec(a.rects[f]);
  const Bits* base = (const Bits*)a.scores.p + (long long)f * a.scores.sn;
  const int cq = (a.c + kScoreWaves - 1) / kScoreWaves, c0 = wave * cq, c1 = min(a.c, c0 + cq);
  float s[EPC];
  int cls[EPC];
#pragma unroll
  for (int e = 0; e < EPC; ++e)
    s[e] = -INFINITY, cls[e] = 0;
  if (k0 + EPC <= a.k) {
#pragma unroll 5
    for (int c = c0; c < c1; ++c) {
      u32 w[4];
      load_elems<ES, EPC>(base + (long long)c * a.scores.sc + k0, w);
#pragma unroll
      for (int e = 0; e < EPC; ++e) {
        const float v = E::f(elem_bits<ES>(w, e));
        if (v > s[e])
          s[e] = v, cls[e] = c;
      }
    }
  } else if (k0 < a.k) {
    for (int c = c0; c < c1; ++c) {
      const Bits* p = base + (long long)c * a.scores.sc;
#pragma unroll
      for (int e = 0; e < EPC; ++e) {
        const float v = E::f(p[min(k0 + e, a.k - 1)]);
        if (v > s[e])
          s[e] = v, cls[e] = c;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < EPC; ++e)
    ss[wave][e][lane] = s[e], sc[wave][e][lane] = (u16)cls[e];
  __syncthreads();
  // wave e finishes candidate k0 + e of every lane: the boxes of those that pass are fetched by EPC waves side by side
  if (wave < EPC) {
    const int e = wave;
    float bs = ss[0][e][lane];
    int bc = sc[0][e][lane];
#pragma unroll
    for (int w = 1; w < kScoreWaves; ++w) {  // later waves hold higher classes: only a greater score replaces
      const float os = ss[w][e][lane];
      if (os > bs)
        bs = os, bc = sc[w][e][lane];
    }
    if (k0 + e < a.k)
      finish_candidate(a, f, k0 + e, bs, bc, fr);
  }
}

// ---- k_det_select --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_det_select(DetArgs a) {
  __shared__ u32 hist[256];
  __shared__ u64 list[kMaxT];
  __shared__ u32 sh[3];  // digit, candidates above it, candidates in it
  __shared__ u32 s_n;
  const int f = blockIdx.x, tid = threadIdx.x;
  const u32* keys = a.keys + (size_t)f * a.KS;
  const FrameRec fr = frame_rec(a.rects[f]);

  // The first pass over the keys counts the candidates by their top digit and collects them: with T or fewer, which is
  // the usual case, they all go on and the keys are read once.  With more, the T-th largest (key, k) is found eight bits
  // a pass, and the candidates from it upwards are collected again.
  if (tid < 256)
    hist[tid] = 0;
  if (tid == 0)
    s_n = 0;
  __syncthreads();
  for (int k0 = tid; k0 < a.k; k0 += 16 * 1024) {  // sixteen loads in flight, then the LDS atomics they lead to
    u32 key[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int k = k0 + u * 1024;
      key[u] = k < a.k ? keys[k] : 0u;
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      if (key[u]) {
        const u64 v = comp56(key[u], k0 + u * 1024);
        atomicAdd(&hist[(u32)(v >> 48) & 0xFFu], 1u);
        const u32 at = atomicAdd(&s_n, 1u);
        if (at < (u32)kMaxT)
          list[at] = v;
      }
    }
  }
  __syncthreads();
  const u32 total = s_n;
  if (total > (u32)a.T) {
    u64 prefix = 0, cut = 0;
    u32 want = (u32)a.T;
    for (int p = 0; p < 7; ++p) {
      const int shift = 48 - 8 * p;
      if (p > 0) {
        if (tid < 256)
          hist[tid] = 0;
        __syncthreads();
        for (int k = tid; k < a.k; k += 1024) {
          const u32 key = keys[k];
          if (key) {
            const u64 v = comp56(key, k);
            if ((v >> (shift + 8)) == prefix)
              atomicAdd(&hist[(u32)(v >> shift) & 0xFFu], 1u);
          }
        }
        __syncthreads();
      }
      if (tid < 64) {
        u32 c[4], t = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u)
          c[u] = hist[255 - (4 * tid + u)], t += c[u];
        u32 incl = t;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const u32 nb = __shfl_up(incl, o);
          if (tid >= o)
            incl += nb;
        }
        u32 run = incl - t, fd = 0, fab = 0, fbk = 0;
        bool fnd = false;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (!fnd && c[u] > 0 && run + c[u] >= want)
            fnd = true, fd = 255 - (4 * tid + u), fab = run, fbk = c[u];
          run += c[u];
        }
        // (the digit exists: the candidates that share the prefix are at least `want`)
        const u64 m = __ballot(fnd);
        if (m != 0 && tid == __ffsll((unsigned long long)m) - 1)
          sh[0] = fd, sh[1] = fab, sh[2] = fbk;
      }
      __syncthreads();
      want -= sh[1];
      prefix = (prefix << 8) | sh[0];
      if (sh[2] == want || p == 6) {  // the whole digit goes on: nothing below it needs to be told apart
        cut = prefix << shift;
        break;
      }
    }
    __syncthreads();
    if (tid == 0)
      s_n = 0;
    __syncthreads();
    for (int k = tid; k < a.k; k += 1024) {
      const u32 key = keys[k];
      if (key) {
        const u64 v = comp56(key, k);
        if (v >= cut) {
          const u32 at = atomicAdd(&s_n, 1u);
          if (at < (u32)kMaxT)
            list[at] = v;
        }
      }
    }
    __syncthreads();
  }
  // the place of a survivor is the number of survivors above it: the pairs are all different, every lane reads the same
  // LDS word at a time (a broadcast), and no barrier is needed
  const int cnt = min((int)s_n, a.T);
  if (tid == 0)
    a.cnt[f] = (u32)cnt;
  if (tid < cnt) {
    const u64 v = list[tid];
    int rank = 0;
#pragma unroll 8
    for (int i = 0; i < cnt; ++i)
      rank += list[i] > v ? 1 : 0;
    const u32 key = (u32)(v >> 24);
    const int k = (int)(0xFFFFFu - ((u32)(v >> 4) & 0xFFFFFu));
    float4 b;
    det_box(a, f, k, fr, b);
    const size_t at = (size_t)f * a.T + rank;
    a.sbox[at] = b;
    a.smeta[at] = make_uint4(a.cls[(size_t)f * a.KS + k], (u32)k, key_score_bits(key), 0u);
  }
}

// ---- k_det_iou -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float lane_f(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// four waves per 64 x 64 tile of the lower triangle: block (w, jb, f) has the rows j = 64 jb + lane; wave q takes the
// sixteen earlier candidates i = 64 w + 16 q + b, whose boxes travel from lane b to all, and writes its sixteen bits of
// the word.  (One wave per tile spent 12 us on its 64 dependent steps; the tile is latency, not work.)
__global__ __launch_bounds__(256) void k_det_iou(DetArgs a) {
  const int w = blockIdx.x, jb = blockIdx.y, f = blockIdx.z;
  const int cnt = (int)a.cnt[f];
  if (w > jb || jb * 64 >= cnt)
    return;
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const float4* sb = a.sbox + (size_t)f * a.T;
  const uint4* sm = a.smeta + (size_t)f * a.T;
  const int j = jb * 64 + lane;
  const bool jv = j < cnt;
  const float4 bj = jv ? sb[j] : make_float4(0.f, 0.f, 0.f, 0.f);
  const int cj = jv ? (int)sm[j].x : 0;
  const float aj = __fmul_rn(bj.z - bj.x, bj.w - bj.y);
  const int i0 = w * 64 + 16 * q, il = i0 + (lane & 15);
  const bool iv = il < cnt;
  const float4 bi = iv ? sb[il] : make_float4(0.f, 0.f, 0.f, 0.f);
  const int ci = iv ? (int)sm[il].x : -1;
  const float ai = __fmul_rn(bi.z - bi.x, bi.w - bi.y);
  u32 bits = 0;
#pragma unroll
  for (int b = 0; b < 16; ++b) {
    const float x1 = lane_f(bi.x, b), y1 = lane_f(bi.y, b), x2 = lane_f(bi.z, b), y2 = lane_f(bi.w, b);
    const float area = lane_f(ai, b);
    const int c = __builtin_amdgcn_readlane(ci, b);
    const float iw = fmaxf(fminf(x2, bj.z) - fmaxf(x1, bj.x), 0.0f);
    const float ih = fmaxf(fminf(y2, bj.w) - fmaxf(y1, bj.y), 0.0f);
    const float inter = __fmul_rn(iw, ih);
    const float uni = __fsub_rn(__fadd_rn(area, aj), inter);
    const bool sup = (a.agnostic || c == cj) && inter > __fmul_rn(a.iou_thr, uni) && (i0 + b) < j;
    bits |= (u32)sup << b;
  }
  if (jv)
    ((u16*)a.mask)[(((size_t)f * a.T + j) * a.W + w) * 4 + q] = (u16)bits;
}

// ---- k_det_reduce --------------------------------------------------------------------------------------------------
// rows of slot `at` = f * D + r for a detection (step 6 of the definition), or the unused forms when !used
__device__ __forceinline__ void emit(const DetArgs& a, const DetOut& o, int f, int at, bool used, const float4& b,
                                     const uint4& m, const vali_roi& rc) {
  const int M = a.n * a.D;
  int x = 0, y = 0, w = 0, h = 0;
  if (used) {
    const float sx = (float)rc.src_w / (float)rc.dst_w, sy = (float)rc.src_h / (float)rc.dst_h;
    const float fdx = (float)rc.dst_x, fdy = (float)rc.dst_y, fsx = (float)rc.src_x, fsy = (float)rc.src_y;
    const float hx = (float)((long long)rc.src_x + (long long)rc.src_w), hy = (float)((long long)rc.src_y + (long long)rc.src_h);
    float X1 = floorf(__fadd_rn(__fmul_rn(__fsub_rn(b.x, fdx), sx), fsx));
    float X2 = ceilf(__fadd_rn(__fmul_rn(__fsub_rn(b.z, fdx), sx), fsx));
    float Y1 = floorf(__fadd_rn(__fmul_rn(__fsub_rn(b.y, fdy), sy), fsy));
    float Y2 = ceilf(__fadd_rn(__fmul_rn(__fsub_rn(b.w, fdy), sy), fsy));
    X1 = fminf(fmaxf(X1, fsx), hx), X2 = fminf(fmaxf(X2, fsx), hx);
    Y1 = fminf(fmaxf(Y1, fsy), hy), Y2 = fminf(fmaxf(Y2, fsy), hy);
    const long long xi = (long long)X1, yi = (long long)Y1;
    const long long wi = max((long long)X2 - xi, 1ll), hi = max((long long)Y2 - yi, 1ll);
    x = (int)min(xi, (long long)INT_MAX), y = (int)min(yi, (long long)INT_MAX);
    w = (int)min(wi, (long long)INT_MAX), h = (int)min(hi, (long long)INT_MAX);
  }
  const int cls = (int)m.x;
  if (o.dets) {
    if (used)
      put_row(o.dets + (size_t)at * 8, f, x, y, w, h, cls, (int)m.z, (int)m.y);
    else
      put_row(o.dets + (size_t)at * 8, -1, 0, 0, 0, 0, 0, 0, 0);
  }
  if (o.rois) {
    if (used)
      put_row(o.rois + (size_t)at * 8, x, y, w, h, o.crop[0], o.crop[1], o.crop[2], o.crop[3]);
    else
      put_row(o.rois + (size_t)at * 8, 0, 0, 0, 0, 0, 0, 0, 0);
  }
  if (o.ms.marks)
    put_marks(o.ms, M, at, used, f, x, y, w, h, used ? cls % o.ms.n_colours : 0, cls < o.ms.n_labels ? cls : -1);
}

__device__ __forceinline__ u64 lane_u64(u64 v, int l) {
  const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)v, l), hi = (u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), l);
  return ((u64)hi << 32) | lo;
}

// one wave per frame.  Candidate j's row holds who suppresses it, so with the kept sets of the earlier 64-blocks final,
// a block needs only its own rows: loaded a block ahead, resolved from registers.
__global__ __launch_bounds__(64) void k_det_reduce(DetArgs a, DetOut o) {
  constexpr int kW = kMaxT / 64;
  const int f = blockIdx.x, lane = threadIdx.x;
  const int cnt = (int)a.cnt[f];
  const vali_roi rc = a.rects[f];
  const u64* rows = a.mask + (size_t)f * a.T * a.W;
  const float4* sb = a.sbox + (size_t)f * a.T;
  const uint4* sm = a.smeta + (size_t)f * a.T;
  u64 kept[kW], cur[kW], nxt[kW];
#pragma unroll
  for (int w = 0; w < kW; ++w)
    kept[w] = 0, cur[w] = 0, nxt[w] = 0;
  if (lane < cnt)
    cur[0] = rows[(size_t)lane * a.W];
  int nkept = 0;
#pragma unroll
  for (int c = 0; c < kW; ++c) {
    if (c * 64 >= cnt || nkept >= a.D)
      break;
    const int j = c * 64 + lane;
    const bool valid = j < cnt;
    if (c + 1 < kW) {
      const int jn = j + 64;
      if (jn < cnt) {
#pragma unroll
        for (int w = 0; w <= c + 1; ++w)
          nxt[w] = rows[(size_t)jn * a.W + w];
      }
    }
    bool pre = !valid;
#pragma unroll
    for (int w = 0; w < c; ++w)
      pre = pre || (cur[w] & kept[w]) != 0;
    const u64 diag = valid ? cur[c] : 0;
    const u64 gone = __ballot(pre);
    u64 km = ~gone;
    u64 todo = __ballot(diag != 0) & ~gone;  // only these depend on the rows before them in the block
    while (todo) {
      const int b = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      if (lane_u64(diag, b) & km)
        km &= ~(1ull << b);
    }
    kept[c] = km;
    const bool mine = (km >> lane) & 1;
    const int rank = nkept + __popcll(km & ((1ull << lane) - 1));
    if (mine && rank < a.D)
      emit(a, o, f, f * a.D + rank, true, sb[j], sm[j], rc);
    nkept += __popcll(km);
#pragma unroll
    for (int w = 0; w < kW; ++w)
      cur[w] = nxt[w];
  }
  const int count = min(nkept, a.D);
  if (lane == 0 && o.counts)
    o.counts[f] = count;
  for (int r = count + lane; r < a.D; r += 64)
    emit(a, o, f, f * a.D + r, false, make_float4(0.f, 0.f, 0.f, 0.f), make_uint4(0, 0, 0, 0), rc);
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

struct WsLayout {
  size_t keys, cls, cnt, sbox, smeta, mask, total;
  int KS, W;
};

WsLayout ws_layout(int n, int k, int T) {
  WsLayout l;
  l.KS = (k + 7) & ~7;
  l.W = (T + 63) / 64;
  size_t at = 0;
  l.keys = at, at += align16((size_t)n * l.KS * 4);
  l.cls = at, at += align16((size_t)n * l.KS * 2);
  l.cnt = at, at += align16((size_t)n * 4);
  l.sbox = at, at += (size_t)n * T * 16;
  l.smeta = at, at += (size_t)n * T * 16;
  l.mask = at, at += (size_t)n * T * l.W * 8;
  l.total = at;
  return l;
}

bool dims_ok(int n, int k, int T) { return n >= 1 && n <= kMaxN && k >= 1 && k <= kMaxK && T >= 1 && T <= kMaxT; }

int check_tensor(const char* who, const vali_detect_tensor& t, const char* name) {
  const int64_t strides[3] = {t.stride_n, t.stride_k, t.stride_c};
  return check_head_tensor(who, name, t.data, t.dtype, strides, 3);
}

template <int DT>
void launch_score(const DetArgs& a, hipStream_t s) {
  constexpr int ES = DT == VALI_DTYPE_F32 ? 4 : 2, EPC = 16 / ES;
  const DetTensor& t = a.scores;
  const auto al = [&](long long stride) { return (stride * ES) % 16 == 0; };
  const bool base16 = ((uintptr_t)t.p & 15u) == 0;
  if (t.sc == 1 && a.c * ES >= 64 && base16 && al(t.sn) && al(t.sk))
    hipLaunchKernelGGL(k_det_score_c<DT>, dim3((a.k + 31) / 32, a.n), dim3(256), 0, s, a);
  else if (t.sk == 1 && a.k >= EPC && base16 && al(t.sn) && al(t.sc))
    hipLaunchKernelGGL(k_det_score_k<DT>, dim3((a.k + 64 * EPC - 1) / (64 * EPC), a.n), dim3(64 * kScoreWaves), 0, s, a);
  else
    hipLaunchKernelGGL(k_det_score<DT>, dim3((a.k + 255) / 256, a.n), dim3(256), 0, s, a);
}

} // namespace
} // namespace vali

using namespace vali;

extern "C" {

size_t vali_detect_workspace_size(int n, int k, int max_candidates) {
  if (!dims_ok(n, k, max_candidates))
    return 0;
  return ws_layout(n, k, max_candidates).total;
}

int vali_detect_select(const vali_detect_in* in, const vali_detect_params* params, const vali_roi* d_rects,
                       const vali_detect_out* out, void* d_ws, size_t ws_bytes, vali_stream_t stream) {
  VALI_REQUIRE(in && params && d_rects && out && d_ws, "null argument");
  VALI_REQUIRE(in->n >= 1 && in->n <= kMaxN, "n outside 1..1024");
  VALI_REQUIRE(in->k >= 1 && in->k <= kMaxK, "k outside 1..2^20");
  VALI_REQUIRE(in->c >= 1 && in->c <= kMaxC, "c outside 1..4096");
  int rc = check_tensor(__func__, in->boxes, "boxes");
  if (rc != VALI_OK)
    return rc;
  rc = check_tensor(__func__, in->scores, "scores");
  if (rc != VALI_OK)
    return rc;
  const int T = params->max_candidates, D = params->max_det;
  VALI_REQUIRE(T >= 1 && T <= kMaxT, "max_candidates outside 1..1024");
  VALI_REQUIRE(D >= 1 && D <= T, "max_det outside 1..max_candidates");
  VALI_REQUIRE((long long)in->n * D <= 65535, "n * max_det exceeds 65535");
  VALI_REQUIRE(isfinite(params->score_thr), "score_thr is not finite");
  VALI_REQUIRE(isfinite(params->iou_thr), "iou_thr is not finite");
  VALI_REQUIRE(params->box_format == VALI_DETECT_XYXY || params->box_format == VALI_DETECT_CXCYWH,
               "box_format is neither VALI_DETECT_XYXY nor VALI_DETECT_CXCYWH");
  VALI_REQUIRE(((uintptr_t)d_rects & 3u) == 0, "rects are not 4-byte aligned");
  VALI_REQUIRE(((uintptr_t)d_ws & 15u) == 0, "the workspace is not 16-byte aligned");
  const WsLayout l = ws_layout(in->n, in->k, T);
  VALI_REQUIRE(ws_bytes >= l.total, "the workspace is smaller than vali_detect_workspace_size");
  VALI_REQUIRE((((uintptr_t)out->dets | (uintptr_t)out->counts | (uintptr_t)out->rois | (uintptr_t)out->marks |
                 (uintptr_t)out->colours | (uintptr_t)out->label_rects) & 3u) == 0, "an output or style array is not 4-byte aligned");
  if (out->marks) {
    VALI_REQUIRE(out->colours && params->n_colours >= 1, "marks without colours");
    VALI_REQUIRE((long long)(out->label_rects ? 3 : 1) * in->n * D <= VALI_MAX_MARKS, "more than 4096 mark rows");
    VALI_REQUIRE(params->thickness >= 1, "thickness below 1");
    VALI_REQUIRE(params->label_alpha >= 0 && params->label_alpha <= 255, "label_alpha outside 0..255");
    VALI_REQUIRE(!out->label_rects || params->n_labels >= 1, "label_rects without n_labels");
  }

  DetArgs a = {};
  a.boxes = {in->boxes.data, in->boxes.dtype, in->boxes.stride_n, in->boxes.stride_k, in->boxes.stride_c};
  a.scores = {in->scores.data, in->scores.dtype, in->scores.stride_n, in->scores.stride_k, in->scores.stride_c};
  a.n = in->n, a.k = in->k, a.c = in->c, a.T = T, a.D = D;
  a.score_thr = params->score_thr, a.iou_thr = params->iou_thr;
  a.agnostic = params->class_agnostic != 0, a.cxcywh = params->box_format == VALI_DETECT_CXCYWH;
  a.rects = d_rects;
  uint8_t* ws = (uint8_t*)d_ws;
  a.keys = (u32*)(ws + l.keys), a.cls = (u16*)(ws + l.cls), a.cnt = (u32*)(ws + l.cnt);
  a.sbox = (float4*)(ws + l.sbox), a.smeta = (uint4*)(ws + l.smeta), a.mask = (u64*)(ws + l.mask);
  a.KS = l.KS, a.W = l.W;
  DetOut o = {};
  o.dets = out->dets, o.counts = out->counts, o.rois = out->rois;
  o.ms = {out->marks, out->colours, out->label_rects, params->n_colours, params->n_labels, params->thickness,
          params->label_alpha, params->text_colour};
  for (int i = 0; i < 4; ++i)
    o.crop[i] = params->crop[i];

  hipStream_t s = as_stream(stream);
  VALI_ENTRY(s);
  with_float_dtype(a.scores.dtype, [&](auto dt) { launch_score<dt>(a, s); });
  VALI_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_det_select, dim3(a.n), dim3(1024), 0, s, a);
  VALI_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_det_iou, dim3(a.W, a.W, a.n), dim3(256), 0, s, a);
  VALI_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_det_reduce, dim3(a.n), dim3(64), 0, s, a, o);
  VALI_LAUNCH_CHECK();
  return VALI_OK;
}

} // extern "C"
