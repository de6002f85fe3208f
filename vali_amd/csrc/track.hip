// vali_track_update: vali_detect_select's rows associated over time with tracks held in device memory (include/vali_hip.h,
// "tracks").  One launch, one wave per stream: the work is sequential in the rows and parallel over the tracks.
//   - the stream's T <= 256 tracks live in registers for the whole call, slot j * 64 + lane in register set j of a lane;
//     they are loaded once and stored once, 16 bytes at a time
//   - a frame's rows are loaded 64 at a time, one a lane, and taken in order: a row's values travel from its lane to all
//     (v_readlane), every lane forms the IoU with the tracks it holds, and the winner is the greatest (iou bits, ~slot)
//     pair of the wave -- read straight from the one lane that has a candidate, which is the usual case
//   - the lane that loaded a row keeps what became of it and writes the row's outputs; the rows that may start a track are
//     a 64-bit mask per group of 64, parked in lane `group`, and are taken after the frame's misses are counted
// No workgroup barrier, no atomic, no LDS.  tests/track_model.py restates the definition in numpy;
// tests/test_gpu_track.py compares bit for bit.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "common.hpp"
#include "dev_util.hpp"
#include "mark_rows.hpp"

#pragma clang fp contract(off)

namespace vali {
namespace {

typedef uint64_t u64;

constexpr int kMaxN = 1024, kMaxD = 1024, kMaxT = 256, kSets = kMaxT / 64, kSat = 1 << 30, kMaxAge = 1 << 20;

struct TrackArgs {
  const int32_t* dets;
  int32_t *tracks, *clock, *tracked, *assoc;
  MarkStyle ms;
  int F, D, T, M;  // frames per stream, rows per frame, tracks per stream, n * D
  float iou_thr, new_thr, momentum;
  int min_hits, max_age, agnostic;
};

__device__ __forceinline__ int lane_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ u64 lane_u64(u64 v, int l) {
  const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)v, l), hi = (u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), l);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ int sat_inc(int v) { return v < kSat ? v + 1 : kSat; }
__device__ __forceinline__ int clamp_count(int v) { return v < 0 ? 0 : v > kSat ? kSat : v; }

// the tracks a lane holds: set j is slot j * 64 + lane; id 0: free (or beyond T)
struct Held {
  int id[kSets], cls[kSets], x[kSets], y[kSets], w[kSets], h[kSets], vx[kSets], vy[kSets];  // vx, vy: float32 bits
  int hits[kSets], miss[kSets], age[kSets], score[kSets], k[kSets];
};

__device__ __forceinline__ void free_slot(Held& t, int j) {
  t.id[j] = t.cls[j] = t.x[j] = t.y[j] = t.w[j] = t.h[j] = t.vx[j] = t.vy[j] = 0;
  t.hits[j] = t.miss[j] = t.age[j] = t.score[j] = t.k[j] = 0;
}

// a row's eight values, 4-byte aligned
__device__ __forceinline__ void load_det(const int32_t* p, int (&d)[8]) {
  const uint4 a = load16_u(p), b = load16_u(p + 4);
  d[0] = (int)a.x, d[1] = (int)a.y, d[2] = (int)a.z, d[3] = (int)a.w;
  d[4] = (int)b.x, d[5] = (int)b.y, d[6] = (int)b.z, d[7] = (int)b.w;
}

// A wave-uniform value parked in a vector register.  The association loop needs every scalar register the wave has (the
// row's values, the masks, the loop's own state); what only the output rows need -- eight pointers and as many numbers --
// would push some of them out (the compiler spilled nine), and vector registers are there in plenty.
__device__ __forceinline__ int park(int v) {
  int r;
  asm("v_mov_b32 %0, %1" : "=v"(r) : "s"(v));
  return r;
}
template <typename P>
__device__ __forceinline__ P* park(P* p) {
  const u64 v = (u64)(uintptr_t)p;
  const u32 lo = (u32)park((int)(u32)v), hi = (u32)park((int)(u32)(v >> 32));
  return (P*)(uintptr_t)(((u64)hi << 32) | lo);
}

// what the output rows are written from, parked
struct TrackOut {
  int32_t *tracked, *assoc;
  MarkStyle ms;
  int D, M, min_hits;
};

__device__ __forceinline__ TrackOut park_outputs(const TrackArgs& a) {
  TrackOut o;
  o.tracked = park(a.tracked), o.assoc = park(a.assoc);
  o.ms.marks = park(a.ms.marks), o.ms.colours = park(a.ms.colours), o.ms.label_rects = park(a.ms.label_rects);
  o.ms.n_colours = park(a.ms.n_colours), o.ms.n_labels = park(a.ms.n_labels), o.ms.thickness = park(a.ms.thickness);
  o.ms.label_alpha = park(a.ms.label_alpha), o.ms.text_colour = park(a.ms.text_colour);
  o.D = park(a.D), o.M = park(a.M), o.min_hits = park(a.min_hits);
  return o;
}

// the outputs of row r of frame i, whose values are d; slot < 0: neither matched nor born
__device__ __forceinline__ void put_outputs(const TrackOut& a, int i, int r, const int (&d)[8], int slot, int id, int hits) {
  const int at = i * a.D + r;
  const bool shown = slot >= 0 && hits >= a.min_hits;
  if (shown)
    put_row(a.tracked + (size_t)at * 8, i, d[1], d[2], d[3], d[4], id, d[6], d[7]);
  else
    put_row(a.tracked + (size_t)at * 8, -1, 0, 0, 0, 0, 0, 0, 0);
  if (a.assoc) {
    int32_t* p = a.assoc + (size_t)at * 4;
    if (slot >= 0)
      p[0] = id, p[1] = slot, p[2] = hits, p[3] = d[5];
    else
      p[0] = 0, p[1] = -1, p[2] = 0, p[3] = 0;
  }
  if (a.ms.marks)
    put_marks(a.ms, a.M, at, shown, i, d[1], d[2], d[3], d[4], shown ? id % a.ms.n_colours : 0,
              shown && a.ms.label_rects ? id % a.ms.n_labels : -1);
}

__global__ __launch_bounds__(64) void k_track_update(TrackArgs a) {
  const int s = blockIdx.x, lane = threadIdx.x;
  int32_t* mine = a.tracks + (size_t)s * a.T * 16;
  const TrackOut out = park_outputs(a);
  Held t;
#pragma unroll
  for (int j = 0; j < kSets; ++j) {
    free_slot(t, j);
    const int slot = j * 64 + lane;
    if (slot < a.T) {
      const int32_t* p = mine + (size_t)slot * 16;
      const uint4 q0 = load16(p), q1 = load16(p + 4), q2 = load16(p + 8), q3 = load16(p + 12);
      if ((int)q0.x >= 1 && (int)q1.x >= 1 && (int)q1.y >= 1) {  // live: id, w, h
        t.id[j] = (int)q0.x, t.cls[j] = (int)q0.y, t.x[j] = (int)q0.z, t.y[j] = (int)q0.w;
        t.w[j] = (int)q1.x, t.h[j] = (int)q1.y, t.vx[j] = (int)q1.z, t.vy[j] = (int)q1.w;
        t.hits[j] = clamp_count((int)q2.x), t.miss[j] = clamp_count((int)q2.y), t.age[j] = clamp_count((int)q2.z);
        t.score[j] = (int)q2.w, t.k[j] = (int)q3.x;
      }
    }
  }
  int next_id = a.clock[s * 4];
  next_id = next_id < 1 ? 1 : next_id;
  const int seen = a.clock[s * 4 + 1];

  for (int f = 0; f < a.F; ++f) {
    const int i = s * a.F + f;
    const int32_t* rows = a.dets + (size_t)i * a.D * 8;
    // step 1
    float px0[kSets], py0[kSets], px1[kSets], py1[kSets], pa[kSets], g[kSets];
#pragma unroll
    for (int j = 0; j < kSets; ++j) {
      g[j] = (float)(t.miss[j] + 1);
      const float fw = (float)t.w[j], fh = (float)t.h[j];
      px0[j] = __fadd_rn((float)t.x[j], __fmul_rn(__int_as_float(t.vx[j]), g[j]));
      py0[j] = __fadd_rn((float)t.y[j], __fmul_rn(__int_as_float(t.vy[j]), g[j]));
      px1[j] = __fadd_rn(px0[j], fw), py1[j] = __fadd_rn(py0[j], fh);
      pa[j] = __fmul_rn(fw, fh);
    }
    u32 matched = 0;    // bit j: the track of set j was matched in this frame
    u64 my_births = 0;  // lane c: the rows of group c that may start a track

    // steps 2 - 4
    for (int c = 0; c * 64 < a.D; ++c) {
      const int r = c * 64 + lane;
      int d[8] = {-1, 0, 0, 0, 0, 0, 0, 0};
      if (r < a.D)
        load_det(rows + (size_t)r * 8, d);
      const bool valid = r < a.D && d[0] == i && d[3] >= 1 && d[4] >= 1;
      int r_slot = -1, r_id = 0, r_hits = 0;
      u64 births = 0;
      u64 todo = __ballot(valid);
      while (todo) {
        const int b = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        // the row's values reach every lane as scalars; its box is formed from them again, which costs no register that
        // has to last
        const int rx = lane_i(d[1], b), ry = lane_i(d[2], b), rw = lane_i(d[3], b), rh = lane_i(d[4], b);
        const int bcls = lane_i(d[5], b), rscore = lane_i(d[6], b), rk = lane_i(d[7], b);
        const float bx0 = (float)rx, by0 = (float)ry, bw = (float)rw, bh = (float)rh;
        const float bx1 = __fadd_rn(bx0, bw), by1 = __fadd_rn(by0, bh), ba = __fmul_rn(bw, bh);
        u64 key = 0;
#pragma unroll
        for (int j = 0; j < kSets; ++j) {
          if (j * 64 < a.T) {
            const bool cand = t.id[j] >= 1 && !((matched >> j) & 1u) && (a.agnostic || t.cls[j] == bcls);
            const float iw = __fsub_rn(bx1 < px1[j] ? bx1 : px1[j], bx0 > px0[j] ? bx0 : px0[j]);
            const float ih = __fsub_rn(by1 < py1[j] ? by1 : py1[j], by0 > py0[j] ? by0 : py0[j]);
            if (cand && iw > 0.0f && ih > 0.0f) {
              const float inter = __fmul_rn(iw, ih);
              const float uni = __fsub_rn(__fadd_rn(pa[j], ba), inter);
              const float iou = __fdiv_rn(inter, uni);
              // inter and uni are positive: iou is no negative number, and such floats order as their bits
              if (iou > a.iou_thr) {
                const u64 k = ((u64)__float_as_uint(iou) << 32) | (u64)(0xFFFFFFFFu - (u32)(j * 64 + lane));
                key = k > key ? k : key;
              }
            }
          }
        }
        const u64 have = __ballot(key != 0);
        if (have == 0) {
          if (__int_as_float(rscore) >= a.new_thr)
            births |= 1ull << b;
          continue;
        }
        u64 best;
        if ((have & (have - 1)) == 0) {
          best = lane_u64(key, __ffsll((unsigned long long)have) - 1);
        } else {
          best = key;
#pragma unroll
          for (int o = 32; o >= 1; o >>= 1) {
            const u32 lo = (u32)__shfl_xor((int)(u32)best, o), hi = (u32)__shfl_xor((int)(u32)(best >> 32), o);
            const u64 other = ((u64)hi << 32) | lo;
            best = other > best ? other : best;
          }
          best = lane_u64(best, 0);
        }
        const int ws = (int)(0xFFFFFFFFu - (u32)best);
        int w_id = 0, w_hits = 0;
#pragma unroll
        for (int j = 0; j < kSets; ++j) {
          if (ws == j * 64 + lane) {
            const long long ddx = (2ll * rx + rw) - (2ll * t.x[j] + t.w[j]), ddy = (2ll * ry + rh) - (2ll * t.y[j] + t.h[j]);
            const float sx = __fdiv_rn(__fmul_rn((float)ddx, 0.5f), g[j]), sy = __fdiv_rn(__fmul_rn((float)ddy, 0.5f), g[j]);
            const float vx = __int_as_float(t.vx[j]), vy = __int_as_float(t.vy[j]);
            t.vx[j] = __float_as_int(__fadd_rn(vx, __fmul_rn(a.momentum, __fsub_rn(sx, vx))));
            t.vy[j] = __float_as_int(__fadd_rn(vy, __fmul_rn(a.momentum, __fsub_rn(sy, vy))));
            t.x[j] = rx, t.y[j] = ry, t.w[j] = rw, t.h[j] = rh, t.cls[j] = bcls, t.score[j] = rscore, t.k[j] = rk;
            t.hits[j] = sat_inc(t.hits[j]), t.miss[j] = 0, t.age[j] = sat_inc(t.age[j]);
            matched |= 1u << j;
            w_id = t.id[j], w_hits = t.hits[j];
          }
        }
        w_id = lane_i(w_id, ws & 63), w_hits = lane_i(w_hits, ws & 63);
        if (lane == b)
          r_slot = ws, r_id = w_id, r_hits = w_hits;
      }
      if (lane == c)
        my_births = births;
      if (r < a.D)
        put_outputs(out, i, r, d, r_slot, r_id, r_hits);
    }

    // step 5
#pragma unroll
    for (int j = 0; j < kSets; ++j) {
      if (t.id[j] >= 1 && !((matched >> j) & 1u)) {
        t.miss[j] = sat_inc(t.miss[j]), t.age[j] = sat_inc(t.age[j]);
        if (t.miss[j] > a.max_age || t.hits[j] < a.min_hits)
          free_slot(t, j);
      }
    }

    // step 6; a born row's outputs are written again by the lane that wrote them above
    bool full = false;
    for (int c = 0; c * 64 < a.D && !full; ++c) {
      u64 births = lane_u64(my_births, c);
      if (births == 0)
        continue;
      const int r = c * 64 + lane;
      int d[8] = {-1, 0, 0, 0, 0, 0, 0, 0};
      if (r < a.D)
        load_det(rows + (size_t)r * 8, d);
      int r_slot = -1, r_id = 0;
      while (births) {
        const int b = __ffsll((unsigned long long)births) - 1;
        births &= births - 1;
        int fs = -1;
#pragma unroll
        for (int j = 0; j < kSets; ++j) {
          const u64 free = __ballot(t.id[j] == 0 && j * 64 + lane < a.T);
          if (fs < 0 && free != 0)
            fs = j * 64 + __ffsll((unsigned long long)free) - 1;
        }
        if (fs < 0) {
          full = true;
          break;
        }
        const int id = next_id;
        next_id = next_id == INT_MAX ? 1 : next_id + 1;
        const int rx = lane_i(d[1], b), ry = lane_i(d[2], b), rw = lane_i(d[3], b), rh = lane_i(d[4], b);
        const int rcls = lane_i(d[5], b), rscore = lane_i(d[6], b), rk = lane_i(d[7], b);
#pragma unroll
        for (int j = 0; j < kSets; ++j) {
          if (fs == j * 64 + lane) {
            t.id[j] = id, t.cls[j] = rcls, t.x[j] = rx, t.y[j] = ry, t.w[j] = rw, t.h[j] = rh, t.vx[j] = 0, t.vy[j] = 0;
            t.hits[j] = 1, t.miss[j] = 0, t.age[j] = 1, t.score[j] = rscore, t.k[j] = rk;
          }
        }
        if (lane == b)
          r_slot = fs, r_id = id;
      }
      if (r_slot >= 0)
        put_outputs(out, i, r, d, r_slot, r_id, 1);
    }
  }

#pragma unroll
  for (int j = 0; j < kSets; ++j) {
    const int slot = j * 64 + lane;
    if (slot < a.T) {
      int32_t* p = mine + (size_t)slot * 16;
      store16(p, make_uint4((u32)t.id[j], (u32)t.cls[j], (u32)t.x[j], (u32)t.y[j]));
      store16(p + 4, make_uint4((u32)t.w[j], (u32)t.h[j], (u32)t.vx[j], (u32)t.vy[j]));
      store16(p + 8, make_uint4((u32)t.hits[j], (u32)t.miss[j], (u32)t.age[j], (u32)t.score[j]));
      store16(p + 12, make_uint4((u32)t.k[j], 0u, 0u, 0u));
    }
  }
  if (lane == 0) {
    int32_t* p = a.clock + s * 4;
    p[0] = next_id, p[1] = (int)((u32)seen + (u32)a.F), p[2] = 0, p[3] = 0;
  }
}

} // namespace
} // namespace vali

using namespace vali;

extern "C" {

int vali_track_update(const vali_track_params* params, const vali_track_io* io, vali_stream_t stream) {
  VALI_REQUIRE(params && io, "null argument");
  VALI_REQUIRE(io->dets && io->tracks && io->clock && io->tracked, "null dets, tracks, clock or tracked");
  const int S = params->streams, F = params->frames, D = params->max_det, T = params->max_tracks;
  VALI_REQUIRE(S >= 1 && S <= kMaxN, "streams outside 1..1024");
  VALI_REQUIRE(F >= 1 && (long long)S * F <= kMaxN, "frames below 1, or streams * frames above 1024");
  VALI_REQUIRE(D >= 1 && D <= kMaxD, "max_det outside 1..1024");
  const int n = S * F;
  VALI_REQUIRE((long long)n * D <= 65535, "n * max_det exceeds 65535");
  VALI_REQUIRE(T >= 1 && T <= kMaxT, "max_tracks outside 1..256");
  VALI_REQUIRE(aligned16(io->tracks), "tracks are not 16-byte aligned");
  VALI_REQUIRE((((uintptr_t)io->dets | (uintptr_t)io->clock | (uintptr_t)io->tracked | (uintptr_t)io->assoc |
                 (uintptr_t)io->marks | (uintptr_t)io->colours | (uintptr_t)io->label_rects) & 3u) == 0,
               "an array is not 4-byte aligned");
  VALI_REQUIRE(isfinite(params->iou_thr), "iou_thr is not finite");
  VALI_REQUIRE(isfinite(params->new_thr), "new_thr is not finite");
  VALI_REQUIRE(params->momentum >= 0.0f && params->momentum <= 1.0f, "momentum outside 0..1");
  VALI_REQUIRE(params->min_hits >= 1, "min_hits below 1");
  VALI_REQUIRE(params->max_age >= 0 && params->max_age <= kMaxAge, "max_age outside 0..2^20");
  if (io->marks) {
    VALI_REQUIRE(io->colours && params->n_colours >= 1, "marks without colours");
    VALI_REQUIRE((long long)(io->label_rects ? 3 : 1) * n * D <= VALI_MAX_MARKS, "more than 4096 mark rows");
    VALI_REQUIRE(params->thickness >= 1, "thickness below 1");
    VALI_REQUIRE(params->label_alpha >= 0 && params->label_alpha <= 255, "label_alpha outside 0..255");
    VALI_REQUIRE(!io->label_rects || params->n_labels >= 1, "label_rects without n_labels");
  }

  TrackArgs a = {};
  a.dets = io->dets, a.tracks = io->tracks, a.clock = io->clock, a.tracked = io->tracked, a.assoc = io->assoc;
  a.ms = {io->marks, io->colours, io->label_rects, params->n_colours, params->n_labels, params->thickness,
          params->label_alpha, params->text_colour};
  a.F = F, a.D = D, a.T = T, a.M = n * D;
  a.iou_thr = params->iou_thr, a.new_thr = params->new_thr, a.momentum = params->momentum;
  a.min_hits = params->min_hits, a.max_age = params->max_age, a.agnostic = params->class_agnostic != 0;

  hipStream_t s = as_stream(stream);
  VALI_ENTRY(s);
  hipLaunchKernelGGL(k_track_update, dim3(S), dim3(64), 0, s, a);
  VALI_LAUNCH_CHECK();
  return VALI_OK;
}

} // extern "C"
