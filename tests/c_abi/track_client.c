/* A plain C99 client of vali_track_update (include/vali_hip.h).
 * A sequence of calls on one state: dets.bin holds `calls` times (s * f * d) rows of 8 int32, one block per call.  The
 * state starts all zero.  Every call has all three outputs (three colours, no labels; iou_thr 0.3, new_thr 0.5, momentum
 * 0.5, min_hits 2, max_age 3, thickness 2); after every call tracks (s * t rows of 16), clock (s rows of 4), tracked
 * (n * d rows of 8), assoc (n * d rows of 4) and marks (n * d rows of 8) are read back and appended, in that order, to
 * got.bin, which is compared with want.bin: tests/test_gpu_c_abi_track.py wrote it with tests/track_model.py.
 *   usage: track_client <s> <f> <d> <t> <calls> <dets.bin> <want.bin> <got.bin>
 * exit status 0: equal; 5: the outputs differ (got.bin holds them); 4: a refusal did not come. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "vali_hip.h"

#define CHECK(call)                                                              \
  do {                                                                           \
    int rc_ = (call);                                                            \
    if (rc_ != VALI_OK) {                                                        \
      fprintf(stderr, "%s -> %d: %s\n", #call, rc_, vali_last_error());         \
      return 1;                                                                  \
    }                                                                            \
  } while (0)

static unsigned char* read_file(const char* path, size_t bytes) {
  unsigned char* p = (unsigned char*)malloc(bytes ? bytes : 1);
  FILE* f = fopen(path, "rb");
  if (!p || !f || fread(p, 1, bytes, f) != bytes) {
    fprintf(stderr, "cannot read %lu bytes of %s\n", (unsigned long)bytes, path);
    return NULL;
  }
  fclose(f);
  return p;
}

int main(int argc, char** argv) {
  if (argc != 9) {
    fprintf(stderr, "usage: %s s f d t calls dets.bin want.bin got.bin\n", argv[0]);
    return 2;
  }
  const int s = atoi(argv[1]), f = atoi(argv[2]), d = atoi(argv[3]), t = atoi(argv[4]), calls = atoi(argv[5]), dev = 0;
  if (s < 1 || f < 1 || d < 1 || t < 1 || calls < 1) return 2;
  const size_t rows = (size_t)s * f * d, det_bytes = rows * 8 * sizeof(int32_t);
  const size_t state_bytes = ((size_t)s * t * 16 + (size_t)s * 4) * sizeof(int32_t);      /* tracks, then clock */
  const size_t out_bytes = rows * (8 + 4 + 8) * sizeof(int32_t);                          /* tracked, assoc, marks */
  const size_t per_call = state_bytes + out_bytes, total = per_call * calls;
  unsigned char* dets = read_file(argv[6], det_bytes * calls);
  unsigned char* want = read_file(argv[7], total);
  unsigned char* got = (unsigned char*)malloc(total);
  if (!dets || !want || !got) return 2;

  int count = 0;
  CHECK(vali_device_count(&count));
  if (count < 1) {
    fprintf(stderr, "no device\n");
    return 3;
  }
  vali_stream_t stream = NULL;
  CHECK(vali_stream_create(dev, &stream));

  const int32_t colours[3] = {(int32_t)0xff28ff50u, (int32_t)0x80ff0000u, 0x00010203};
  void *d_dets = NULL, *d_colours = NULL, *d_all = NULL;
  CHECK(vali_mem_alloc(dev, det_bytes, &d_dets));
  CHECK(vali_mem_alloc(dev, sizeof colours, &d_colours));
  CHECK(vali_memcpy2d_async(dev, d_colours, sizeof colours, colours, sizeof colours, sizeof colours, 1, 0, stream));
  CHECK(vali_mem_alloc(dev, per_call, &d_all));
  CHECK(vali_memset2d_async(dev, d_all, state_bytes, 0, state_bytes, 1, stream));         /* no tracks */

  vali_track_params prm;
  memset(&prm, 0, sizeof prm);
  prm.streams = s; prm.frames = f; prm.max_det = d; prm.max_tracks = t;
  prm.iou_thr = 0.3f; prm.new_thr = 0.5f; prm.momentum = 0.5f;
  prm.min_hits = 2; prm.max_age = 3;
  prm.thickness = 2; prm.n_colours = 3;
  vali_track_io io;
  memset(&io, 0, sizeof io);
  io.dets = (const int32_t*)d_dets;
  io.tracks = (int32_t*)d_all;
  io.clock = io.tracks + (size_t)s * t * 16;
  io.tracked = io.clock + (size_t)s * 4;
  io.assoc = io.tracked + rows * 8;
  io.marks = io.assoc + rows * 4;
  io.colours = (const int32_t*)d_colours;

  /* refusals are decided on the host, before anything is launched */
  vali_track_params bad = prm;
  bad.max_tracks = 257;
  if (vali_track_update(&bad, &io, stream) != VALI_ERR_INVALID_ARG) return 4;
  bad = prm;
  bad.momentum = 1.5f;
  if (vali_track_update(&bad, &io, stream) != VALI_ERR_INVALID_ARG) return 4;
  bad = prm;
  bad.n_colours = 0;
  if (vali_track_update(&bad, &io, stream) != VALI_ERR_INVALID_ARG) return 4;
  vali_track_io bad_io = io;
  bad_io.tracks = io.tracks + 1;
  if (vali_track_update(&prm, &bad_io, stream) != VALI_ERR_INVALID_ARG) return 4;
  bad_io = io;
  bad_io.tracked = NULL;
  if (vali_track_update(&prm, &bad_io, stream) != VALI_ERR_INVALID_ARG) return 4;
  if (vali_track_update(&prm, NULL, stream) != VALI_ERR_INVALID_ARG) return 4;

  for (int c = 0; c < calls; ++c) {
    CHECK(vali_memcpy2d_async(dev, d_dets, det_bytes, dets + det_bytes * c, det_bytes, det_bytes, 1, 0, stream));
    CHECK(vali_memset2d_async(dev, (unsigned char*)d_all + state_bytes, out_bytes, 0x5a, out_bytes, 1, stream));
    CHECK(vali_track_update(&prm, &io, stream));
    CHECK(vali_memcpy2d_async(dev, got + per_call * c, per_call, d_all, per_call, per_call, 1, 1, stream));
    CHECK(vali_stream_sync(dev, stream));         /* dets + det_bytes * c is host memory the next copy replaces */
  }
  FILE* o = fopen(argv[8], "wb");
  if (!o || fwrite(got, 1, total, o) != total) return 2;
  fclose(o);
  const int equal = memcmp(got, want, total) == 0;

  vali_mem_free(dev, d_dets); vali_mem_free(dev, d_colours); vali_mem_free(dev, d_all);
  vali_stream_destroy(dev, stream);
  free(dets); free(want); free(got);
  if (!equal) {
    fprintf(stderr, "the outputs differ from want.bin\n");
    return 5;
  }
  printf("ok %s\n", vali_version());
  return 0;
}
