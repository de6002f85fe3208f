/* A plain C99 client of vali_detect_select (include/vali_hip.h).
 * A float32 head comes from two files, (n, k, 4) boxes and (n, k, c) scores, tightly packed; the frame records from a file
 * of n x 8 int32.  One call with all four outputs (three colours, no labels, thresholds 0.25 / 0.45, crop placement
 * 0, 0, 224, 224, thickness 2); dets (n * d rows), counts (n), rois and marks (n * d rows each) are read back, written to
 * got.bin in that order and compared with want.bin, which tests/test_gpu_c_abi_detect.py wrote with tests/detect_model.py.
 *   usage: detect_client <n> <k> <c> <t> <d> <boxes.bin> <scores.bin> <rects.bin> <want.bin> <got.bin>
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

static int upload(int dev, void** d, const void* host, size_t bytes, vali_stream_t stream) {
  CHECK(vali_mem_alloc(dev, bytes, d));
  CHECK(vali_memcpy2d_async(dev, *d, bytes, host, bytes, bytes, 1, 0, stream));
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 11) {
    fprintf(stderr, "usage: %s n k c t d boxes.bin scores.bin rects.bin want.bin got.bin\n", argv[0]);
    return 2;
  }
  const int n = atoi(argv[1]), k = atoi(argv[2]), c = atoi(argv[3]), t = atoi(argv[4]), d = atoi(argv[5]), dev = 0;
  if (n < 1 || k < 1 || c < 1 || t < 1 || d < 1) return 2;
  const size_t bbytes = (size_t)n * k * 4 * sizeof(float), sbytes = (size_t)n * k * c * sizeof(float);
  const size_t rows = (size_t)n * d, rbytes = rows * 8 * sizeof(int32_t), total = 3 * rbytes + (size_t)n * sizeof(int32_t);
  unsigned char* boxes = read_file(argv[6], bbytes);
  unsigned char* scores = read_file(argv[7], sbytes);
  unsigned char* rects = read_file(argv[8], (size_t)n * sizeof(vali_roi));
  unsigned char* want = read_file(argv[9], total);
  unsigned char* got = (unsigned char*)malloc(total);
  if (!boxes || !scores || !rects || !want || !got) return 2;

  int count = 0;
  CHECK(vali_device_count(&count));
  if (count < 1) {
    fprintf(stderr, "no device\n");
    return 3;
  }
  vali_stream_t stream = NULL;
  CHECK(vali_stream_create(dev, &stream));

  const int32_t colours[3] = {(int32_t)0xff28ff50u, (int32_t)0x80ff0000u, 0x00010203};
  void *d_boxes = NULL, *d_scores = NULL, *d_rects = NULL, *d_colours = NULL, *d_out = NULL, *ws = NULL;
  if (upload(dev, &d_boxes, boxes, bbytes, stream) || upload(dev, &d_scores, scores, sbytes, stream) ||
      upload(dev, &d_rects, rects, (size_t)n * sizeof(vali_roi), stream) ||
      upload(dev, &d_colours, colours, sizeof colours, stream))
    return 1;
  CHECK(vali_mem_alloc(dev, total, &d_out));
  CHECK(vali_memset2d_async(dev, d_out, total, 0x5a, total, 1, stream));
  const size_t ws_bytes = vali_detect_workspace_size(n, k, t);
  if (ws_bytes == 0 || vali_detect_workspace_size(n, k, 1025) != 0) return 4;
  CHECK(vali_mem_alloc(dev, ws_bytes, &ws));

  vali_detect_in in;
  memset(&in, 0, sizeof in);
  in.boxes.data = d_boxes; in.boxes.dtype = VALI_DTYPE_F32;
  in.boxes.stride_n = (int64_t)k * 4; in.boxes.stride_k = 4; in.boxes.stride_c = 1;
  in.scores.data = d_scores; in.scores.dtype = VALI_DTYPE_F32;
  in.scores.stride_n = (int64_t)k * c; in.scores.stride_k = c; in.scores.stride_c = 1;
  in.n = n; in.k = k; in.c = c;
  vali_detect_params prm;
  memset(&prm, 0, sizeof prm);
  prm.max_candidates = t; prm.max_det = d;
  prm.score_thr = 0.25f; prm.iou_thr = 0.45f;
  prm.box_format = VALI_DETECT_XYXY;
  prm.crop[2] = 224; prm.crop[3] = 224;
  prm.thickness = 2; prm.n_colours = 3;
  vali_detect_out out;
  memset(&out, 0, sizeof out);
  out.dets = (int32_t*)d_out;
  out.counts = out.dets + rows * 8;
  out.rois = out.counts + n;
  out.marks = out.rois + rows * 8;
  out.colours = (const int32_t*)d_colours;

  /* refusals are decided on the host, before anything is launched */
  vali_detect_params bad = prm;
  bad.max_det = t + 1;
  if (vali_detect_select(&in, &bad, (const vali_roi*)d_rects, &out, ws, ws_bytes, stream) != VALI_ERR_INVALID_ARG) return 4;
  bad = prm;
  bad.n_colours = 0;
  if (vali_detect_select(&in, &bad, (const vali_roi*)d_rects, &out, ws, ws_bytes, stream) != VALI_ERR_INVALID_ARG) return 4;
  if (vali_detect_select(&in, &prm, (const vali_roi*)d_rects, &out, ws, ws_bytes - 1, stream) != VALI_ERR_INVALID_ARG) return 4;
  if (vali_detect_select(&in, &prm, NULL, &out, ws, ws_bytes, stream) != VALI_ERR_INVALID_ARG) return 4;

  CHECK(vali_detect_select(&in, &prm, (const vali_roi*)d_rects, &out, ws, ws_bytes, stream));
  CHECK(vali_memcpy2d_async(dev, got, total, d_out, total, total, 1, 1, stream));
  CHECK(vali_stream_sync(dev, stream));
  FILE* o = fopen(argv[10], "wb");
  if (!o || fwrite(got, 1, total, o) != total) return 2;
  fclose(o);
  const int equal = memcmp(got, want, total) == 0;

  vali_mem_free(dev, d_boxes); vali_mem_free(dev, d_scores); vali_mem_free(dev, d_rects); vali_mem_free(dev, d_colours);
  vali_mem_free(dev, d_out); vali_mem_free(dev, ws);
  vali_stream_destroy(dev, stream);
  free(boxes); free(scores); free(rects); free(want); free(got);
  if (!equal) {
    fprintf(stderr, "the outputs differ from want.bin\n");
    return 5;
  }
  printf("ok %s\n", vali_version());
  return 0;
}
