/* A plain C99 client of vali_mask_workspace_size / vali_mask_paint (include/vali_hip.h).
 * One tightly packed RGB frame of w x h comes from a file, with float32 prototypes (1, m, hp, wp), float32 coefficients
 * (1, k, m), d detection rows of 8 int32, the frame's record of 8 int32 and three packed colours.  One call paints the
 * masks; the frame is read back, written to got.bin and compared with want.bin, which tests/test_gpu_c_abi_masks.py wrote
 * with tests/mask_model.py.
 *   usage: mask_client <w> <h> <m> <hp> <wp> <k> <d> <net_w> <net_h> <alpha> <frame.bin> <protos.bin> <coeffs.bin>
 *                      <dets.bin> <rect.bin> <colours.bin> <want.bin> <got.bin>
 * exit status 0: equal; 5: the frames differ (got.bin holds the painted one); 4: a refusal did not come. */
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
  if (argc != 19) {
    fprintf(stderr, "usage: %s w h m hp wp k d net_w net_h alpha frame protos coeffs dets rect colours want got\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[1]), h = atoi(argv[2]), m = atoi(argv[3]), hp = atoi(argv[4]), wp = atoi(argv[5]);
  const int k = atoi(argv[6]), d = atoi(argv[7]), net_w = atoi(argv[8]), net_h = atoi(argv[9]), alpha = atoi(argv[10]);
  const int dev = 0;
  if (w < 1 || h < 1 || m < 1 || hp < 1 || wp < 1 || k < 1 || d < 1) return 2;
  const size_t fbytes = (size_t)w * h * 3, pbytes = (size_t)m * hp * wp * sizeof(float);
  const size_t cbytes = (size_t)k * m * sizeof(float), dbytes = (size_t)d * 8 * sizeof(int32_t);
  unsigned char* frame = read_file(argv[11], fbytes);
  unsigned char* protos = read_file(argv[12], pbytes);
  unsigned char* coeffs = read_file(argv[13], cbytes);
  unsigned char* dets = read_file(argv[14], dbytes);
  unsigned char* rect = read_file(argv[15], sizeof(vali_roi));
  unsigned char* colours = read_file(argv[16], 3 * sizeof(int32_t));
  unsigned char* want = read_file(argv[17], fbytes);
  unsigned char* got = (unsigned char*)malloc(fbytes);
  if (!frame || !protos || !coeffs || !dets || !rect || !colours || !want || !got) return 2;

  int count = 0;
  CHECK(vali_device_count(&count));
  if (count < 1) {
    fprintf(stderr, "no device\n");
    return 3;
  }
  vali_stream_t stream = NULL;
  CHECK(vali_stream_create(dev, &stream));

  void *d_frame = NULL, *d_protos = NULL, *d_coeffs = NULL, *d_dets = NULL, *d_rect = NULL, *d_colours = NULL;
  void *d_desc = NULL, *ws = NULL;
  if (upload(dev, &d_frame, frame, fbytes, stream) || upload(dev, &d_protos, protos, pbytes, stream) ||
      upload(dev, &d_coeffs, coeffs, cbytes, stream) || upload(dev, &d_dets, dets, dbytes, stream) ||
      upload(dev, &d_rect, rect, sizeof(vali_roi), stream) || upload(dev, &d_colours, colours, 3 * sizeof(int32_t), stream))
    return 1;
  vali_surface desc;
  memset(&desc, 0, sizeof desc);
  desc.plane[0] = d_frame;
  desc.pitch[0] = 3 * w;
  desc.width = w; desc.height = h; desc.format = VALI_FMT_RGB;
  if (upload(dev, &d_desc, &desc, sizeof desc, stream)) return 1;

  const size_t ws_bytes = vali_mask_workspace_size(1, d, hp, wp);
  if (ws_bytes != (size_t)d * hp * wp * 4 || vali_mask_workspace_size(1, d, 1025, wp) != 0 ||
      vali_mask_workspace_size(1, 1025, hp, wp) != 0 || vali_mask_workspace_size(0, d, hp, wp) != 0)
    return 4;
  CHECK(vali_mem_alloc(dev, ws_bytes, &ws));

  vali_mask_in in;
  memset(&in, 0, sizeof in);
  in.protos.data = d_protos; in.protos.dtype = VALI_DTYPE_F32;
  in.protos.stride_n = (int64_t)m * hp * wp; in.protos.stride_m = (int64_t)hp * wp; in.protos.stride_y = wp;
  in.coeffs.data = d_coeffs; in.coeffs.dtype = VALI_DTYPE_F32;
  in.coeffs.stride_n = (int64_t)k * m; in.coeffs.stride_k = m; in.coeffs.stride_c = 1;
  in.m = m; in.hp = hp; in.wp = wp; in.k = k;
  in.max_det = d; in.net_w = net_w; in.net_h = net_h;

#define PAINT(FRAMES, DFRAMES, N, FMT, IN, DETS, RECTS, COLS, NC, ALPHA, WS, WSB)                                      \
  vali_mask_paint(FRAMES, (const vali_surface*)(DFRAMES), N, FMT, IN, (const int32_t*)(DETS), (const vali_roi*)(RECTS), \
                  (const int32_t*)(COLS), NC, ALPHA, NULL, WS, WSB, stream)
  /* refusals are decided on the host, before anything is launched */
  vali_mask_in bad = in;
  bad.m = 65;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &bad, d_dets, d_rect, d_colours, 3, alpha, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  bad = in;
  bad.net_w = 0;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &bad, d_dets, d_rect, d_colours, 3, alpha, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  bad = in;
  bad.protos.dtype = 3;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &bad, d_dets, d_rect, d_colours, 3, alpha, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  bad = in;
  bad.coeffs.stride_k = -1;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &bad, d_dets, d_rect, d_colours, 3, alpha, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, NULL, d_rect, d_colours, 3, alpha, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_dets, NULL, d_colours, 3, alpha, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_dets, d_rect, d_colours, 0, alpha, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_dets, d_rect, d_colours, 3, 256, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_dets, d_rect, d_colours, 3, alpha, ws, ws_bytes - 1) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_dets, d_rect, d_colours, 3, alpha, (char*)ws + 8, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_BGR, &in, d_dets, d_rect, d_colours, 3, alpha, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_Y, &in, d_dets, d_rect, d_colours, 3, alpha, ws, ws_bytes) != VALI_ERR_UNSUPPORTED) return 4;
  if (PAINT(&desc, d_desc, 0, VALI_FMT_RGB, &in, d_dets, d_rect, d_colours, 3, alpha, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;

  CHECK(PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_dets, d_rect, d_colours, 3, alpha, ws, ws_bytes));
  CHECK(vali_memcpy2d_async(dev, got, fbytes, d_frame, fbytes, fbytes, 1, 1, stream));
  CHECK(vali_stream_sync(dev, stream));
  FILE* o = fopen(argv[18], "wb");
  if (!o || fwrite(got, 1, fbytes, o) != fbytes) return 2;
  fclose(o);
  const int equal = memcmp(got, want, fbytes) == 0;

  vali_mem_free(dev, d_frame); vali_mem_free(dev, d_protos); vali_mem_free(dev, d_coeffs); vali_mem_free(dev, d_dets);
  vali_mem_free(dev, d_rect); vali_mem_free(dev, d_colours); vali_mem_free(dev, d_desc); vali_mem_free(dev, ws);
  vali_stream_destroy(dev, stream);
  free(frame); free(protos); free(coeffs); free(dets); free(rect); free(colours); free(want); free(got);
  if (!equal) {
    fprintf(stderr, "the painted frame differs from want.bin\n");
    return 5;
  }
  printf("ok %s\n", vali_version());
  return 0;
}
