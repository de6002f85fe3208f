/* A plain C99 client of vali_semantic_paint (include/vali_hip.h).
 * One tightly packed RGB frame of w x h comes from a file, with float32 logits (1, c, hs, ws), the frame's record of 8
 * int32 and nc packed colours.  One call writes the labels into a Y surface and paints the classes; both are read back,
 * written to got.bin (the frame, then the labels) and compared with want.bin, which tests/test_gpu_c_abi_semantic.py
 * wrote with tests/semantic_model.py.
 *   usage: semantic_client <w> <h> <c> <hs> <ws> <net_w> <net_h> <nc> <alpha> <frame.bin> <logits.bin> <rect.bin>
 *                          <colours.bin> <want.bin> <got.bin>
 * exit status 0: equal; 5: frame or labels differ (got.bin holds what was made); 4: a refusal did not come. */
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
  if (argc != 16) {
    fprintf(stderr, "usage: %s w h c hs ws net_w net_h nc alpha frame logits rect colours want got\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[1]), h = atoi(argv[2]), c = atoi(argv[3]), hs = atoi(argv[4]), ws = atoi(argv[5]);
  const int net_w = atoi(argv[6]), net_h = atoi(argv[7]), nc = atoi(argv[8]), alpha = atoi(argv[9]);
  const int dev = 0;
  if (w < 1 || h < 1 || c < 1 || hs < 1 || ws < 1 || nc < 1) return 2;
  const size_t fbytes = (size_t)w * h * 3, lbytes = (size_t)w * h, gbytes = (size_t)c * hs * ws * sizeof(float);
  unsigned char* frame = read_file(argv[10], fbytes);
  unsigned char* logits = read_file(argv[11], gbytes);
  unsigned char* rect = read_file(argv[12], sizeof(vali_roi));
  unsigned char* colours = read_file(argv[13], nc * sizeof(int32_t));
  unsigned char* want = read_file(argv[14], fbytes + lbytes);
  unsigned char* got = (unsigned char*)malloc(fbytes + lbytes);
  if (!frame || !logits || !rect || !colours || !want || !got) return 2;
  memset(got + fbytes, 0x5a, lbytes);

  int count = 0;
  CHECK(vali_device_count(&count));
  if (count < 1) {
    fprintf(stderr, "no device\n");
    return 3;
  }
  vali_stream_t stream = NULL;
  CHECK(vali_stream_create(dev, &stream));

  void *d_frame = NULL, *d_lab = NULL, *d_logits = NULL, *d_rect = NULL, *d_colours = NULL, *d_desc = NULL, *d_ldesc = NULL;
  if (upload(dev, &d_frame, frame, fbytes, stream) || upload(dev, &d_lab, got + fbytes, lbytes, stream) ||
      upload(dev, &d_logits, logits, gbytes, stream) || upload(dev, &d_rect, rect, sizeof(vali_roi), stream) ||
      upload(dev, &d_colours, colours, nc * sizeof(int32_t), stream))
    return 1;
  vali_surface desc, ldesc;
  memset(&desc, 0, sizeof desc);
  desc.plane[0] = d_frame;
  desc.pitch[0] = 3 * w;
  desc.width = w; desc.height = h; desc.format = VALI_FMT_RGB;
  memset(&ldesc, 0, sizeof ldesc);
  ldesc.plane[0] = d_lab;
  ldesc.pitch[0] = w;
  ldesc.width = w; ldesc.height = h; ldesc.format = VALI_FMT_Y;
  if (upload(dev, &d_desc, &desc, sizeof desc, stream) || upload(dev, &d_ldesc, &ldesc, sizeof ldesc, stream)) return 1;

  vali_semantic_in in;
  memset(&in, 0, sizeof in);
  in.logits.data = d_logits; in.logits.dtype = VALI_DTYPE_F32;
  in.logits.stride_n = (int64_t)c * hs * ws; in.logits.stride_m = (int64_t)hs * ws; in.logits.stride_y = ws;
  in.c = c; in.hs = hs; in.ws = ws; in.net_w = net_w; in.net_h = net_h;

#define PAINT(FRAMES, DFRAMES, N, FMT, IN, RECTS, LABS, DLABS, COLS, NC, ALPHA)                                     \
  vali_semantic_paint(FRAMES, (const vali_surface*)(DFRAMES), N, FMT, IN, (const vali_roi*)(RECTS), LABS,            \
                      (const vali_surface*)(DLABS), (const int32_t*)(COLS), NC, ALPHA, NULL, stream)
  /* refusals are decided on the host, before anything is launched */
  vali_semantic_in bad = in;
  bad.c = 256;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &bad, d_rect, &ldesc, d_ldesc, d_colours, nc, alpha) != VALI_ERR_INVALID_ARG) return 4;
  bad = in;
  bad.ws = 4097;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &bad, d_rect, &ldesc, d_ldesc, d_colours, nc, alpha) != VALI_ERR_INVALID_ARG) return 4;
  bad = in;
  bad.net_w = 0;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &bad, d_rect, &ldesc, d_ldesc, d_colours, nc, alpha) != VALI_ERR_INVALID_ARG) return 4;
  bad = in;
  bad.logits.dtype = 3;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &bad, d_rect, &ldesc, d_ldesc, d_colours, nc, alpha) != VALI_ERR_INVALID_ARG) return 4;
  bad = in;
  bad.logits.data = (const char*)d_logits + 2;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &bad, d_rect, &ldesc, d_ldesc, d_colours, nc, alpha) != VALI_ERR_INVALID_ARG) return 4;
  bad = in;
  bad.logits.stride_y = -1;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &bad, d_rect, &ldesc, d_ldesc, d_colours, nc, alpha) != VALI_ERR_INVALID_ARG) return 4;
  bad = in;
  bad.logits.data = NULL;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &bad, d_rect, &ldesc, d_ldesc, d_colours, nc, alpha) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, NULL, d_rect, &ldesc, d_ldesc, d_colours, nc, alpha) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, NULL, &ldesc, d_ldesc, d_colours, nc, alpha) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_rect, &ldesc, NULL, d_colours, nc, alpha) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_rect, NULL, d_ldesc, d_colours, nc, alpha) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_rect, NULL, NULL, NULL, nc, alpha) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_rect, &ldesc, d_ldesc, d_colours, 0, alpha) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_rect, &ldesc, d_ldesc, d_colours, nc, 256) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_BGR, &in, d_rect, &ldesc, d_ldesc, d_colours, nc, alpha) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_Y, &in, d_rect, &ldesc, d_ldesc, d_colours, nc, alpha) != VALI_ERR_UNSUPPORTED) return 4;
  if (PAINT(&desc, d_desc, 0, VALI_FMT_RGB, &in, d_rect, &ldesc, d_ldesc, d_colours, nc, alpha) != VALI_ERR_INVALID_ARG) return 4;
  vali_surface lbad = ldesc;
  lbad.format = VALI_FMT_RGB;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_rect, &lbad, d_ldesc, d_colours, nc, alpha) != VALI_ERR_INVALID_ARG) return 4;
  lbad = ldesc;
  lbad.height = h + 1;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_rect, &lbad, d_ldesc, d_colours, nc, alpha) != VALI_ERR_INVALID_ARG) return 4;

  CHECK(PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_rect, &ldesc, d_ldesc, d_colours, nc, alpha));
  CHECK(vali_memcpy2d_async(dev, got, fbytes, d_frame, fbytes, fbytes, 1, 1, stream));
  CHECK(vali_memcpy2d_async(dev, got + fbytes, lbytes, d_lab, lbytes, lbytes, 1, 1, stream));
  CHECK(vali_stream_sync(dev, stream));
  FILE* o = fopen(argv[15], "wb");
  if (!o || fwrite(got, 1, fbytes + lbytes, o) != fbytes + lbytes) return 2;
  fclose(o);
  const int equal = memcmp(got, want, fbytes + lbytes) == 0;

  vali_mem_free(dev, d_frame); vali_mem_free(dev, d_lab); vali_mem_free(dev, d_logits); vali_mem_free(dev, d_rect);
  vali_mem_free(dev, d_colours); vali_mem_free(dev, d_desc); vali_mem_free(dev, d_ldesc);
  vali_stream_destroy(dev, stream);
  free(frame); free(logits); free(rect); free(colours); free(want); free(got);
  if (!equal) {
    fprintf(stderr, "the painted frame or the labels differ from want.bin\n");
    return 5;
  }
  printf("ok %s\n", vali_version());
  return 0;
}
