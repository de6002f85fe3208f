/* A plain C99 client of the region encoder of include/vali_hip.h: upload a raw RGB picture into a pitched surface,
 * plan rectangles of it on the host (vali_jpeg_plan_rois), upload the records, encode them in one call
 * (vali_jpeg_encode_rois), download each image's bytes and write the files: header + device bytes + EOI.
 *   usage: jpeg_roi_client <in.rgb> <width> <height> <quality> <h_samp> <v_samp> <optimize> <out prefix> x,y,w,h ...
 * Prints "ok <n>" and exits 0 on success; prints vali_last_error() otherwise.
 * tests/test_gpu_c_abi_jpeg_roi.py compares the files with the model. */
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

#define MAX_ROIS 64

int main(int argc, char** argv) {
  if (argc < 10 || argc - 9 > MAX_ROIS) {
    fprintf(stderr, "usage: %s in.rgb width height quality h_samp v_samp optimize prefix x,y,w,h ...\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[2]), h = atoi(argv[3]), n = argc - 9;
  const size_t row = (size_t)w * 3;
  unsigned char* pixels = (unsigned char*)malloc(row * (size_t)h);
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(pixels, 1, row * (size_t)h, f) != row * (size_t)h)
    return 2;
  fclose(f);

  vali_jpeg_params params;
  CHECK(vali_jpeg_params_init_sampled(atoi(argv[4]), VALI_FMT_RGB, atoi(argv[5]), atoi(argv[6]), &params));
  params.optimize = atoi(argv[7]);
  vali_jpeg_roi rois[MAX_ROIS];
  int32_t src_w[MAX_ROIS], src_h[MAX_ROIS];
  for (int i = 0; i < n; ++i) {
    int x, y, rw, rh;
    if (sscanf(argv[9 + i], "%d,%d,%d,%d", &x, &y, &rw, &rh) != 4)
      return 2;
    rois[i].x = x, rois[i].y = y, rois[i].width = rw, rois[i].height = rh;
    src_w[i] = w, src_h[i] = h;
  }
  vali_jpeg_item* items = (vali_jpeg_item*)malloc((size_t)n * sizeof(vali_jpeg_item));
  size_t ws_bytes = 0, out_bytes = 0;
  CHECK(vali_jpeg_plan_rois(rois, src_w, src_h, n, &params, items, &ws_bytes, &out_bytes));

  const int dev = 0;
  vali_stream_t stream = NULL;
  CHECK(vali_stream_create(dev, &stream));
  void *d_rgb = NULL, *d_src = NULL, *d_items = NULL, *ws = NULL, *d_out = NULL, *d_sizes = NULL;
  size_t pitch = 0;
  CHECK(vali_mem_alloc_pitch(dev, row, (size_t)h, &d_rgb, &pitch));
  CHECK(vali_mem_alloc(dev, (size_t)n * sizeof(vali_surface), &d_src));
  CHECK(vali_mem_alloc(dev, (size_t)n * sizeof(vali_jpeg_item), &d_items));
  CHECK(vali_mem_alloc(dev, ws_bytes, &ws));
  CHECK(vali_mem_alloc(dev, out_bytes, &d_out));
  CHECK(vali_mem_alloc(dev, (size_t)n * sizeof(uint32_t), &d_sizes));
  vali_surface* srcs = (vali_surface*)malloc((size_t)n * sizeof(vali_surface));
  memset(srcs, 0, (size_t)n * sizeof(vali_surface));
  for (int i = 0; i < n; ++i) { /* every item reads the one surface */
    srcs[i].plane[0] = d_rgb;
    srcs[i].pitch[0] = (int)pitch;
    srcs[i].width = w;
    srcs[i].height = h;
    srcs[i].format = VALI_FMT_RGB;
  }
  CHECK(vali_memcpy2d_async(dev, d_rgb, pitch, pixels, row, row, (size_t)h, 0, stream));
  CHECK(vali_memcpy2d_async(dev, d_src, (size_t)n * sizeof(vali_surface), srcs, (size_t)n * sizeof(vali_surface),
                            (size_t)n * sizeof(vali_surface), 1, 0, stream));
  CHECK(vali_memcpy2d_async(dev, d_items, (size_t)n * sizeof(vali_jpeg_item), items, (size_t)n * sizeof(vali_jpeg_item),
                            (size_t)n * sizeof(vali_jpeg_item), 1, 0, stream));
  CHECK(vali_jpeg_encode_rois((const vali_surface*)d_src, items, (const vali_jpeg_item*)d_items, n, &params, ws,
                              ws_bytes, (uint8_t*)d_out, out_bytes, (uint32_t*)d_sizes, stream));
  uint32_t sizes[MAX_ROIS];
  CHECK(vali_memcpy2d_async(dev, sizes, (size_t)n * 4, d_sizes, (size_t)n * 4, (size_t)n * 4, 1, 1, stream));
  CHECK(vali_stream_sync(dev, stream));

  for (int i = 0; i < n; ++i) {
    unsigned char header[1024];
    size_t hlen = 0, cap = 0;
    CHECK(vali_jpeg_header(items[i].width, items[i].height, &params, header, sizeof header, &hlen));
    CHECK(vali_jpeg_stream_capacity(items[i].width, items[i].height, &params, &cap));
    if (sizes[i] > cap) {
      fprintf(stderr, "image %d: %u bytes in a slot of %zu\n", i, (unsigned)sizes[i], cap);
      return 1;
    }
    unsigned char* body = (unsigned char*)malloc(sizes[i]);
    CHECK(vali_memcpy2d_async(dev, body, sizes[i], (const uint8_t*)d_out + items[i].out_offset, sizes[i], sizes[i], 1,
                              1, stream));
    CHECK(vali_stream_sync(dev, stream));
    char name[1024];
    snprintf(name, sizeof name, "%s%d.jpg", argv[8], i);
    static const unsigned char eoi[2] = {0xFF, 0xD9};
    f = fopen(name, "wb");
    if (!f || fwrite(header, 1, hlen, f) != hlen || fwrite(body, 1, sizes[i], f) != sizes[i] ||
        fwrite(eoi, 1, 2, f) != 2)
      return 2;
    fclose(f);
    free(body);
  }
  void* bufs[6] = {d_rgb, d_src, d_items, ws, d_out, d_sizes};
  for (int i = 0; i < 6; ++i)
    CHECK(vali_mem_free(dev, bufs[i]));
  CHECK(vali_stream_destroy(dev, stream));
  printf("ok %d\n", n);
  free(srcs);
  free(items);
  free(pixels);
  return 0;
}
