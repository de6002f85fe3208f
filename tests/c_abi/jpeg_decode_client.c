/* A plain C99 client of the JPEG decoder of include/vali_hip.h: parse a file on the host, upload its info and its
 * entropy-coded data, decode it into a pitched RGB surface, download the pixels, write them out.
 *   usage: jpeg_decode_client <in.jpg> <out.rgb>
 * Prints "ok <width> <height>" and exits 0 on success; prints vali_last_error() otherwise.
 * tests/test_gpu_c_abi_jpeg_decode.py compares the output with Pillow. */
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

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s in.jpg out.rgb\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f)
    return 2;
  fseek(f, 0, SEEK_END);
  const long len = ftell(f);
  fseek(f, 0, SEEK_SET);
  unsigned char* file = (unsigned char*)malloc((size_t)len);
  if (fread(file, 1, (size_t)len, f) != (size_t)len)
    return 2;
  fclose(f);

  const int dev = 0;
  vali_jpeg_info* info = (vali_jpeg_info*)malloc(sizeof(vali_jpeg_info));
  CHECK(vali_jpeg_parse(file, (size_t)len, info));
  const int w = info->width, h = info->height;
  const size_t data_len = (size_t)info->data_len;
  const unsigned char* body = file + info->data_offset;
  info->data_offset = 0; /* the entropy data sits at the start of the device buffer */
  size_t ws_bytes = 0;
  CHECK(vali_jpeg_decode_workspace_size(info, 1, &ws_bytes));

  vali_stream_t stream = NULL;
  CHECK(vali_stream_create(dev, &stream));
  void *d_info = NULL, *d_data = NULL, *d_dst = NULL, *d_status = NULL, *ws = NULL, *d_rgb = NULL;
  size_t pitch = 0;
  CHECK(vali_mem_alloc(dev, sizeof(vali_jpeg_info), &d_info));
  CHECK(vali_mem_alloc(dev, data_len + 16, &d_data));
  CHECK(vali_mem_alloc(dev, sizeof(vali_surface), &d_dst));
  CHECK(vali_mem_alloc(dev, sizeof(int32_t), &d_status));
  CHECK(vali_mem_alloc(dev, ws_bytes, &ws));
  CHECK(vali_mem_alloc_pitch(dev, (size_t)w * 3, (size_t)h, &d_rgb, &pitch));
  vali_surface dst;
  memset(&dst, 0, sizeof dst);
  dst.plane[0] = d_rgb;
  dst.pitch[0] = (int)pitch;
  dst.width = w;
  dst.height = h;
  dst.format = VALI_FMT_RGB;
  CHECK(vali_memcpy2d_async(dev, d_info, sizeof(vali_jpeg_info), info, sizeof(vali_jpeg_info),
                            sizeof(vali_jpeg_info), 1, 0, stream));
  CHECK(vali_memcpy2d_async(dev, d_data, data_len, body, data_len, data_len, 1, 0, stream));
  CHECK(vali_memcpy2d_async(dev, d_dst, sizeof dst, &dst, sizeof dst, sizeof dst, 1, 0, stream));
  CHECK(vali_jpeg_decode_batch(info, (const vali_jpeg_info*)d_info, 1, (const uint8_t*)d_data, VALI_FMT_RGB,
                               (const vali_surface*)d_dst, ws, ws_bytes, (int32_t*)d_status, stream));
  unsigned char* out = (unsigned char*)malloc((size_t)w * h * 3);
  int32_t status = -1;
  CHECK(vali_memcpy2d_async(dev, out, (size_t)w * 3, d_rgb, pitch, (size_t)w * 3, (size_t)h, 1, stream));
  CHECK(vali_memcpy2d_async(dev, &status, 4, d_status, 4, 4, 1, 1, stream));
  CHECK(vali_stream_sync(dev, stream));
  if (status != 0) {
    fprintf(stderr, "decode status %d\n", (int)status);
    return 1;
  }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out, 1, (size_t)w * h * 3, f) != (size_t)w * h * 3)
    return 2;
  fclose(f);
  void* bufs[6] = {d_info, d_data, d_dst, d_status, ws, d_rgb};
  for (int i = 0; i < 6; ++i)
    CHECK(vali_mem_free(dev, bufs[i]));
  CHECK(vali_stream_destroy(dev, stream));
  printf("ok %d %d\n", w, h);
  free(out);
  free(info);
  free(file);
  return 0;
}
