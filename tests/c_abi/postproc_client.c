/* A plain C99 client of vali_tensor_to_surfaces (include/vali_hip.h).
 * One uint8 planar tensor (n, 3, h, w) from a file, scale 1, offset 0, channels R, G, B, with the matrix
 *   Y = (0, 1, 0, 0)   U = (0, 0, 1, 0.5)   V = (1, 0, 0, 0.25)
 * so Y is G, every 2 x 2 mean of U lands on k / 4 + 0.5 (ties among them) and of V on k / 4 + 0.25: chroma rounding made
 * visible.  Written as YUV420 planes (out.yuv420: per item Y, U, V back to back) and as NV12 (out.nv12).
 *   usage: postproc_client <tensor.u8> <n> <w> <h> <out.yuv420> <out.nv12>
 * tests/test_gpu_c_abi_postproc.py compares both with the CPU oracle. */
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

#define MAX_N 8

int main(int argc, char** argv) {
  if (argc != 7) {
    fprintf(stderr, "usage: %s tensor.u8 n w h out.yuv420 out.nv12\n", argv[0]);
    return 2;
  }
  const int n = atoi(argv[2]), w = atoi(argv[3]), h = atoi(argv[4]), dev = 0;
  if (n < 1 || n > MAX_N || w < 2 || h < 2) return 2;
  const size_t tbytes = (size_t)n * 3 * w * h, ibytes = (size_t)w * h * 3 / 2;
  unsigned char* host = (unsigned char*)malloc(tbytes);
  FILE* f = fopen(argv[1], "rb");
  if (!host || !f || fread(host, 1, tbytes, f) != tbytes) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  fclose(f);
  int count = 0;
  CHECK(vali_device_count(&count));
  if (count < 1) {
    fprintf(stderr, "no device\n");
    return 3;
  }
  vali_stream_t stream = NULL;
  CHECK(vali_stream_create(dev, &stream));
  void* d_tensor = NULL;
  CHECK(vali_mem_alloc(dev, tbytes, &d_tensor));
  CHECK(vali_memcpy2d_async(dev, d_tensor, tbytes, host, tbytes, tbytes, 1, 0, stream));

  /* per item: one pitched allocation of h + h / 2 + h / 2 rows for Y, U, V, and one of h * 3 / 2 rows for NV12 */
  void *m420[MAX_N], *mnv[MAX_N];
  size_t p420 = 0, pnv = 0;
  vali_surface s420[MAX_N], snv[MAX_N];
  for (int i = 0; i < n; ++i) {
    CHECK(vali_mem_alloc_pitch(dev, (size_t)w, (size_t)h * 2, &m420[i], &p420));
    CHECK(vali_mem_alloc_pitch(dev, (size_t)w, (size_t)h * 3 / 2, &mnv[i], &pnv));
    memset(&s420[i], 0, sizeof s420[i]);
    s420[i].plane[0] = m420[i];
    s420[i].plane[1] = (char*)m420[i] + (size_t)h * p420;
    s420[i].plane[2] = (char*)m420[i] + (size_t)(h + h / 2) * p420;
    s420[i].pitch[0] = s420[i].pitch[1] = s420[i].pitch[2] = (int32_t)p420;
    s420[i].width = w; s420[i].height = h; s420[i].format = VALI_FMT_YUV420;
    memset(&snv[i], 0, sizeof snv[i]);
    snv[i].plane[0] = mnv[i];
    snv[i].plane[1] = (char*)mnv[i] + (size_t)h * pnv;
    snv[i].pitch[0] = snv[i].pitch[1] = (int32_t)pnv;
    snv[i].width = w; snv[i].height = h; snv[i].format = VALI_FMT_NV12;
  }
  void *d_420 = NULL, *d_nv = NULL;
  const size_t dbytes = (size_t)n * sizeof(vali_surface);
  CHECK(vali_mem_alloc(dev, dbytes, &d_420));
  CHECK(vali_mem_alloc(dev, dbytes, &d_nv));
  CHECK(vali_memcpy2d_async(dev, d_420, dbytes, s420, dbytes, dbytes, 1, 0, stream));
  CHECK(vali_memcpy2d_async(dev, d_nv, dbytes, snv, dbytes, dbytes, 1, 0, stream));

  vali_tensor_src src;
  memset(&src, 0, sizeof src);
  src.data = d_tensor; src.dtype = VALI_DTYPE_U8; src.packed = 0;
  src.n = n; src.width = w; src.height = h;
  src.stride_n = (int64_t)3 * w * h; src.stride_c = (int64_t)w * h; src.stride_y = w;
  const float scale[3] = {1.0f, 1.0f, 1.0f}, offset[3] = {0.0f, 0.0f, 0.0f};
  vali_cvt_params prm;
  memset(&prm, 0, sizeof prm);
  prm.rgb2yuv[0][1] = 1.0f;
  prm.rgb2yuv[1][2] = 1.0f; prm.rgb2yuv[1][3] = 0.5f;
  prm.rgb2yuv[2][0] = 1.0f; prm.rgb2yuv[2][3] = 0.25f;
  CHECK(vali_tensor_to_surfaces(&src, scale, offset, 0, (const vali_surface*)d_420, VALI_FMT_YUV420, &prm, stream));
  CHECK(vali_tensor_to_surfaces(&src, scale, offset, 0, (const vali_surface*)d_nv, VALI_FMT_NV12, &prm, stream));

  unsigned char* o420 = (unsigned char*)malloc(ibytes * n);
  unsigned char* onv = (unsigned char*)malloc(ibytes * n);
  if (!o420 || !onv) return 2;
  for (int i = 0; i < n; ++i) {
    unsigned char* o = o420 + ibytes * i;
    CHECK(vali_memcpy2d_async(dev, o, (size_t)w, s420[i].plane[0], p420, (size_t)w, (size_t)h, 1, stream));
    CHECK(vali_memcpy2d_async(dev, o + (size_t)w * h, (size_t)w / 2, s420[i].plane[1], p420, (size_t)w / 2, (size_t)h / 2,
                              1, stream));
    CHECK(vali_memcpy2d_async(dev, o + (size_t)w * h * 5 / 4, (size_t)w / 2, s420[i].plane[2], p420, (size_t)w / 2,
                              (size_t)h / 2, 1, stream));
    CHECK(vali_memcpy2d_async(dev, onv + ibytes * i, (size_t)w, mnv[i], pnv, (size_t)w, (size_t)h * 3 / 2, 1, stream));
  }
  CHECK(vali_stream_sync(dev, stream));
  FILE* a = fopen(argv[5], "wb");
  FILE* b = fopen(argv[6], "wb");
  if (!a || !b || fwrite(o420, 1, ibytes * n, a) != ibytes * n || fwrite(onv, 1, ibytes * n, b) != ibytes * n) return 2;
  fclose(a);
  fclose(b);

  /* refusals are decided on the host: an odd size for a 4:2:0 destination, a destination format outside the list */
  src.width = w - 1;
  if (vali_tensor_to_surfaces(&src, scale, offset, 0, (const vali_surface*)d_nv, VALI_FMT_NV12, &prm, stream) !=
      VALI_ERR_INVALID_ARG)
    return 4;
  src.width = w;
  if (vali_tensor_to_surfaces(&src, scale, offset, 0, (const vali_surface*)d_nv, VALI_FMT_BGR, &prm, stream) !=
      VALI_ERR_UNSUPPORTED)
    return 4;

  for (int i = 0; i < n; ++i) {
    vali_mem_free(dev, m420[i]);
    vali_mem_free(dev, mnv[i]);
  }
  vali_mem_free(dev, d_tensor); vali_mem_free(dev, d_420); vali_mem_free(dev, d_nv);
  vali_stream_destroy(dev, stream);
  free(host); free(o420); free(onv);
  printf("ok %s\n", vali_version());
  return 0;
}
