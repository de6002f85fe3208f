/* A plain C99 client of the region entry points of include/vali_hip.h.
 * Two NV12 frames of different sizes; three rectangle records and the descriptor arrays are uploaded, then
 *   vali_nv12_preproc_roi_batch: pad on, RGB_32F_PLANAR canvases (out_batch.f32, 3 items, planes back to back)
 *   vali_nv12_preproc_roi:       pad off, one BGR canvas filled with 0x5A first (out_single.bgr)
 *   usage: roi_client <a.nv12> <wa> <ha> <b.nv12> <wb> <hb> <cw> <ch> <out_batch.f32> <out_single.bgr>
 * The rectangles are fixed here and restated in tests/test_gpu_c_abi_roi.py, which compares with the oracle. */
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
  unsigned char* p = (unsigned char*)malloc(bytes);
  FILE* f = fopen(path, "rb");
  if (!p || !f || fread(p, 1, bytes, f) != bytes) {
    fprintf(stderr, "cannot read %s\n", path);
    exit(2);
  }
  fclose(f);
  return p;
}

static int write_file(const char* path, const void* p, size_t bytes) {
  FILE* f = fopen(path, "wb");
  if (!f || fwrite(p, 1, bytes, f) != bytes) return 2;
  fclose(f);
  return 0;
}

/* upload a tightly packed NV12 image into a pitched allocation; fill its descriptor */
static int nv12_surface(int dev, const unsigned char* host, int w, int h, vali_stream_t stream, void** mem,
                        vali_surface* s) {
  size_t pitch = 0;
  CHECK(vali_mem_alloc_pitch(dev, (size_t)w, (size_t)h * 3 / 2, mem, &pitch));
  CHECK(vali_memcpy2d_async(dev, *mem, pitch, host, (size_t)w, (size_t)w, (size_t)h * 3 / 2, 0, stream));
  memset(s, 0, sizeof *s);
  s->plane[0] = *mem; s->plane[1] = (char*)*mem + (size_t)h * pitch;
  s->pitch[0] = s->pitch[1] = (int32_t)pitch; s->width = w; s->height = h; s->format = VALI_FMT_NV12;
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 11) {
    fprintf(stderr, "usage: %s a.nv12 wa ha b.nv12 wb hb cw ch out_batch.f32 out_single.bgr\n", argv[0]);
    return 2;
  }
  const int wa = atoi(argv[2]), ha = atoi(argv[3]), wb = atoi(argv[5]), hb = atoi(argv[6]);
  const int cw = atoi(argv[7]), ch = atoi(argv[8]), dev = 0, n = 3;
  unsigned char* a = read_file(argv[1], (size_t)wa * ha * 3 / 2);
  unsigned char* b = read_file(argv[4], (size_t)wb * hb * 3 / 2);
  int count = 0;
  CHECK(vali_device_count(&count));
  if (count < 1) {
    fprintf(stderr, "no device\n");
    return 3;
  }
  vali_stream_t stream = NULL;
  CHECK(vali_stream_create(dev, &stream));
  void *ma = NULL, *mb = NULL;
  vali_surface src[3], dst[3], bgr;
  if (nv12_surface(dev, a, wa, ha, stream, &ma, &src[0]) || nv12_surface(dev, b, wb, hb, stream, &mb, &src[1]))
    return 1;
  src[2] = src[0]; /* a source may repeat */

  /* three RGB_32F_PLANAR canvases: plane c of item i at base + (3 i + c) * ch * pitch */
  void* mf = NULL;
  size_t fp = 0;
  CHECK(vali_mem_alloc_pitch(dev, (size_t)cw * 4, (size_t)ch * 3 * n, &mf, &fp));
  for (int i = 0; i < n; ++i) {
    memset(&dst[i], 0, sizeof dst[i]);
    for (int c = 0; c < 3; ++c) {
      dst[i].plane[c] = (char*)mf + (size_t)(3 * i + c) * ch * fp;
      dst[i].pitch[c] = (int32_t)fp;
    }
    dst[i].width = cw; dst[i].height = ch; dst[i].format = VALI_FMT_RGB_32F_PLANAR;
  }
  const vali_roi rois[3] = {
      {0, 0, wa, ha, 0, ch / 4, cw, ch / 2},        /* whole frame a, banded */
      {2, 2, wb - 4, hb / 2, 2, 0, cw - 4, ch},      /* upper half of frame b */
      {wa / 2, ha / 2, wa / 4, ha / 4, 6, 10, 96, 64} /* a box of frame a */
  };
  void *d_src = NULL, *d_dst = NULL, *d_roi = NULL;
  CHECK(vali_mem_alloc(dev, sizeof src, &d_src));
  CHECK(vali_mem_alloc(dev, sizeof dst, &d_dst));
  CHECK(vali_mem_alloc(dev, sizeof rois, &d_roi));
  CHECK(vali_memcpy2d_async(dev, d_src, sizeof src, src, sizeof src, sizeof src, 1, 0, stream));
  CHECK(vali_memcpy2d_async(dev, d_dst, sizeof dst, dst, sizeof dst, sizeof dst, 1, 0, stream));
  CHECK(vali_memcpy2d_async(dev, d_roi, sizeof rois, rois, sizeof rois, sizeof rois, 1, 0, stream));

  vali_preproc_params prm;
  memset(&prm, 0, sizeof prm);
  /* nppiNV12ToRGB_709CSC_8u_P2C3R coefficients; ImageNet normalisation of the 0..1 range */
  prm.csc.y0 = 16.0f; prm.csc.cy = 1.164f; prm.csc.crv = 1.793f; prm.csc.cgu = -0.213f; prm.csc.cgv = -0.533f;
  prm.csc.cbu = 2.112f;
  prm.div = 1.0f;
  prm.mean[0] = 0.485f; prm.mean[1] = 0.456f; prm.mean[2] = 0.406f;
  prm.std_[0] = 0.229f; prm.std_[1] = 0.224f; prm.std_[2] = 0.225f;
  const uint8_t pad[3] = {114, 114, 114};
  CHECK(vali_nv12_preproc_roi_batch((const vali_surface*)d_src, (const vali_surface*)d_dst, (const vali_roi*)d_roi,
                                    n, cw, ch, VALI_FMT_RGB_32F_PLANAR, &prm, 1, pad, stream));

  /* one BGR canvas, padding off: everything outside the placement keeps 0x5A */
  void* mc = NULL;
  size_t cp = 0;
  CHECK(vali_mem_alloc_pitch(dev, (size_t)cw * 3, (size_t)ch, &mc, &cp));
  CHECK(vali_memset2d_async(dev, mc, cp, 0x5A, (size_t)cw * 3, (size_t)ch, stream));
  memset(&bgr, 0, sizeof bgr);
  bgr.plane[0] = mc; bgr.pitch[0] = (int32_t)cp; bgr.width = cw; bgr.height = ch; bgr.format = VALI_FMT_BGR;
  const vali_roi one = {wb / 4, hb / 4, wb / 2, hb / 2, 2, 4, cw / 2, ch / 2};
  CHECK(vali_nv12_preproc_roi(&src[1], &bgr, &one, &prm, 0, NULL, stream));

  const size_t fbytes = (size_t)cw * 4 * ch * 3 * n, cbytes = (size_t)cw * 3 * ch;
  unsigned char* of = (unsigned char*)malloc(fbytes);
  unsigned char* oc = (unsigned char*)malloc(cbytes);
  CHECK(vali_memcpy2d_async(dev, of, (size_t)cw * 4, mf, fp, (size_t)cw * 4, (size_t)ch * 3 * n, 1, stream));
  CHECK(vali_memcpy2d_async(dev, oc, (size_t)cw * 3, mc, cp, (size_t)cw * 3, (size_t)ch, 1, stream));
  CHECK(vali_stream_sync(dev, stream));
  if (write_file(argv[9], of, fbytes) || write_file(argv[10], oc, cbytes)) return 2;

  /* strict host validation of the single form: an odd crop is refused, not launched */
  const vali_roi odd = {1, 0, 4, 4, 0, 0, 4, 4};
  if (vali_nv12_preproc_roi(&src[0], &bgr, &odd, &prm, 0, NULL, stream) != VALI_ERR_INVALID_ARG) return 4;

  vali_mem_free(dev, ma); vali_mem_free(dev, mb); vali_mem_free(dev, mf); vali_mem_free(dev, mc);
  vali_mem_free(dev, d_src); vali_mem_free(dev, d_dst); vali_mem_free(dev, d_roi);
  vali_stream_destroy(dev, stream);
  free(a); free(b); free(of); free(oc);
  printf("ok %s\n", vali_version());
  return 0;
}
