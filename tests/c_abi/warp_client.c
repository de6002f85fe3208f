/* A plain C99 client of vali_warp_fit / vali_warp_tensor (include/vali_hip.h).
 * One tightly packed NV12 frame of w x h comes from a file, with float32 keypoints (1, k, p, 3), d detection rows of 8
 * int32, the frame's record of 8 int32, a template of p float32 pairs and the 64 bytes of a vali_preproc_params.  One call
 * fits the d matrices, one samples them into a float32 planar (d, 3, ch, cw) tensor; the matrices and the tensor are read
 * back, written to got_rows.bin and got.bin and compared with want_rows.bin and want.bin, which
 * tests/test_gpu_c_abi_warp.py wrote with tests/warp_model.py.
 *   usage: warp_client <w> <h> <k> <p> <d> <cw> <ch> <thr> <min_points> <frame.bin> <kpts.bin> <dets.bin> <rect.bin>
 *                      <template.bin> <params.bin> <want_rows.bin> <want.bin> <got_rows.bin> <got.bin>
 * exit status 0: equal; 5: the tensors differ (got.bin holds the sampled one); 6: the matrices differ; 4: a refusal did
 * not come. */
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

static int write_file(const char* path, const void* data, size_t bytes) {
  FILE* o = fopen(path, "wb");
  if (!o || fwrite(data, 1, bytes, o) != bytes) return 1;
  fclose(o);
  return 0;
}

static int upload(int dev, void** d, const void* host, size_t bytes, vali_stream_t stream) {
  CHECK(vali_mem_alloc(dev, bytes, d));
  CHECK(vali_memcpy2d_async(dev, *d, bytes, host, bytes, bytes, 1, 0, stream));
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 20) {
    fprintf(stderr, "usage: %s w h k p d cw ch thr min_points frame kpts dets rect template params want_rows want "
                    "got_rows got\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[1]), h = atoi(argv[2]), k = atoi(argv[3]), p = atoi(argv[4]), d = atoi(argv[5]);
  const int cw = atoi(argv[6]), ch = atoi(argv[7]), min_points = atoi(argv[9]);
  const float thr = (float)atof(argv[8]);
  const int dev = 0;
  if (w < 2 || h < 2 || k < 1 || p < 2 || d < 1 || cw < 1 || ch < 1) return 2;
  if (sizeof(vali_preproc_params) != 64 || sizeof(vali_warp_fit_in) != 80) return 2;
  const size_t fbytes = (size_t)w * h * 3 / 2, kbytes = (size_t)k * p * 3 * sizeof(float);
  const size_t dbytes = (size_t)d * 8 * sizeof(int32_t), tbytes = (size_t)p * 2 * sizeof(float);
  const size_t obytes = (size_t)d * 3 * ch * cw * sizeof(float);
  unsigned char* frame = read_file(argv[10], fbytes);
  unsigned char* kpts = read_file(argv[11], kbytes);
  unsigned char* dets = read_file(argv[12], dbytes);
  unsigned char* rect = read_file(argv[13], sizeof(vali_roi));
  unsigned char* tmpl = read_file(argv[14], tbytes);
  unsigned char* prm = read_file(argv[15], sizeof(vali_preproc_params));
  unsigned char* want_rows = read_file(argv[16], dbytes);
  unsigned char* want = read_file(argv[17], obytes);
  unsigned char* got_rows = (unsigned char*)malloc(dbytes);
  unsigned char* got = (unsigned char*)malloc(obytes);
  if (!frame || !kpts || !dets || !rect || !tmpl || !prm || !want_rows || !want || !got_rows || !got) return 2;
  vali_preproc_params params;
  memcpy(&params, prm, sizeof params);

  int count = 0;
  CHECK(vali_device_count(&count));
  if (count < 1) {
    fprintf(stderr, "no device\n");
    return 3;
  }
  vali_stream_t stream = NULL;
  CHECK(vali_stream_create(dev, &stream));

  void *d_frame = NULL, *d_kpts = NULL, *d_dets = NULL, *d_rect = NULL, *d_tmpl = NULL, *d_desc = NULL, *d_rows = NULL;
  void* d_out = NULL;
  if (upload(dev, &d_frame, frame, fbytes, stream) || upload(dev, &d_kpts, kpts, kbytes, stream) ||
      upload(dev, &d_dets, dets, dbytes, stream) || upload(dev, &d_rect, rect, sizeof(vali_roi), stream) ||
      upload(dev, &d_tmpl, tmpl, tbytes, stream))
    return 1;
  vali_surface desc;
  memset(&desc, 0, sizeof desc);
  desc.plane[0] = d_frame;
  desc.plane[1] = (unsigned char*)d_frame + (size_t)w * h;
  desc.pitch[0] = desc.pitch[1] = w;
  desc.width = w; desc.height = h; desc.format = VALI_FMT_NV12;
  if (upload(dev, &d_desc, &desc, sizeof desc, stream)) return 1;
  CHECK(vali_mem_alloc(dev, dbytes, &d_rows));
  /* the pad colour fills what the test's canary would: every element is written */
  CHECK(vali_mem_alloc(dev, obytes, &d_out));

  vali_warp_fit_in in;
  memset(&in, 0, sizeof in);
  in.kpts = d_kpts; in.dtype = VALI_DTYPE_F32; in.kdim = 3;
  in.stride_n = (int64_t)k * p * 3; in.stride_k = (int64_t)p * 3; in.stride_p = 3; in.stride_c = 1;
  in.k = k; in.p = p; in.max_det = d; in.min_points = min_points;
  in.d_template = (const float*)d_tmpl;
  in.kpt_thr = thr;
  vali_tensor_dst dst;
  memset(&dst, 0, sizeof dst);
  dst.data = d_out; dst.dtype = VALI_DTYPE_F32; dst.packed = 0;
  dst.n = d; dst.width = cw; dst.height = ch;
  dst.stride_n = (int64_t)3 * ch * cw; dst.stride_c = (int64_t)ch * cw; dst.stride_y = cw;
  const uint8_t pad_rgb[3] = {30, 60, 90};

#define FIT(DFRAMES, N, IN, DETS, RECTS, ROWS)                                                                        \
  vali_warp_fit((const vali_surface*)(DFRAMES), N, IN, (const int32_t*)(DETS), (const vali_roi*)(RECTS), (int32_t*)(ROWS), stream)
#define SAMPLE(FRAMES, DFRAMES, N, FMT, ROWS, DST, PRM, PAD, RGB)                                                     \
  vali_warp_tensor(FRAMES, (const vali_surface*)(DFRAMES), N, FMT, (const int32_t*)(ROWS), DST, PRM, PAD, RGB, stream)
  /* refusals are decided on the host, before anything is launched */
  vali_warp_fit_in bad = in;
  bad.p = 65;
  if (FIT(d_desc, 1, &bad, d_dets, d_rect, d_rows) != VALI_ERR_INVALID_ARG) return 4;
  bad = in;
  bad.min_points = 1;
  if (FIT(d_desc, 1, &bad, d_dets, d_rect, d_rows) != VALI_ERR_INVALID_ARG) return 4;
  bad = in;
  bad.min_points = p + 1;
  if (FIT(d_desc, 1, &bad, d_dets, d_rect, d_rows) != VALI_ERR_INVALID_ARG) return 4;
  bad = in;
  bad.kdim = 4;
  if (FIT(d_desc, 1, &bad, d_dets, d_rect, d_rows) != VALI_ERR_INVALID_ARG) return 4;
  bad = in;
  bad.dtype = 3;
  if (FIT(d_desc, 1, &bad, d_dets, d_rect, d_rows) != VALI_ERR_INVALID_ARG) return 4;
  bad = in;
  bad.stride_p = -1;
  if (FIT(d_desc, 1, &bad, d_dets, d_rect, d_rows) != VALI_ERR_INVALID_ARG) return 4;
  bad = in;
  bad.d_template = NULL;
  if (FIT(d_desc, 1, &bad, d_dets, d_rect, d_rows) != VALI_ERR_INVALID_ARG) return 4;
  if (FIT(NULL, 1, &in, d_dets, d_rect, d_rows) != VALI_ERR_INVALID_ARG) return 4;
  if (FIT(d_desc, 0, &in, d_dets, d_rect, d_rows) != VALI_ERR_INVALID_ARG) return 4;
  if (FIT(d_desc, 1, &in, NULL, d_rect, d_rows) != VALI_ERR_INVALID_ARG) return 4;
  if (FIT(d_desc, 1, &in, d_dets, NULL, d_rows) != VALI_ERR_INVALID_ARG) return 4;
  if (FIT(d_desc, 1, &in, d_dets, d_rect, NULL) != VALI_ERR_INVALID_ARG) return 4;
  if (FIT(d_desc, 1, &in, d_dets, d_rect, (char*)d_rows + 8) != VALI_ERR_INVALID_ARG) return 4;
  vali_tensor_dst bdst = dst;
  bdst.dtype = 3;
  if (SAMPLE(&desc, d_desc, 1, VALI_FMT_NV12, d_rows, &bdst, &params, 1, pad_rgb) != VALI_ERR_INVALID_ARG) return 4;
  bdst = dst;
  bdst.stride_y = cw - 1;
  if (SAMPLE(&desc, d_desc, 1, VALI_FMT_NV12, d_rows, &bdst, &params, 1, pad_rgb) != VALI_ERR_INVALID_ARG) return 4;
  bdst = dst;
  bdst.n = 0;
  if (SAMPLE(&desc, d_desc, 1, VALI_FMT_NV12, d_rows, &bdst, &params, 1, pad_rgb) != VALI_ERR_INVALID_ARG) return 4;
  if (SAMPLE(NULL, d_desc, 1, VALI_FMT_NV12, d_rows, &dst, &params, 1, pad_rgb) != VALI_ERR_INVALID_ARG) return 4;
  if (SAMPLE(&desc, NULL, 1, VALI_FMT_NV12, d_rows, &dst, &params, 1, pad_rgb) != VALI_ERR_INVALID_ARG) return 4;
  if (SAMPLE(&desc, d_desc, 1, VALI_FMT_NV12, NULL, &dst, &params, 1, pad_rgb) != VALI_ERR_INVALID_ARG) return 4;
  if (SAMPLE(&desc, d_desc, 1, VALI_FMT_NV12, d_rows, NULL, &params, 1, pad_rgb) != VALI_ERR_INVALID_ARG) return 4;
  if (SAMPLE(&desc, d_desc, 1, VALI_FMT_NV12, d_rows, &dst, NULL, 1, pad_rgb) != VALI_ERR_INVALID_ARG) return 4;
  if (SAMPLE(&desc, d_desc, 1, VALI_FMT_NV12, d_rows, &dst, &params, 1, NULL) != VALI_ERR_INVALID_ARG) return 4;
  if (SAMPLE(&desc, d_desc, 0, VALI_FMT_NV12, d_rows, &dst, &params, 1, pad_rgb) != VALI_ERR_INVALID_ARG) return 4;
  if (SAMPLE(&desc, d_desc, 1, VALI_FMT_RGB, d_rows, &dst, &params, 1, pad_rgb) != VALI_ERR_INVALID_ARG) return 4;
  if (SAMPLE(&desc, d_desc, 1, VALI_FMT_YUV420, d_rows, &dst, &params, 1, pad_rgb) != VALI_ERR_UNSUPPORTED) return 4;
  if (SAMPLE(&desc, d_desc, 1, VALI_FMT_Y, d_rows, &dst, &params, 1, pad_rgb) != VALI_ERR_UNSUPPORTED) return 4;

  CHECK(FIT(d_desc, 1, &in, d_dets, d_rect, d_rows));
  CHECK(SAMPLE(&desc, d_desc, 1, VALI_FMT_NV12, d_rows, &dst, &params, 1, pad_rgb));
  CHECK(vali_memcpy2d_async(dev, got_rows, dbytes, d_rows, dbytes, dbytes, 1, 1, stream));
  CHECK(vali_memcpy2d_async(dev, got, obytes, d_out, obytes, obytes, 1, 1, stream));
  CHECK(vali_stream_sync(dev, stream));
  if (write_file(argv[18], got_rows, dbytes) || write_file(argv[19], got, obytes)) return 2;
  const int equal = memcmp(got, want, obytes) == 0;
  const int rows_equal = memcmp(got_rows, want_rows, dbytes) == 0;

  vali_mem_free(dev, d_frame); vali_mem_free(dev, d_kpts); vali_mem_free(dev, d_dets); vali_mem_free(dev, d_rect);
  vali_mem_free(dev, d_tmpl); vali_mem_free(dev, d_desc); vali_mem_free(dev, d_rows); vali_mem_free(dev, d_out);
  vali_stream_destroy(dev, stream);
  free(frame); free(kpts); free(dets); free(rect); free(tmpl); free(prm); free(want_rows); free(want); free(got_rows);
  free(got);
  if (!rows_equal) {
    fprintf(stderr, "the matrices differ from want_rows.bin\n");
    return 6;
  }
  if (!equal) {
    fprintf(stderr, "the tensor differs from want.bin\n");
    return 5;
  }
  printf("ok %s\n", vali_version());
  return 0;
}
