/* A plain C99 client of vali_kpt_decode and vali_pose_paint_points (include/vali_hip.h).
 * One tightly packed RGB frame of w x h comes from a file, with float32 heatmaps (m, p, hh, wh), m matrix rows of 8 int32
 * that all name frame 0, l limb pairs, three limb colours and two joint colours.  One call decodes the heatmaps into
 * points and kpts, a second draws the points onto the frame (max_det = m); frame, points and kpts are read back, written
 * to got.bin, points.bin and kpts.bin and compared with want.bin, want_points.bin and want_kpts.bin, which
 * tests/test_gpu_c_abi_kpt_decode.py wrote with tests/kpt_decode_model.py.
 *   usage: kpt_decode_client <w> <h> <m> <p> <hh> <wh> <cw> <ch> <thr> <l> <thickness> <diameter> <alpha> <frame.bin>
 *                            <heat.bin> <matrices.bin> <limbs.bin> <limb_colours.bin> <joint_colours.bin> <want.bin>
 *                            <want_points.bin> <want_kpts.bin> <got.bin> <points.bin> <kpts.bin>
 * exit status 0: equal; 5: the frames differ; 6: the points differ; 7: the kpts differ; 4: a refusal did not come. */
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
  if (argc != 26) {
    fprintf(stderr, "usage: %s w h m p hh wh cw ch thr l thickness diameter alpha frame heat matrices limbs limb_colours "
                    "joint_colours want want_points want_kpts got points kpts\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[1]), h = atoi(argv[2]), m = atoi(argv[3]), p = atoi(argv[4]), hh = atoi(argv[5]);
  const int wh = atoi(argv[6]), cw = atoi(argv[7]), ch = atoi(argv[8]), l = atoi(argv[10]);
  const int thickness = atoi(argv[11]), diameter = atoi(argv[12]), alpha = atoi(argv[13]);
  const float thr = (float)atof(argv[9]);
  const int dev = 0;
  if (w < 1 || h < 1 || m < 1 || p < 1 || hh < 1 || wh < 1 || l < 1) return 2;
  const size_t fbytes = (size_t)w * h * 3, hbytes = (size_t)m * p * hh * wh * sizeof(float);
  const size_t mbytes = (size_t)m * 8 * sizeof(int32_t), lbytes = (size_t)l * 2 * sizeof(int32_t);
  const size_t pbytes = (size_t)m * p * 4 * sizeof(int32_t), kbytes = (size_t)m * p * 3 * sizeof(float);
  unsigned char* frame = read_file(argv[14], fbytes);
  unsigned char* heat = read_file(argv[15], hbytes);
  unsigned char* mats = read_file(argv[16], mbytes);
  unsigned char* limbs = read_file(argv[17], lbytes);
  unsigned char* lcol = read_file(argv[18], 3 * sizeof(int32_t));
  unsigned char* jcol = read_file(argv[19], 2 * sizeof(int32_t));
  unsigned char* want = read_file(argv[20], fbytes);
  unsigned char* want_points = read_file(argv[21], pbytes);
  unsigned char* want_kpts = read_file(argv[22], kbytes);
  unsigned char* got = (unsigned char*)malloc(fbytes);
  unsigned char* points = (unsigned char*)malloc(pbytes);
  unsigned char* kpts = (unsigned char*)malloc(kbytes);
  if (!frame || !heat || !mats || !limbs || !lcol || !jcol || !want || !want_points || !want_kpts || !got || !points || !kpts)
    return 2;

  int count = 0;
  CHECK(vali_device_count(&count));
  if (count < 1) {
    fprintf(stderr, "no device\n");
    return 3;
  }
  vali_stream_t stream = NULL;
  CHECK(vali_stream_create(dev, &stream));

  void *d_frame = NULL, *d_heat = NULL, *d_mats = NULL, *d_limbs = NULL, *d_lcol = NULL, *d_jcol = NULL;
  void *d_desc = NULL, *d_points = NULL, *d_kpts = NULL, *ws = NULL;
  if (upload(dev, &d_frame, frame, fbytes, stream) || upload(dev, &d_heat, heat, hbytes, stream) ||
      upload(dev, &d_mats, mats, mbytes, stream) || upload(dev, &d_limbs, limbs, lbytes, stream) ||
      upload(dev, &d_lcol, lcol, 3 * sizeof(int32_t), stream) || upload(dev, &d_jcol, jcol, 2 * sizeof(int32_t), stream))
    return 1;
  vali_surface desc;
  memset(&desc, 0, sizeof desc);
  desc.plane[0] = d_frame;
  desc.pitch[0] = 3 * w;
  desc.width = w; desc.height = h; desc.format = VALI_FMT_RGB;
  if (upload(dev, &d_desc, &desc, sizeof desc, stream)) return 1;
  CHECK(vali_mem_alloc(dev, pbytes, &d_points));
  CHECK(vali_mem_alloc(dev, kbytes, &d_kpts));
  const size_t ws_bytes = vali_pose_workspace_size(1, m, p);
  CHECK(vali_mem_alloc(dev, ws_bytes, &ws));

  vali_kpt_decode_in in;
  memset(&in, 0, sizeof in);
  in.heat = d_heat; in.dtype = VALI_DTYPE_F32;
  in.refine = VALI_KPT_REFINE_QUARTER; in.align = VALI_KPT_ALIGN_CENTRE;
  in.stride_m = (int64_t)p * hh * wh; in.stride_p = (int64_t)hh * wh; in.stride_y = wh;
  in.m = m; in.p = p; in.hh = hh; in.wh = wh;
  in.canvas_w = cw; in.canvas_h = ch;
  in.kpt_thr = thr;
  in.max_det = m;

#define DECODE(DFRAMES, N, IN, MATS, ROIS, POINTS, KPTS)                                                              \
  vali_kpt_decode((const vali_surface*)(DFRAMES), N, IN, (const int32_t*)(MATS), (const vali_roi*)(ROIS),             \
                  (int32_t*)(POINTS), (float*)(KPTS), stream)
  /* refusals are decided on the host, before anything is launched */
  vali_kpt_decode_in bad = in;
  if (DECODE(NULL, 1, &in, d_mats, NULL, d_points, d_kpts) != VALI_ERR_INVALID_ARG) return 4;
  if (DECODE(d_desc, 1, NULL, d_mats, NULL, d_points, d_kpts) != VALI_ERR_INVALID_ARG) return 4;
  if (DECODE(d_desc, 1, &in, d_mats, NULL, NULL, d_kpts) != VALI_ERR_INVALID_ARG) return 4;
  if (DECODE(d_desc, 1, &in, NULL, NULL, d_points, d_kpts) != VALI_ERR_INVALID_ARG) return 4;
  if (DECODE(d_desc, 1, &in, d_mats, d_mats, d_points, d_kpts) != VALI_ERR_INVALID_ARG) return 4;
  if (DECODE(d_desc, 0, &in, d_mats, NULL, d_points, d_kpts) != VALI_ERR_INVALID_ARG) return 4;
  if (DECODE(d_desc, 1025, &in, d_mats, NULL, d_points, d_kpts) != VALI_ERR_INVALID_ARG) return 4;
  if (DECODE(d_desc, 1, &in, (char*)d_mats + 2, NULL, d_points, d_kpts) != VALI_ERR_INVALID_ARG) return 4;
  if (DECODE(d_desc, 1, &in, d_mats, NULL, (char*)d_points + 4, d_kpts) != VALI_ERR_INVALID_ARG) return 4;
  if (DECODE(d_desc, 1, &in, d_mats, NULL, d_points, (char*)d_kpts + 2) != VALI_ERR_INVALID_ARG) return 4;
#define REFUSED(FIELD, VALUE)                                                                                        \
  bad = in;                                                                                                          \
  bad.FIELD = VALUE;                                                                                                 \
  if (DECODE(d_desc, 1, &bad, d_mats, NULL, d_points, d_kpts) != VALI_ERR_INVALID_ARG) return 4;
  REFUSED(heat, NULL)
  REFUSED(simcc_x, d_heat)
  REFUSED(heat, (char*)d_heat + 2)
  REFUSED(dtype, 3)
  REFUSED(m, 0)
  REFUSED(m, 65536)
  REFUSED(p, 65)
  REFUSED(hh, 0)
  REFUSED(wh, 4097)
  REFUSED(canvas_w, 0)
  REFUSED(canvas_h, 65536)
  REFUSED(refine, 2)
  REFUSED(align, -1)
  REFUSED(stride_y, -1)
  REFUSED(stride_m, ((int64_t)1 << 40) + 1)
  volatile float zero = 0.0f;
  REFUSED(kpt_thr, zero / zero)
  bad = in;
  bad.hh = 1024; bad.wh = 1025;
  if (DECODE(d_desc, 1, &bad, d_mats, NULL, d_points, d_kpts) != VALI_ERR_INVALID_ARG) return 4;
  bad = in;                              /* SimCC vectors take no refinement */
  bad.heat = NULL; bad.simcc_x = d_heat; bad.simcc_y = d_heat;
  if (DECODE(d_desc, 1, &bad, d_mats, NULL, d_points, d_kpts) != VALI_ERR_INVALID_ARG) return 4;
  bad = in;                              /* rois: m is n * max_det */
  bad.max_det = m + 1;
  if (DECODE(d_desc, 1, &bad, NULL, d_mats, d_points, d_kpts) != VALI_ERR_INVALID_ARG) return 4;
  bad.max_det = 0;
  if (DECODE(d_desc, 1, &bad, NULL, d_mats, d_points, d_kpts) != VALI_ERR_INVALID_ARG) return 4;

  vali_pose_style st;
  memset(&st, 0, sizeof st);
  st.d_limb_colours = (const int32_t*)d_lcol; st.d_joint_colours = (const int32_t*)d_jcol;
  st.n_limb_colours = 3; st.n_joint_colours = 2;
  st.thickness = thickness; st.diameter = diameter; st.alpha = alpha;
#define PAINT(FRAMES, DFRAMES, N, FMT, POINTS, P, D, LIMBS, L, STYLE, WS, WSB)                                       \
  vali_pose_paint_points(FRAMES, (const vali_surface*)(DFRAMES), N, FMT, (const int32_t*)(POINTS), P, D,              \
                         (const int32_t*)(LIMBS), L, STYLE, NULL, WS, WSB, stream)
  vali_pose_style bst = st;
  if (PAINT(NULL, d_desc, 1, VALI_FMT_RGB, d_points, p, m, d_limbs, l, &st, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, NULL, 1, VALI_FMT_RGB, d_points, p, m, d_limbs, l, &st, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, NULL, p, m, d_limbs, l, &st, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, d_points, p, m, d_limbs, l, NULL, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, d_points, p, m, d_limbs, l, &st, NULL, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 0, VALI_FMT_RGB, d_points, p, m, d_limbs, l, &st, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, d_points, 65, m, d_limbs, l, &st, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, d_points, p, 1025, d_limbs, l, &st, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, d_points, p, m, d_limbs, 129, &st, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, d_points, p, m, NULL, l, &st, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, (char*)d_points + 4, p, m, d_limbs, l, &st, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, d_points, p, m, d_limbs, l, &st, ws, ws_bytes - 1) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, d_points, p, m, d_limbs, l, &st, (char*)ws + 8, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_BGR, d_points, p, m, d_limbs, l, &st, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_Y, d_points, p, m, d_limbs, l, &st, ws, ws_bytes) != VALI_ERR_UNSUPPORTED) return 4;
  bst.thickness = 0;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, d_points, p, m, d_limbs, l, &bst, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  bst = st;
  bst.diameter = 65;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, d_points, p, m, d_limbs, l, &bst, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  bst = st;
  bst.alpha = 256;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, d_points, p, m, d_limbs, l, &bst, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  bst = st;
  bst.n_limb_colours = 0;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, d_points, p, m, d_limbs, l, &bst, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  bst = st;
  bst.d_joint_colours = NULL;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, d_points, p, m, d_limbs, l, &bst, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;

  CHECK(DECODE(d_desc, 1, &in, d_mats, NULL, d_points, d_kpts));
  CHECK(PAINT(&desc, d_desc, 1, VALI_FMT_RGB, d_points, p, m, d_limbs, l, &st, ws, ws_bytes));
  CHECK(vali_memcpy2d_async(dev, got, fbytes, d_frame, fbytes, fbytes, 1, 1, stream));
  CHECK(vali_memcpy2d_async(dev, points, pbytes, d_points, pbytes, pbytes, 1, 1, stream));
  CHECK(vali_memcpy2d_async(dev, kpts, kbytes, d_kpts, kbytes, kbytes, 1, 1, stream));
  CHECK(vali_stream_sync(dev, stream));
  if (write_file(argv[23], got, fbytes) || write_file(argv[24], points, pbytes) || write_file(argv[25], kpts, kbytes)) return 2;
  const int equal = memcmp(got, want, fbytes) == 0;
  const int points_equal = memcmp(points, want_points, pbytes) == 0;
  const int kpts_equal = memcmp(kpts, want_kpts, kbytes) == 0;

  vali_mem_free(dev, d_frame); vali_mem_free(dev, d_heat); vali_mem_free(dev, d_mats); vali_mem_free(dev, d_limbs);
  vali_mem_free(dev, d_lcol); vali_mem_free(dev, d_jcol); vali_mem_free(dev, d_desc); vali_mem_free(dev, d_points);
  vali_mem_free(dev, d_kpts); vali_mem_free(dev, ws);
  vali_stream_destroy(dev, stream);
  free(frame); free(heat); free(mats); free(limbs); free(lcol); free(jcol); free(want); free(want_points);
  free(want_kpts); free(got); free(points); free(kpts);
  if (!points_equal) {
    fprintf(stderr, "the points differ from want_points.bin\n");
    return 6;
  }
  if (!kpts_equal) {
    fprintf(stderr, "the kpts differ from want_kpts.bin\n");
    return 7;
  }
  if (!equal) {
    fprintf(stderr, "the drawn frame differs from want.bin\n");
    return 5;
  }
  printf("ok %s\n", vali_version());
  return 0;
}
