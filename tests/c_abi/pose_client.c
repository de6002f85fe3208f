/* A plain C99 client of vali_pose_workspace_size / vali_pose_paint (include/vali_hip.h).
 * One tightly packed RGB frame of w x h comes from a file, with float32 keypoints (1, k, p, 3), d detection rows of 8
 * int32, the frame's record of 8 int32, l limb pairs, three limb colours and two joint colours.  One call draws the
 * skeletons; the frame and the points are read back, written to got.bin and points.bin and compared with want.bin and
 * want_points.bin, which tests/test_gpu_c_abi_pose.py wrote with tests/pose_model.py.
 *   usage: pose_client <w> <h> <k> <p> <d> <l> <thr> <thickness> <diameter> <alpha> <frame.bin> <kpts.bin> <dets.bin>
 *                      <rect.bin> <limbs.bin> <limb_colours.bin> <joint_colours.bin> <want.bin> <want_points.bin>
 *                      <got.bin> <points.bin>
 * exit status 0: equal; 5: the frames differ (got.bin holds the drawn one); 6: the points differ; 4: a refusal did not
 * come. */
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
  if (argc != 22) {
    fprintf(stderr, "usage: %s w h k p d l thr thickness diameter alpha frame kpts dets rect limbs limb_colours "
                    "joint_colours want want_points got points\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[1]), h = atoi(argv[2]), k = atoi(argv[3]), p = atoi(argv[4]), d = atoi(argv[5]);
  const int l = atoi(argv[6]), thickness = atoi(argv[8]), diameter = atoi(argv[9]), alpha = atoi(argv[10]);
  const float thr = (float)atof(argv[7]);
  const int dev = 0;
  if (w < 1 || h < 1 || k < 1 || p < 1 || d < 1 || l < 1) return 2;
  const size_t fbytes = (size_t)w * h * 3, kbytes = (size_t)k * p * 3 * sizeof(float);
  const size_t dbytes = (size_t)d * 8 * sizeof(int32_t), lbytes = (size_t)l * 2 * sizeof(int32_t);
  const size_t pbytes = (size_t)d * p * 4 * sizeof(int32_t);
  unsigned char* frame = read_file(argv[11], fbytes);
  unsigned char* kpts = read_file(argv[12], kbytes);
  unsigned char* dets = read_file(argv[13], dbytes);
  unsigned char* rect = read_file(argv[14], sizeof(vali_roi));
  unsigned char* limbs = read_file(argv[15], lbytes);
  unsigned char* lcol = read_file(argv[16], 3 * sizeof(int32_t));
  unsigned char* jcol = read_file(argv[17], 2 * sizeof(int32_t));
  unsigned char* want = read_file(argv[18], fbytes);
  unsigned char* want_points = read_file(argv[19], pbytes);
  unsigned char* got = (unsigned char*)malloc(fbytes);
  unsigned char* points = (unsigned char*)malloc(pbytes);
  if (!frame || !kpts || !dets || !rect || !limbs || !lcol || !jcol || !want || !want_points || !got || !points) return 2;

  int count = 0;
  CHECK(vali_device_count(&count));
  if (count < 1) {
    fprintf(stderr, "no device\n");
    return 3;
  }
  vali_stream_t stream = NULL;
  CHECK(vali_stream_create(dev, &stream));

  void *d_frame = NULL, *d_kpts = NULL, *d_dets = NULL, *d_rect = NULL, *d_limbs = NULL, *d_lcol = NULL, *d_jcol = NULL;
  void *d_desc = NULL, *d_points = NULL, *ws = NULL;
  if (upload(dev, &d_frame, frame, fbytes, stream) || upload(dev, &d_kpts, kpts, kbytes, stream) ||
      upload(dev, &d_dets, dets, dbytes, stream) || upload(dev, &d_rect, rect, sizeof(vali_roi), stream) ||
      upload(dev, &d_limbs, limbs, lbytes, stream) || upload(dev, &d_lcol, lcol, 3 * sizeof(int32_t), stream) ||
      upload(dev, &d_jcol, jcol, 2 * sizeof(int32_t), stream))
    return 1;
  vali_surface desc;
  memset(&desc, 0, sizeof desc);
  desc.plane[0] = d_frame;
  desc.pitch[0] = 3 * w;
  desc.width = w; desc.height = h; desc.format = VALI_FMT_RGB;
  if (upload(dev, &d_desc, &desc, sizeof desc, stream)) return 1;
  CHECK(vali_mem_alloc(dev, pbytes, &d_points));

  const size_t ws_bytes = vali_pose_workspace_size(1, d, p);
  if (ws_bytes != (size_t)d * (1 + p) * 16 || vali_pose_workspace_size(1, d, 65) != 0 ||
      vali_pose_workspace_size(1, 1025, p) != 0 || vali_pose_workspace_size(0, d, p) != 0)
    return 4;
  CHECK(vali_mem_alloc(dev, ws_bytes, &ws));

  vali_pose_in in;
  memset(&in, 0, sizeof in);
  in.kpts = d_kpts; in.dtype = VALI_DTYPE_F32; in.kdim = 3;
  in.stride_n = (int64_t)k * p * 3; in.stride_k = (int64_t)p * 3; in.stride_p = 3; in.stride_c = 1;
  in.k = k; in.p = p; in.max_det = d; in.n_limbs = l;
  in.d_limbs = (const int32_t*)d_limbs;
  vali_pose_style st;
  memset(&st, 0, sizeof st);
  st.d_limb_colours = (const int32_t*)d_lcol; st.d_joint_colours = (const int32_t*)d_jcol;
  st.n_limb_colours = 3; st.n_joint_colours = 2;
  st.kpt_thr = thr; st.thickness = thickness; st.diameter = diameter; st.alpha = alpha;

#define PAINT(FRAMES, DFRAMES, N, FMT, IN, DETS, RECTS, STYLE, POINTS, WS, WSB)                                        \
  vali_pose_paint(FRAMES, (const vali_surface*)(DFRAMES), N, FMT, IN, (const int32_t*)(DETS), (const vali_roi*)(RECTS), \
                  STYLE, (int32_t*)(POINTS), NULL, WS, WSB, stream)
  /* refusals are decided on the host, before anything is launched */
  vali_pose_in bad = in;
  bad.p = 65;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &bad, d_dets, d_rect, &st, d_points, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  bad = in;
  bad.kdim = 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &bad, d_dets, d_rect, &st, d_points, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  bad = in;
  bad.dtype = 3;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &bad, d_dets, d_rect, &st, d_points, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  bad = in;
  bad.stride_p = -1;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &bad, d_dets, d_rect, &st, d_points, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  bad = in;
  bad.n_limbs = 129;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &bad, d_dets, d_rect, &st, d_points, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  bad = in;
  bad.d_limbs = NULL;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &bad, d_dets, d_rect, &st, d_points, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  vali_pose_style bst = st;
  bst.thickness = 0;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_dets, d_rect, &bst, d_points, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  bst = st;
  bst.diameter = 65;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_dets, d_rect, &bst, d_points, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  bst = st;
  bst.alpha = 256;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_dets, d_rect, &bst, d_points, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  bst = st;
  bst.n_joint_colours = 0;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_dets, d_rect, &bst, d_points, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, NULL, d_rect, &st, d_points, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_dets, NULL, &st, d_points, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_dets, d_rect, NULL, d_points, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_dets, d_rect, &st, (char*)d_points + 4, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_dets, d_rect, &st, d_points, ws, ws_bytes - 1) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_dets, d_rect, &st, d_points, (char*)ws + 8, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_BGR, &in, d_dets, d_rect, &st, d_points, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;
  if (PAINT(&desc, d_desc, 1, VALI_FMT_Y, &in, d_dets, d_rect, &st, d_points, ws, ws_bytes) != VALI_ERR_UNSUPPORTED) return 4;
  if (PAINT(&desc, d_desc, 0, VALI_FMT_RGB, &in, d_dets, d_rect, &st, d_points, ws, ws_bytes) != VALI_ERR_INVALID_ARG) return 4;

  CHECK(PAINT(&desc, d_desc, 1, VALI_FMT_RGB, &in, d_dets, d_rect, &st, d_points, ws, ws_bytes));
  CHECK(vali_memcpy2d_async(dev, got, fbytes, d_frame, fbytes, fbytes, 1, 1, stream));
  CHECK(vali_memcpy2d_async(dev, points, pbytes, d_points, pbytes, pbytes, 1, 1, stream));
  CHECK(vali_stream_sync(dev, stream));
  if (write_file(argv[20], got, fbytes) || write_file(argv[21], points, pbytes)) return 2;
  const int equal = memcmp(got, want, fbytes) == 0;
  const int points_equal = memcmp(points, want_points, pbytes) == 0;

  vali_mem_free(dev, d_frame); vali_mem_free(dev, d_kpts); vali_mem_free(dev, d_dets); vali_mem_free(dev, d_rect);
  vali_mem_free(dev, d_limbs); vali_mem_free(dev, d_lcol); vali_mem_free(dev, d_jcol); vali_mem_free(dev, d_desc);
  vali_mem_free(dev, d_points); vali_mem_free(dev, ws);
  vali_stream_destroy(dev, stream);
  free(frame); free(kpts); free(dets); free(rect); free(limbs); free(lcol); free(jcol); free(want); free(want_points);
  free(got); free(points);
  if (!equal) {
    fprintf(stderr, "the drawn frame differs from want.bin\n");
    return 5;
  }
  if (!points_equal) {
    fprintf(stderr, "the points differ from want_points.bin\n");
    return 6;
  }
  printf("ok %s\n", vali_version());
  return 0;
}
