/* A plain C99 client of vali_annotate_batch_atlas (include/vali_hip.h).
 * Two frames of one format (NV12 or RGB) and of different sizes come from a file as tightly packed host images, back to
 * back; the marks come from a file of int32 rows, the coverage atlas from a file of aw x ah bytes.  The atlas is placed
 * at an odd offset inside an allocation of 255s with a pitch of aw + 6; the frames are uploaded into pitched
 * allocations, drawn on, read back and compared with the bytes of want.bin, which tests/test_gpu_c_abi_stamps.py wrote
 * with tests/annotate_stamp_model.py.  For NV12 the colours go through nppiRGBToYUV's matrix.
 *   usage: stamp_client <nv12|rgb> <w0> <h0> <w1> <h1> <frames.bin> <marks.bin> <m> <want.bin> <got.bin> <atlas.bin> <aw> <ah>
 * exit status 0: equal; 5: the frames differ (got.bin holds them); 4: a refusal did not come. */
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

int main(int argc, char** argv) {
  if (argc != 14) {
    fprintf(stderr, "usage: %s nv12|rgb w0 h0 w1 h1 frames.bin marks.bin m want.bin got.bin atlas.bin aw ah\n", argv[0]);
    return 2;
  }
  const int aw = atoi(argv[12]), ah = atoi(argv[13]);
  if (aw < 1 || ah < 1) return 2;
  const int nv12 = strcmp(argv[1], "nv12") == 0, dev = 0, n = 2;
  const int format = nv12 ? VALI_FMT_NV12 : VALI_FMT_RGB;
  const int w[2] = {atoi(argv[2]), atoi(argv[4])}, h[2] = {atoi(argv[3]), atoi(argv[5])};
  const int m = atoi(argv[8]);
  size_t rows[2], cols[2], bytes[2], total = 0;
  for (int i = 0; i < n; ++i) {
    if (w[i] < 1 || h[i] < 1) return 2;
    rows[i] = nv12 ? (size_t)h[i] * 3 / 2 : (size_t)h[i];
    cols[i] = nv12 ? (size_t)w[i] : (size_t)w[i] * 3;
    bytes[i] = rows[i] * cols[i];
    total += bytes[i];
  }
  unsigned char* host = read_file(argv[6], total);
  unsigned char* want = read_file(argv[9], total);
  unsigned char* hmarks = read_file(argv[7], (size_t)m * sizeof(vali_mark));
  unsigned char* got = (unsigned char*)malloc(total);
  unsigned char* hatlas = read_file(argv[11], (size_t)aw * (size_t)ah);
  const size_t apitch = (size_t)aw + 6, abytes = apitch * ((size_t)ah + 2);
  unsigned char* around = (unsigned char*)malloc(abytes);
  if (!host || !want || !hmarks || !got || !hatlas || !around) return 2;
  memset(around, 255, abytes);
  for (int y = 0; y < ah; ++y)
    memcpy(around + ((size_t)y + 1) * apitch + 3, hatlas + (size_t)y * (size_t)aw, (size_t)aw);

  int count = 0;
  CHECK(vali_device_count(&count));
  if (count < 1) {
    fprintf(stderr, "no device\n");
    return 3;
  }
  vali_stream_t stream = NULL;
  CHECK(vali_stream_create(dev, &stream));

  vali_surface frames[2];
  void* mem[2];
  size_t pitch[2], off = 0;
  for (int i = 0; i < n; ++i) {
    CHECK(vali_mem_alloc_pitch(dev, cols[i], rows[i], &mem[i], &pitch[i]));
    CHECK(vali_memcpy2d_async(dev, mem[i], pitch[i], host + off, cols[i], cols[i], rows[i], 0, stream));
    off += bytes[i];
    memset(&frames[i], 0, sizeof frames[i]);
    frames[i].plane[0] = mem[i];
    frames[i].pitch[0] = (int32_t)pitch[i];
    if (nv12) {
      frames[i].plane[1] = (char*)mem[i] + (size_t)h[i] * pitch[i];
      frames[i].pitch[1] = (int32_t)pitch[i];
    }
    frames[i].width = w[i]; frames[i].height = h[i]; frames[i].format = format;
  }
  void *d_frames = NULL, *d_marks = NULL, *ws = NULL, *d_atlas = NULL;
  size_t ws_bytes = 0;
  CHECK(vali_annotate_workspace_size(n, frames, &ws_bytes));
  CHECK(vali_mem_alloc(dev, sizeof frames, &d_frames));
  CHECK(vali_mem_alloc(dev, (size_t)m * sizeof(vali_mark) + 16, &d_marks));
  CHECK(vali_mem_alloc(dev, ws_bytes, &ws));
  CHECK(vali_mem_alloc(dev, abytes, &d_atlas));
  CHECK(vali_memcpy2d_async(dev, d_atlas, abytes, around, abytes, abytes, 1, 0, stream));
  vali_surface atlas;
  memset(&atlas, 0, sizeof atlas);
  atlas.plane[0] = (char*)d_atlas + apitch + 3;
  atlas.pitch[0] = (int32_t)apitch;
  atlas.width = aw; atlas.height = ah; atlas.format = VALI_FMT_Y;
  CHECK(vali_memcpy2d_async(dev, d_frames, sizeof frames, frames, sizeof frames, sizeof frames, 1, 0, stream));
  if (m > 0)
    CHECK(vali_memcpy2d_async(dev, d_marks, (size_t)m * sizeof(vali_mark), hmarks, (size_t)m * sizeof(vali_mark),
                              (size_t)m * sizeof(vali_mark), 1, 0, stream));

  vali_cvt_params prm;
  memset(&prm, 0, sizeof prm);
  const float yuv[3][4] = {{0.299f, 0.587f, 0.114f, 0.0f}, {-0.147f, -0.289f, 0.436f, 128.0f}, {0.615f, -0.515f, -0.100f, 128.0f}};
  memcpy(prm.rgb2yuv, yuv, sizeof yuv);

  /* refusals are decided on the host, before anything is launched */
  vali_surface bad = atlas;
  bad.format = format;
  if (vali_annotate_batch_atlas(frames, (const vali_surface*)d_frames, n, format, (const vali_mark*)d_marks, m, &bad, &prm, ws,
                                ws_bytes, stream) != VALI_ERR_INVALID_ARG)
    return 4;
  bad = atlas;
  bad.pitch[0] = aw - 1;
  if (vali_annotate_batch_atlas(frames, (const vali_surface*)d_frames, n, format, (const vali_mark*)d_marks, m, &bad, &prm, ws,
                                ws_bytes, stream) != VALI_ERR_INVALID_ARG)
    return 4;
  if (vali_annotate_batch_atlas(frames, (const vali_surface*)d_frames, n, format, (const vali_mark*)d_marks, VALI_MAX_MARKS + 1,
                                &atlas, &prm, ws, ws_bytes, stream) != VALI_ERR_INVALID_ARG)
    return 4;

  CHECK(vali_annotate_batch_atlas(frames, (const vali_surface*)d_frames, n, format, (const vali_mark*)d_marks, m, &atlas,
                                  nv12 ? &prm : NULL, ws, ws_bytes, stream));

  off = 0;
  for (int i = 0; i < n; ++i) {
    CHECK(vali_memcpy2d_async(dev, got + off, cols[i], mem[i], pitch[i], cols[i], rows[i], 1, stream));
    off += bytes[i];
  }
  CHECK(vali_stream_sync(dev, stream));
  FILE* o = fopen(argv[10], "wb");
  if (!o || fwrite(got, 1, total, o) != total) return 2;
  fclose(o);
  const int equal = memcmp(got, want, total) == 0;

  for (int i = 0; i < n; ++i) vali_mem_free(dev, mem[i]);
  vali_mem_free(dev, d_frames); vali_mem_free(dev, d_marks); vali_mem_free(dev, ws); vali_mem_free(dev, d_atlas);
  vali_stream_destroy(dev, stream);
  free(host); free(want); free(hmarks); free(got); free(hatlas); free(around);
  if (!equal) {
    fprintf(stderr, "the frames differ from want.bin\n");
    return 5;
  }
  printf("ok %s\n", vali_version());
  return 0;
}
