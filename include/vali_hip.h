/*
 * vali_hip.h -- C ABI of libvali_hip.so, the MI355X (gfx950) surface-processing
 * kernel library behind the python_vali Surface/Task API.
 *
 * This header is the drop-in boundary of the hot path.  In the reference the
 * same boundary is the table of dlsym'd NVIDIA NPP entry points
 * (reference: src/TC/inc/LibNpp.hpp:35-198, loader src/TC/src/LibNpp.cpp:20-51)
 * plus the two first-party launchers UD_NV12 / UD_NV12_HBD
 * (reference: src/TC/inc/ResizeUtils.hpp:30-50) and the CUDA driver calls of
 * src/TC/inc/LibCuda.hpp.  Conventions are the NPP ones:
 *   - raw device pointers + byte pitches, sizes in pixels, no allocation and no
 *     ownership transfer inside an operator;
 *   - every operator is asynchronous on `stream` (a hipStream_t passed as void*);
 *   - return 0 on success, a negative VALI_ERR_* otherwise; the text of the last
 *     failure on the calling thread is vali_last_error().
 * No torch / pybind11 / C++ types appear in any signature.
 */
#ifndef VALI_HIP_H
#define VALI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VALI_API __attribute__((visibility("default")))

/* ---- status codes ------------------------------------------------------- */
#define VALI_OK 0
#define VALI_ERR_INVALID_ARG (-1) /* null pointer, bad size, bad enum value      */
#define VALI_ERR_UNSUPPORTED (-2) /* format pair / parameter combination absent  */
#define VALI_ERR_RUNTIME (-3)     /* a HIP runtime call failed                   */
#define VALI_ERR_NO_DEVICE (-4)   /* no usable GPU                               */

/* ---- pixel formats: numbering identical to the reference's Pixel_Format
 *      (reference: src/TC/inc/MemoryInterfaces.hpp:29-46) ------------------- */
enum vali_pixel_format {
  VALI_FMT_UNDEFINED = 0,
  VALI_FMT_Y = 1,
  VALI_FMT_RGB = 2,
  VALI_FMT_NV12 = 3,
  VALI_FMT_YUV420 = 4,
  VALI_FMT_RGB_PLANAR = 5,
  VALI_FMT_BGR = 6,
  VALI_FMT_YUV444 = 7,
  VALI_FMT_RGB_32F = 8,
  VALI_FMT_RGB_32F_PLANAR = 9,
  VALI_FMT_YUV422 = 10,
  VALI_FMT_P10 = 11,
  VALI_FMT_P12 = 12,
  VALI_FMT_YUV444_10BIT = 13,
  VALI_FMT_YUV420_10BIT = 14,
  VALI_FMT_GRAY12 = 15
};

typedef void* vali_stream_t; /* hipStream_t */
typedef void* vali_event_t;  /* hipEvent_t  */
typedef void* vali_graph_t;  /* hipGraphExec_t */

/*
 * A borrowed view of one surface: what the reference hands to NPP as
 * pSrc[]/nSrcStep/oSizeROI (e.g. TaskConvertSurface.cpp:120-136).
 * plane[c] is the device pointer of COMPONENT c, i.e. Surface::PixelPtr(c):
 *   NV12/P10/P12   plane[0]=Y, plane[1]=interleaved UV (= Y + height*pitch)
 *   YUV420/422/444 plane[0..2] = Y,U,V allocations
 *   RGB/BGR/RGB_32F plane[0]    = packed pixels
 *   RGB_PLANAR/RGB_32F_PLANAR plane[c] = base + c*height*pitch
 *   Y              plane[0]
 * width/height are in pixels of the full-resolution (luma) grid.
 * Every plane must be smaller than 4 GiB (the gather kernels form row offsets in 32 bits);
 * the single-surface entry points check it (VALI_ERR_INVALID_ARG), batch callers guarantee it.
 */
typedef struct vali_surface {
  void* plane[3];
  int32_t pitch[3]; /* bytes */
  int32_t width;
  int32_t height;
  int32_t format; /* enum vali_pixel_format */
} vali_surface;

/*
 * YUV -> RGB colour matrix.  One instance per NPP colour variant the reference
 * selects between in nv12_rgb / yuv420_rgb / yuv444_rgb
 * (reference: src/TC/src/TaskConvertSurface.cpp:128-149, 271-292, 360-383).
 *   Yf = cy * (Y - y0);  Uc = U - 128;  Vc = V - 128
 *   R = Yf + crv*Vc ;  G = Yf + (cgu*Uc + cgv*Vc) ;  B = Yf + cbu*Uc
 * exact operation order and rounding: oracle/vali_oracle.c (the specification).
 * This 32-byte block is what the multi-GPU pipeline broadcasts over RCCL.
 */
typedef struct vali_csc {
  float y0, cy, crv, cgu, cgv, cbu;
  float reserved[2];
} vali_csc;

/* ---- runtime: replaces the LibCuda dlsym table
 *      (reference: src/TC/inc/LibCuda.hpp, src/TC/src/CudaUtils.cpp) --------- */

VALI_API const char* vali_last_error(void);
VALI_API const char* vali_version(void);

/* cuDeviceGetCount (CudaUtils.cpp:185-205) */
VALI_API int vali_device_count(int* count);
/* Sizes of surfaces with subsampled chroma -- ONE rule for every entry point below: 4:2:0 formats (NV12, P10, P12,
 * YUV420, YUV420_10BIT) need an even width AND height, YUV422 an even width (their chroma planes hold W/2 x H/2 resp.
 * W/2 x H samples; the reference allocates with integer division and would read past them).  VALI_ERR_INVALID_ARG
 * otherwise; python_vali reports (False, TaskExecInfo.INVALID_INPUT) at Run time -- Surface.Make itself, like the
 * reference's, allocates any size. */

/* cuCtxPushCurrent of the reference's CudaCtxPush (CudaUtils.hpp:29-47), without the pop: makes `device` the calling
 * thread's current device.  Every entry point that takes a stream runs on the STREAM's device; the null stream has
 * none and means "the legacy default stream of the thread's current device" -- a host that is handed stream 0 together
 * with a GPU index (python_vali's Task(gpu_id, stream) constructors) calls this first. */
VALI_API int vali_device_set(int device);
/* the calling thread's current device (cuCtxGetCurrent): what a caller saves before vali_device_set and puts back after
 * the call -- the pop of the reference's CudaCtxPush (CudaUtils.hpp:29-47) */
VALI_API int vali_device_get(int* device);
/* device of a device pointer: GetDeviceIdByDptr (CudaUtils.cpp:150-163) */
VALI_API int vali_ptr_device(const void* dptr, int* device);

/* one non-blocking stream per call: cuStreamCreate(CU_STREAM_NON_BLOCKING)
 * (CudaUtils.cpp:222-238) */
VALI_API int vali_stream_create(int device, vali_stream_t* stream);
/* waits for what the stream has been given (hipStreamSynchronize), drops the library's per-stream state (completion word,
 * tap-table reader lists), then destroys it */
VALI_API int vali_stream_destroy(int device, vali_stream_t stream);
VALI_API int vali_stream_sync(int device, vali_stream_t stream);
/* the same guarantee -- everything issued on `stream` so far has finished -- through a host-visible completion word the
 * stream writes (hipStreamWriteValue32 into pinned memory) and the caller spins on: 3 us less per blocking call than
 * hipStreamSynchronize around a small kernel; falls back to it after ~150 us.  The blocking Run forms of python_vali
 * (Run = RunAsync + event record + host wait, PySurfaceConverter.cpp:76-86) end here. */
VALI_API int vali_stream_wait(int device, vali_stream_t stream);

/* CudaStreamEvent (CudaUtils.cpp:35-68); timing enabled so bench.py can use them */
VALI_API int vali_event_create(int device, vali_event_t* event);
VALI_API int vali_event_destroy(int device, vali_event_t event);
VALI_API int vali_event_record(int device, vali_event_t event, vali_stream_t stream);
VALI_API int vali_event_sync(int device, vali_event_t event);
/* cuEventQuery: *done = 1 when the event has happened, 0 while work in front of it is still running (no wait) */
VALI_API int vali_event_query(int device, vali_event_t event, int* done);
/* cuStreamWaitEvent: work issued on `stream` after this call starts only when `event` has happened (no host wait).  The
 * ingest ring of the batched pipeline orders its copy stream and its compute stream with it. */
VALI_API int vali_stream_wait_event(int device, vali_stream_t stream, vali_event_t event);
VALI_API int vali_event_elapsed_ms(vali_event_t start, vali_event_t stop, float* ms);

/*
 * Stream capture (no reference counterpart: the reference issues every NPP call eagerly).
 * Per-frame chains of small launches (BASELINE config 2: 1080p, batch 1) are bound by the
 * ~5 us host cost of each launch, not by the GPU.  Between capture_begin and capture_end every
 * asynchronous vali_* call on `stream` is RECORDED instead of executed (device pointers and
 * sizes are frozen into the graph); vali_graph_launch replays the whole chain with one
 * submission.  Capture is thread-local; do not synchronise or allocate while capturing.
 */
VALI_API int vali_graph_capture_begin(int device, vali_stream_t stream);
VALI_API int vali_graph_capture_end(int device, vali_stream_t stream, vali_graph_t* graph);
VALI_API int vali_graph_launch(int device, vali_graph_t graph, vali_stream_t stream);
VALI_API int vali_graph_destroy(int device, vali_graph_t graph);

/* cuMemAllocPitch / cuMemAlloc / cuMemFree (SurfacePlane.cpp:186-213).
 * Pitch policy: width_bytes rounded up to 256 B, so every row starts on two
 * 128-byte lines and 16-byte vector access is always legal. */
VALI_API int vali_mem_alloc_pitch(int device, size_t width_bytes, size_t height,
                                  void** dptr, size_t* pitch);
VALI_API int vali_mem_alloc(int device, size_t bytes, void** dptr);
VALI_API int vali_mem_free(int device, void* dptr);
/* page-locked host memory (cuMemAllocHost): the staging buffers of asynchronous host <-> device copies; pageable memory
 * makes vali_memcpy2d_async synchronous and halves its rate */
VALI_API int vali_host_alloc(int device, size_t bytes, void** hptr);
VALI_API int vali_host_free(int device, void* hptr);
/* free / total bytes of the device (cuMemGetInfo): bench.py's pre-flight check */
VALI_API int vali_mem_info(int device, size_t* free_bytes, size_t* total_bytes);
/* PCI address "dddd:bb:dd.f" of the device (cuDeviceGetPCIBusId), for NUMA placement of its host thread */
VALI_API int vali_device_pci_bus_id(int device, char* out, int len);

/* cuMemcpy2DAsync (TaskCudaUploadFrame.cpp:54-72, TaskCudaDownloadSurface.cpp:54-72,
 * MemoryInterfaces.cpp:413-431).  kind: 0 = host->device, 1 = device->host,
 * 2 = device->device. */
VALI_API int vali_memcpy2d_async(int device, void* dst, size_t dst_pitch,
                                 const void* src, size_t src_pitch,
                                 size_t width_bytes, size_t height, int kind,
                                 vali_stream_t stream);
VALI_API int vali_memset2d_async(int device, void* dst, size_t dst_pitch, int value,
                                 size_t width_bytes, size_t height,
                                 vali_stream_t stream);

/* ---- colour conversion: replaces the NPP nppicc entry points ---------------- */

/*
 * NV12 -> RGB / BGR (packed u8) or RGB_PLANAR (u8); any other dst->format returns
 * VALI_ERR_UNSUPPORTED.  (Float outputs -- the fused form of the reference's
 * NV12->RGB->RGB_32F(->PLANAR) chain -- are vali_nv12_preproc below.)
 * Replaces nppiNV12ToRGB_709HDTV_8u_P2C3R_Ctx, nppiNV12ToRGB_709CSC_8u_P2C3R_Ctx,
 * nppiNV12ToRGB_8u_P2C3R_Ctx and their BGR twins
 * (reference call sites: TaskConvertSurface.cpp:61-156; LibNpp.hpp table).
 * dst->format selects the output layout; src->format must be VALI_FMT_NV12.
 */
VALI_API int vali_nv12_to_rgb(const vali_surface* src, const vali_surface* dst,
                              const vali_csc* csc, vali_stream_t stream);

/*
 * Batched form: ONE launch over n independent frames of identical geometry.
 * d_src / d_dst are DEVICE arrays of n vali_surface descriptors (upload them
 * once with vali_memcpy2d_async or hipMemcpy); width/height/dst_format restate
 * the common geometry for grid sizing.  Semantics per frame are exactly those
 * of vali_nv12_to_rgb.  Precedent for the list-in / one-sync idiom:
 * reference src/python_vali/src/PyNvJpegEncoder.cpp:31-81.
 */
VALI_API int vali_nv12_to_rgb_batch(const vali_surface* d_src,
                                    const vali_surface* d_dst, int n, int width,
                                    int height, int dst_format, const vali_csc* csc,
                                    vali_stream_t stream);

/*
 * Parameters of the generic converter.  yuv2rgb is used by YUV -> RGB pairs; rgb2yuv by
 * RGB -> YUV / grey pairs: row c = (kR, kG, kB, offset) of output channel c (Y, U/Cb, V/Cr),
 *   out_c = kB*B + (kG*G + (kR*R + offset))   evaluated with fused multiply-adds.
 */
typedef struct vali_cvt_params {
  vali_csc yuv2rgb;
  float rgb2yuv[3][4];
} vali_cvt_params;

/*
 * Every other 8-bit pair of ConvertSurface::GetSupportedConversions()
 * (reference: src/TC/src/TaskConvertSurface.cpp:966-994) plus the three element-type
 * conversions, selected by (src->format, dst->format):
 *   NV12<->YUV420, NV12->Y, Y->YUV444, RGB<->RGB_PLANAR, RGB<->BGR   byte permutations
 *   YUV420->RGB/BGR, YUV444->RGB/BGR, NV12->RGB/BGR/RGB_PLANAR       params->yuv2rgb
 *   RGB/BGR/RGB_PLANAR->YUV444, RGB->YUV420, RGB->Y                  params->rgb2yuv
 *   P10/P12->NV12 (round(v/256), saturated), RGB->RGB_32F (v/255), RGB_32F->RGB_32F_PLANAR
 * replacing the NPP calls listed at the top of vali_amd/csrc/cvt_generic.hip.
 * 4:2:0 formats need even width and height.  Unsupported pair -> VALI_ERR_UNSUPPORTED.
 */
VALI_API int vali_convert(const vali_surface* src, const vali_surface* dst,
                          const vali_cvt_params* params, vali_stream_t stream);
VALI_API int vali_convert_batch(const vali_surface* d_src, const vali_surface* d_dst, int n,
                                int src_format, int dst_format, int width, int height,
                                const vali_cvt_params* params, vali_stream_t stream);

/* ---- fused inference pre-processing ------------------------------- */

/*
 * NV12 -> (bilinear resize to the dst size) -> RGB u8 -> float -> normalised, one launch.
 * No reference kernel: replaces the CHAIN the reference's samples run
 * (tests/test_TorchSegmentation.py:176-240): PySurfaceConverter NV12->RGB, RGB->RGB_32F
 * (nppiScale_8u32f_C3R, v/255), RGB_32F->RGB_32F_PLANAR, torch.divide(x, 255.0),
 * torchvision Normalize -- optionally behind a PySurfaceResizer.  Defined as that chain step
 * by step and bit-identical to running it with vali_resize + vali_nv12_to_rgb + vali_convert:
 *   q_c   = u8 RGB of vali_nv12_to_rgb(csc) on the (resized) NV12
 *   out_c = ((q_c / 255.0f) / div - mean[c]) / std_[c]          c = R, G, B ; IEEE float32
 * div = 1, mean = 0, std_ = 1 gives plain NV12 -> RGB_32F[_PLANAR].
 * dst->format: VALI_FMT_RGB_32F_PLANAR or VALI_FMT_RGB_32F; all four sizes even.
 * 8-bit destinations (VALI_FMT_RGB, VALI_FMT_BGR, VALI_FMT_RGB_PLANAR) stop after q_c: the
 * fused form of PySurfaceResizer -> PySurfaceConverter; div / mean / std_ are ignored.
 */
typedef struct vali_preproc_params {
  vali_csc csc;
  float div;
  float mean[3];
  float std_[3];
  float reserved;
} vali_preproc_params;

VALI_API int vali_nv12_preproc(const vali_surface* src, const vali_surface* dst,
                               const vali_preproc_params* params, vali_stream_t stream);
VALI_API int vali_nv12_preproc_batch(const vali_surface* d_src, const vali_surface* d_dst, int n,
                                     int src_width, int src_height, int dst_width, int dst_height,
                                     int dst_format, const vali_preproc_params* params,
                                     vali_stream_t stream);

/*
 * Regions: crop, letterbox, mosaic.  Item i takes the rectangle `src_*` of its NV12 source
 * (luma pixels) and places it at the rectangle `dst_*` of its destination (destination pixels).
 * Inside the placement the result is bit-identical to vali_nv12_preproc on the two views
 *   view(src, crop)  = plane[0] + src_y * pitch[0] + src_x, plane[1] + (src_y / 2) * pitch[1] + src_x,
 *                      src_w x src_h
 *   view(dst, place) = every plane + dst_y * pitch + dst_x * (bytes per pixel of dst->format),
 *                      dst_w x dst_h
 * so sampling never reads outside the crop.  Outside the placement, with pad != 0 every pixel is
 * the colour pad_rgb = (R, G, B) in u8 taken through the same definition: out_c =
 * ((pad_rgb[c] / 255.0f) / div - mean[c]) / std_[c] for float destinations, the bytes themselves
 * (in the format's memory order) for 8-bit ones.  With pad == 0 those pixels are not written
 * (a mosaic).  pad_rgb is read at call time (it may be NULL when pad == 0).
 * All eight values are even (4:2:0 chroma); both rectangles are at least 2 x 2 and lie inside
 * their surfaces.  dst->format / dst_format and the normalisation as for vali_nv12_preproc.
 */
typedef struct vali_roi {
  int32_t src_x, src_y, src_w, src_h; /* crop, source luma pixels, even */
  int32_t dst_x, dst_y, dst_w, dst_h; /* placement, destination pixels, even */
} vali_roi;                           /* 32 bytes; arrays of it are read by the kernel */

/* roi is in host memory and checked strictly (VALI_ERR_INVALID_ARG); it travels in the kernel arguments */
VALI_API int vali_nv12_preproc_roi(const vali_surface* src, const vali_surface* dst, const vali_roi* roi,
                                   const vali_preproc_params* params, int pad, const uint8_t pad_rgb[3],
                                   vali_stream_t stream);
/*
 * Batched form: d_src, d_dst and d_roi are DEVICE arrays of n (0..65535) entries.  The sources
 * may differ in size (each item reads its own descriptor) and may repeat; the destinations share
 * dst_width x dst_height and dst_format.  The rectangles cannot be checked on the host, so the
 * kernel sanitises each one against its own surface (W x H):
 *   x = clamp(x, 0, W) rounded down to even;  w = clamp(w, 0, W - x) rounded down to even
 *   (y / h likewise against H; the placement against the destination's size)
 * An item whose crop or placement is then narrower or shorter than 2 is empty: its destination
 * is all pad (pad != 0) or untouched (pad == 0).  Whatever the rectangles hold, an item reads only
 * inside src[i] and writes only inside dst[i]; a valid rectangle is left as it is.
 */
VALI_API int vali_nv12_preproc_roi_batch(const vali_surface* d_src, const vali_surface* d_dst,
                                         const vali_roi* d_roi, int n, int dst_width, int dst_height,
                                         int dst_format, const vali_preproc_params* params, int pad,
                                         const uint8_t pad_rgb[3], vali_stream_t stream);

/*
 * Regions of RGB-family sources: what a decoder gives for files that are not 4:2:0 of even size.
 * Source VALI_FMT_RGB, VALI_FMT_BGR or VALI_FMT_RGB_PLANAR (8 bit); destination VALI_FMT_RGB_32F_PLANAR,
 * VALI_FMT_RGB_32F, VALI_FMT_RGB, VALI_FMT_BGR or VALI_FMT_RGB_PLANAR, as for NV12.  For a crop (src_x, src_y,
 * src_w, src_h) of the source placed at (dst_x, dst_y, dst_w, dst_h) of the destination, inside the placement:
 *   1. q = the bilinear resize of the crop VIEW to dst_w x dst_h, channel by channel, exactly as
 *      vali_resize(..., VALI_INTERP_LINEAR) does it for that format: scales (float)src_w / (float)dst_w and
 *      (float)src_h / (float)dst_h, grid src = dst * scale, t0 / t1 / v by fma, round-half-even to u8; the taps
 *      never leave the crop.  Equal sizes: q is the texel.
 *   2. the channels are named by colour, not by position: q_R, q_G, q_B whatever the source's memory order.
 *   3. float destinations: out_c = ((q_c / 255.0f) / div - mean[c]) / std_[c], c = R, G, B, IEEE float32 (step 3 of
 *      vali_nv12_preproc).  8-bit destinations: the bytes q_c in the destination's memory order; div / mean / std_
 *      are ignored.
 * Outside the placement: the pad colour through step 3, or nothing written (pad == 0) -- the NV12 rule.
 * There is NO colour matrix: params->csc is ignored.
 * There is NO evenness rule: sizes, crops and placements are any integers; a rectangle is at least 1 x 1 and lies
 * inside its surface.  The result is bit-identical to vali_resize on the views, vali_convert to the destination's
 * layout, then step 3.
 * roi is in host memory and checked strictly (VALI_ERR_INVALID_ARG); NULL = the whole source onto the whole
 * destination.  Formats outside the lists: VALI_ERR_UNSUPPORTED.  Both are decided before any device is touched.
 */
VALI_API int vali_rgb_preproc_roi(const vali_surface* src, const vali_surface* dst, const vali_roi* roi,
                                  const vali_preproc_params* params, int pad, const uint8_t pad_rgb[3],
                                  vali_stream_t stream);
/*
 * Batched form: device arrays of n (0..65535) entries; all sources have the format src_format (their sizes may
 * differ, they may repeat), the destinations share dst_width x dst_height and dst_format.  d_roi == NULL: every
 * item is its whole source onto its whole destination.  Device rectangles are sanitised by clamping only:
 *   x = clamp(x, 0, W);  w = clamp(w, 0, W - x)      (y / h likewise; the placement against the destination)
 * An item whose crop or placement is then narrower or shorter than 1 is empty: all pad, or untouched.  Whatever
 * the records hold, an item reads only inside src[i] and writes only inside dst[i].
 */
VALI_API int vali_rgb_preproc_roi_batch(const vali_surface* d_src, const vali_surface* d_dst, const vali_roi* d_roi,
                                        int n, int src_format, int dst_width, int dst_height, int dst_format,
                                        const vali_preproc_params* params, int pad, const uint8_t pad_rgb[3],
                                        vali_stream_t stream);

/*
 * Regions into ONE batch tensor: the network's input itself, float32, float16 or bfloat16, with no surfaces in
 * between.  For item i, colour c (0 = R, 1 = G, 2 = B by name, whatever the source's memory order) and pixel (x, y) of
 * the canvas dst->width x dst->height:
 *   element (i, c, y, x) = convert(dtype, v),
 *   v = the float32 that vali_nv12_preproc_roi_batch / vali_rgb_preproc_roi_batch write to a VALI_FMT_RGB_32F_PLANAR
 *       destination of the canvas size from the same sources, rectangle records, parameters and pad colour.
 * convert: the identity for VALI_DTYPE_F32; IEEE round-to-nearest-even for VALI_DTYPE_F16 (subnormals are kept,
 * magnitudes that round past 65504 become +-inf) and for VALI_DTYPE_BF16.  Element (i, c, y, x) lies at
 *   planar (packed == 0):        data + (i * stride_n + c * stride_c + y * stride_y + x) * element size
 *   channels last (packed == 1): data + (i * stride_n + y * stride_y + 3 * x + c) * element size
 * so a contiguous (N, 3, H, W) tensor, any slice of it that keeps rows contiguous, and a channels-last tensor all
 * fit as they are.  With pad == 0 elements outside the placement are not written.
 * d_src is a DEVICE array of dst->n descriptors (NV12 of even size / all of src_format: RGB, BGR or RGB_PLANAR);
 * d_roi is a DEVICE array of dst->n records, sanitised on the device by the rules of the batched forms above, or
 * NULL: every item is its whole source onto the whole canvas.  dst is a HOST struct that travels in the kernel
 * arguments.  One launch; nothing is allocated, nothing synchronises.
 * VALI_ERR_INVALID_ARG, before any device is touched, for: null arguments; dtype or packed out of range; n outside
 * 1..65535; a canvas below 1 x 1 (NV12: below 2 x 2 or odd); strides <= 0; stride_y below the row's extent (width,
 * 3 * width when packed); data not aligned to the element; a row pitch of 2 GiB or more or a plane (height x pitch,
 * in bytes) of 4 GiB or more; pad without a colour.  VALI_ERR_UNSUPPORTED for a src_format outside the list.
 */
enum vali_dtype { VALI_DTYPE_F32 = 0, VALI_DTYPE_F16 = 1, VALI_DTYPE_BF16 = 2,
                  VALI_DTYPE_U8 = 3 /* a source of vali_jpeg_encode_tensor only: the tensor forms above refuse it */ };
typedef struct vali_tensor_dst {
  void* data;               /* device memory, aligned to the element size */
  int32_t dtype;            /* enum vali_dtype */
  int32_t packed;           /* 0: planar, x stride 1.  1: channels last, c stride 1, x stride 3 */
  int32_t n, width, height; /* items, canvas size */
  int32_t reserved;
  int64_t stride_n, stride_c, stride_y; /* in ELEMENTS; stride_c is ignored when packed */
} vali_tensor_dst;                      /* 56 bytes */

VALI_API int vali_nv12_preproc_roi_tensor(const vali_surface* d_src, const vali_roi* d_roi,
                                          const vali_tensor_dst* dst, const vali_preproc_params* params, int pad,
                                          const uint8_t pad_rgb[3], vali_stream_t stream);
VALI_API int vali_rgb_preproc_roi_tensor(const vali_surface* d_src, const vali_roi* d_roi, int src_format,
                                         const vali_tensor_dst* dst, const vali_preproc_params* params, int pad,
                                         const uint8_t pad_rgb[3], vali_stream_t stream);

/* ---- JPEG: baseline sequential JFIF encoder ------------------------------------------------
 *
 * The reference's PyNvJpegEncoder (src/TC/src/TaskNvJpegEncode.cpp) on nvJPEG.  Definition (tests/jpeg_model.py
 * restates it; with no restart markers its entropy data is byte-identical to libjpeg's for the same pixels):
 *   - RGB, BGR, RGB_PLANAR: libjpeg's fixed-point rgb_ycc, coded 4:4:4 (vali_jpeg_params_init) or 4:2:2 / 4:2:0
 *     (vali_jpeg_params_init_sampled).  YUV444, YUV422, YUV420: the planes as they are (no colour conversion), coded
 *     with their own sampling.  Other formats: VALI_ERR_UNSUPPORTED.
 *   - RGB sources coded 4:2:2 / 4:2:0 are downsampled as libjpeg-turbo does by default (jcsample, no smoothing, no
 *     fancy downsampling), for any size (component size ceil(w / H) x ceil(h / V)).  Every full-resolution pixel is
 *     converted and truncated to 8 bits first; then
 *       4:2:0  c[y][x] = (p[2y][2x] + p[2y][2x+1] + p[2y+1][2x] + p[2y+1][2x+1] + bias) >> 2, bias 1 / 2 for even / odd x
 *       4:2:2  c[y][x] = (p[y][2x] + p[y][2x+1] + bias) >> 1,                                bias 0 / 1 for even / odd x
 *     The edges are not symmetric.  Horizontally the full-resolution row is replicated at its last pixel out to the
 *     edge of the chroma component's last real block: a chroma sample at x >= ceil(w / 2) is an average of replicated
 *     pixels with its own bias, not a copy of its neighbour.  Vertically the full-resolution image is replicated to a
 *     multiple of V rows only, and below ch = ceil(h / V) the downsampled rows are replicated.  In index form: chroma
 *     (x, y) reads columns min(2x, w-1), min(2x+1, w-1) and, with y' = min(y, ch-1), rows min(2y', h-1), min(2y'+1, h-1)
 *     at 4:2:0, row y' at 4:2:2.  Luma is coded as at 4:4:4.
 *   - the last column and row of every component are replicated out to its block edge; the dummy blocks of a
 *     partial MCU have zero AC and the DC of the block to their left (a dummy row: of the previous block of the
 *     same component in that MCU), as libjpeg's jccoefct;
 *   - level shift by 128, accurate integer FDCT (libjpeg "islow"), each coefficient / (8 q) rounded half away from
 *     zero; q from the Annex K tables scaled as jpeg_set_quality(quality, force_baseline = TRUE);
 *   - Huffman coding with the Annex K tables, a restart marker every restart_interval MCUs (DRI).
 * A file is vali_jpeg_header + the entropy data of vali_jpeg_encode_batch + EOI (FF D9).
 *
 * optimize = 1: every image is coded with Huffman tables built from its own symbol statistics, libjpeg's
 * optimize_coding (tests/jpeg_optimize_model.py restates it and is pinned to Pillow's optimize=True table for table
 * and byte for byte).  Nothing before entropy coding changes.  The counts are those of the symbols the scan codes: for
 * tables DC 0 (Y) and DC 1 (Cb and Cr together) the size category of every DC difference, prediction restarting with
 * every restart segment; for AC 0 and AC 1 every (run << 4 | size), ZRL and EOB; the dummy blocks of partial MCUs
 * included.  Each table is jpeg_gen_optimal_table of its counts: a pseudo-symbol 256 of count 1; merges of the two
 * least frequent entries (c1 the largest index among the minima, c2 the largest among the minima of the rest, the sum
 * stays at c1); code length = depth in the merge tree; lengths above 16 limited as Annex K.2 does; one code of the
 * longest length removed for the pseudo-symbol; HUFFVAL by length, then by value; codes as Annex C.  The counts fit 32
 * bits: an image's output slot is addressed with 32 bits, which caps it far below 2^32 symbols.
 * With optimize = 1 vali_jpeg_header writes only what does not depend on the pixels, SOI, APP0, DQT and SOF0, and the
 * device writes, in front of image i's entropy data at d_out + i * out_stride, one DHT segment with the image's four
 * tables (in the order 0x00, 0x10, 0x01, 0x11 of the plain header), DRI and SOS; d_sizes[i] counts all of it.  A file
 * is still vali_jpeg_header + the device's bytes + EOI.  vali_jpeg_stream_capacity grows by the worst case of that
 * prefix (440 bytes: a DHT of 4 + 4 * 17 + 12 + 12 + 162 + 162, DRI 6, SOS 14), vali_jpeg_workspace_size by each
 * image's four histograms, four code tables and DHT parts.  Any other value of optimize is VALI_ERR_INVALID_ARG from
 * every function that takes params; with optimize = 0 every function returns and writes what it always did.
 */
typedef struct vali_jpeg_params {
  int32_t quality;          /* 1..100 (clamped by vali_jpeg_params_init)                           */
  int32_t format;           /* enum vali_pixel_format of the source surfaces                       */
  int32_t h_samp, v_samp;   /* luma sampling factors: 1x1 (4:4:4), 2x1 (4:2:2), 2x2 (4:2:0)        */
  int32_t restart_interval; /* MCUs per restart segment: 1 .. 64 / blocks per MCU                  */
  int32_t optimize;         /* 0: the Annex K Huffman tables; 1: each image's own (below)            */
  int32_t reserved[2];
  uint8_t qtable[2][64];    /* quantisation tables in natural order: 0 luma, 1 both chroma, 1..255 */
} vali_jpeg_params;         /* 160 bytes */

/* host only: the parameters of `quality` (clamped to 1..100) for surfaces of `format`; restart_interval is the
 * largest that keeps a segment within 64 blocks (21 MCUs at 4:4:4, 16 at 4:2:2, 10 at 4:2:0) */
VALI_API int vali_jpeg_params_init(int quality, int format, vali_jpeg_params* out);
/* host only: as vali_jpeg_params_init, with the luma sampling h_samp x v_samp: 1x1, 2x1 or 2x2 for RGB, BGR and
 * RGB_PLANAR (chroma is downsampled as above); for a YUV format only its own.  Everything else is
 * VALI_ERR_INVALID_ARG; a format that cannot be encoded is VALI_ERR_UNSUPPORTED */
VALI_API int vali_jpeg_params_init_sampled(int quality, int format, int h_samp, int v_samp, vali_jpeg_params* out);
/* host only: SOI, APP0 (JFIF), DQT, SOF0, DHT, DRI, SOS of a width x height image (1..65535) into out[0..cap)
 * (optimize = 1: SOI, APP0, DQT, SOF0 only; the rest comes from the device with the entropy data),
 * its length in *len.  out == NULL asks for the length only; cap < length is VALI_ERR_INVALID_ARG (*len still set) */
VALI_API int vali_jpeg_header(int width, int height, const vali_jpeg_params* params, uint8_t* out, size_t cap,
                              size_t* len);
/* worst-case sizes: the device workspace of a batch of n images, and one image's output slot (no input can
 * overflow either: every segment is sized for its worst case of bits and byte stuffing) */
VALI_API int vali_jpeg_workspace_size(int n, int width, int height, const vali_jpeg_params* params, size_t* bytes);
VALI_API int vali_jpeg_stream_capacity(int width, int height, const vali_jpeg_params* params, size_t* bytes);
/*
 * Entropy-codes n (0..65535) images: d_src is a DEVICE array of n descriptors of `format` and width x height
 * (sizes as everywhere: YUV420 even width and height, YUV422 even width; an RGB source takes any size at any sampling).  Image i's entropy data, restart markers
 * included, header and EOI not, goes to d_out + i * out_stride (out_stride >= vali_jpeg_stream_capacity), its
 * length in bytes to d_sizes[i] (device memory).  workspace: ws_bytes >= vali_jpeg_workspace_size, device memory,
 * 256-byte aligned.  Four launches in stream order (optimize = 1: a memset of the histograms and six launches);
 * nothing is allocated and nothing synchronises, so the call can be captured into a graph.
 */
VALI_API int vali_jpeg_encode_batch(const vali_surface* d_src, int n, int width, int height, int format,
                                    const vali_jpeg_params* params, void* workspace, size_t ws_bytes, uint8_t* d_out,
                                    size_t out_stride, uint32_t* d_sizes, vali_stream_t stream);

/*
 * The same files straight from ONE batch tensor of logical shape (N, 3, H, W): float32, float16, bfloat16 or uint8,
 * addressed as vali_tensor_dst is (planar or channels last, strides in elements).  For item i, channel c and pixel
 * (x, y):
 *   e = element (i, c, y, x) as float32        exact for float16 (subnormals included), bfloat16 and uint8
 *   v = fl32(fl32(e * scale[c]) + offset[c])   two IEEE roundings, never a fused multiply-add
 *   p = 0 if v is NaN, else min(max(rint(v), 0), 255)      rint: round half to even; -inf -> 0, +inf -> 255
 * which is torch.nan_to_num(x.float() * scale + offset, nan=0.0).round().clamp(0, 255).to(torch.uint8) bit for bit.
 * The entropy data of item i is byte for byte what vali_jpeg_encode_batch writes for an 8-bit surface of
 * params->format that holds p, with the same params.  params->format names the channels:
 *   RGB, RGB_PLANAR: R, G, B;  BGR: B, G, R  -- coded 1x1, 2x1 or 2x2 as vali_jpeg_params_init_sampled allows;
 *   YUV444: Y, Cb, Cr, coded as they are, 1x1;  every other format: VALI_ERR_UNSUPPORTED.
 * The file never depends on the tensor's layout or dtype beyond p.  Any size, odd ones included, at every sampling.
 * Workspace, stream capacity and header: vali_jpeg_workspace_size, vali_jpeg_stream_capacity and vali_jpeg_header
 * of (src->n, src->width, src->height, params).  Output layout, d_sizes and the launches (params->optimize included:
 * everything after the first launch is shared) are those of vali_jpeg_encode_batch; src is a HOST struct that travels in the kernel arguments; nothing is allocated, nothing
 * synchronises.  VALI_ERR_INVALID_ARG, before any device is touched, for: null arguments; dtype outside 0..3 or
 * packed outside 0..1; n outside 1..65535; a size outside 1..65535; strides <= 0 or stride_y below the row's extent
 * (width, 3 * width when packed); data not aligned to its element; a non-finite scale or offset; and whatever
 * vali_jpeg_encode_batch refuses in params, workspace and out_stride.
 */
typedef struct vali_tensor_src {
  const void* data;         /* device memory, aligned to the element size */
  int32_t dtype;            /* enum vali_dtype, VALI_DTYPE_U8 included */
  int32_t packed;           /* 0: planar, x stride 1.  1: channels last, c stride 1, x stride 3 */
  int32_t n, width, height; /* items, image size */
  int32_t reserved;
  int64_t stride_n, stride_c, stride_y; /* in ELEMENTS; stride_c is ignored when packed */
} vali_tensor_src;                      /* 56 bytes: vali_tensor_dst with const data */

VALI_API int vali_jpeg_encode_tensor(const vali_tensor_src* src, const float scale[3], const float offset[3],
                                     const vali_jpeg_params* params, void* workspace, size_t ws_bytes,
                                     uint8_t* d_out, size_t out_stride, uint32_t* d_sizes, vali_stream_t stream);

/* ---- batch tensor -> video frames: the way back from a network's output ---------------------
 *
 * One (N, 3, H, W) tensor -> N 8-bit surfaces of W x H, one launch.  src: as vali_jpeg_encode_tensor takes it (HOST
 * struct, float32 / float16 / bfloat16 / uint8, planar or channels last, strides in elements).  d_dst: DEVICE array of
 * src->n descriptors of dst_format.  bgr: 0 = tensor channels are R, G, B; 1 = B, G, R.
 * For item i and pixel (x, y):
 *   p[c] = clamp(rint(fl32(fl32(e[c] * scale[c]) + offset[c])), 0, 255), NaN -> 0, ties to even, never a fused
 *          multiply-add: the words, and the code, of vali_jpeg_encode_tensor; scale and offset belong to TENSOR channel
 *          c; R, G, B are then named by bgr.
 *   VALI_FMT_RGB, VALI_FMT_RGB_PLANAR   the bytes R, G, B; params may be NULL
 *   VALI_FMT_YUV444   o_k = fmaf(m[k][2], B, fmaf(m[k][1], G, fmaf(m[k][0], R, m[k][3]))), m = params->rgb2yuv; each
 *                     value is sat_u8(rint(o_k))
 *   VALI_FMT_YUV420   Y as above; chroma = sat_u8(rint(((o00 + o01) + (o10 + o11)) * 0.25f)) over the UN-ROUNDED values
 *                     of the 2 x 2 block, in exactly that association: byte for byte what vali_convert RGB -> YUV420
 *                     writes for an RGB surface that holds p
 *   VALI_FMT_NV12     the YUV420 values with U and V interleaved in plane 1
 * NV12 and YUV420 need even W and H; the others take any size, 1 x 1 included.  The destinations may be pitched and may
 * be views at any address and pitch: misaligned ones take a slower store path with the same bytes.  Only the W x H
 * image area of each plane is written.
 * VALI_ERR_INVALID_ARG, before any device is touched, for: null src, scale, offset or d_dst; null params with a YUV
 * destination; everything vali_jpeg_encode_tensor refuses in src, scale and offset; bgr outside 0..1; an odd size for a
 * 4:2:0 destination.  VALI_ERR_UNSUPPORTED for every other dst_format.  Nothing is allocated and nothing synchronises,
 * so the call can be captured into a graph.
 *
 * The BT.709 matrices python_vali's PySurfacePostprocessor passes (this project's own definition: the reference has no
 * RGB -> YUV call for BT.709).  Kr = 0.2126, Kb = 0.0722, Kg = 1 - Kr - Kb; full range Y (Kr, Kg, Kb, 0),
 * Cb (-Kr / (2 (1 - Kb)), -Kg / (2 (1 - Kb)), 0.5, 128), Cr (0.5, -Kg / (2 (1 - Kr)), -Kb / (2 (1 - Kr)), 128); MPEG
 * range: the Y row x 219 / 255 with offset 16, the chroma rows x 224 / 255 with offset 128.  Each constant is computed
 * in double and rounded to float32 once:
 *   full range   Y   0.2125999927520752    0.7152000069618225    0.0722000002861023      0
 *                Cb -0.11457210779190063  -0.38542789220809937   0.5                   128
 *                Cr  0.5                  -0.454152911901474    -0.0458470918238163    128
 *   MPEG range   Y   0.18258588016033173   0.6142305731773376    0.062007058411836624   16
 *                Cb -0.10064373165369034  -0.3385719656944275    0.43921568989753723   128
 *                Cr  0.43921568989753723  -0.39894217252731323  -0.040273524820804596  128
 */
VALI_API int vali_tensor_to_surfaces(const vali_tensor_src* src, const float scale[3], const float offset[3], int bgr,
                                     const vali_surface* d_dst, int dst_format, const vali_cvt_params* params,
                                     vali_stream_t stream);

/* ---- marks on frames: outlines, fills and pixelation from a device-held list ---------------
 *
 * m marks are drawn IN PLACE onto n frames of one format (NV12, YUV420, YUV444, RGB, BGR, RGB_PLANAR; any sizes, 4:2:0
 * even) in TWO launches, whatever m and the data.  d_marks is DEVICE memory (4-byte aligned): a detector's output is
 * drawn without a device-to-host copy.  Marks are applied in row order; the result is what applying them one after the
 * other gives.  A row is SKIPPED when kind is VALI_MARK_NONE or unknown, frame is outside 0..n-1, w < 1 or h < 1, arg
 * is invalid for its kind or the rectangle does not meet its frame; every int32 value of x, y, w, h is handled
 * (intersections are formed in 64 bits).
 *   colour   a << 24 | r << 16 | g << 8 | b.  A sample's colour value c is r, g or b by name for RGB, BGR, RGB_PLANAR;
 *            for the YUV formats sat_u8(rint(fmaf(m[k][2], b, fmaf(m[k][1], g, fmaf(m[k][0], r, m[k][3]))))), k = Y, U,
 *            V, m = params->rgb2yuv: what vali_tensor_to_surfaces writes into YUV444 for that pixel
 *   NV12, YUV420   first x0 = x & ~1, y0 = y & ~1, x1 = (x + w + 1) & ~1, y1 = (y + h + 1) & ~1 and a BOX thickness is
 *            rounded up to even: a chroma sample is painted exactly when its four luma pixels are
 *   VALI_MARK_FILL      every sample of every plane in rectangle ^ frame: v = (v * (255 - a) + c * a + 127) / 255
 *   VALI_MARK_BOX       arg = thickness t >= 1: the same blend for the pixels of the UNCLIPPED rectangle outside its
 *                       inner rectangle [x0 + t, x1 - t) x [y0 + t, y1 - t), then clipped to the frame
 *   VALI_MARK_PIXELATE  arg = cell s in {4, 8, 16, 32}; the rectangle grows outward to the frame's s-grid and is
 *                       clipped to the frame; per plane every sample of (cell ^ frame) becomes (sum + cnt / 2) / cnt
 *                       over the plane's samples in (cell ^ frame); 4:2:0 chroma planes use cells of s / 2
 * Only samples inside the image area of a plane are written, and only those a mark changed; frames and tiles no
 * mark meets are neither read nor written.  frames is the HOST copy of the descriptors in d_frames (sizes and the
 * launch grid come from it).  workspace: vali_annotate_workspace_size bytes of device memory, 16-byte aligned; its
 * contents need not survive between calls.  Nothing is allocated and nothing synchronises, so the call can be captured
 * and replayed after d_marks was rewritten in place.  n = 0 or m = 0: success, nothing is launched.
 * VALI_ERR_INVALID_ARG, before any device is touched: null arguments (frames and d_frames with n > 0, d_marks with
 * m > 0, params for a YUV format, workspace with n > 0); n outside 0..65535; m outside 0..4096; a frame with a null
 * plane, a size outside 1..65535, an odd size in a 4:2:0 format, a pitch shorter than a row or a format other than
 * `format`; a workspace that is too small or not 16-byte aligned.  VALI_ERR_UNSUPPORTED for a format outside the list.
 *
 * Stamps (vali_annotate_batch_atlas): labels, logos and ready-made masks from a COVERAGE ATLAS, one 8-bit plane
 * (VALI_FMT_Y) in device memory, AW x AH with both in 1..65535, at any address and pitch, given per call as a HOST
 * vali_surface that travels in the kernel arguments.
 *   VALI_MARK_STAMP     arg = the stamp's origin in the atlas, u = arg & 0xffff, v = (arg >> 16) & 0xffff; w x h is its
 *                       size on the frame and in the atlas (1:1, no resampling).  With dx = px - x, dy = py - y (64 bits)
 *                       the coverage of frame pixel (px, py) is cov = atlas[v + dy][u + dx] if 0 <= dx < w, 0 <= dy < h,
 *                       u + dx < AW and v + dy < AH, else 0: a rectangle that runs off the atlas reads as zero there, and
 *                       no byte outside the atlas's AW x AH area is ever read.  The weight k of a sample is cov(px, py)
 *                       for full-resolution channels and (cov(2cx, 2cy) + cov(2cx + 1, 2cy) + cov(2cx, 2cy + 1) +
 *                       cov(2cx + 1, 2cy + 1) + 2) >> 2 for the 4:2:0 chroma sample (cx, cy); a STAMP rectangle is NOT
 *                       snapped to even coordinates.  With a the colour's alpha, a_eff = (k * a + 127) / 255 and
 *                       v = (v * (255 - a_eff) + c * a_eff + 127) / 255, c as for FILL: k = 255 is FILL's sample bit
 *                       for bit, k = 0 leaves the sample as it is (and unwritten).
 * A STAMP row is skipped when the call has no atlas (the kind is then unknown), w < 1 or h < 1, u >= AW or v >= AH, the
 * frame is outside the batch or the rectangle does not meet its frame.  Stamps are applied in row order among the other
 * kinds.  atlas may be NULL: the call is then vali_annotate_batch, and vali_annotate_batch is that call.  In addition
 * VALI_ERR_INVALID_ARG, before any device is touched, for an atlas that is not VALI_FMT_Y, has a null plane, a size outside
 * 1..65535 or a pitch shorter than a row.  The workspace, the two launches and every other rule are unchanged.
 */
#define VALI_MARK_NONE 0
#define VALI_MARK_BOX 1
#define VALI_MARK_FILL 2
#define VALI_MARK_PIXELATE 3
#define VALI_MARK_STAMP 4
#define VALI_MAX_MARKS 4096
typedef struct vali_mark {
  int32_t frame, x, y, w, h, kind, arg, colour;
} vali_mark; /* 32 bytes */

VALI_API int vali_annotate_workspace_size(int n, const vali_surface* frames, size_t* bytes);
VALI_API int vali_annotate_batch(const vali_surface* frames, const vali_surface* d_frames, int n, int format,
                                 const vali_mark* d_marks, int m, const vali_cvt_params* params, void* workspace,
                                 size_t ws_bytes, vali_stream_t stream);
VALI_API int vali_annotate_batch_atlas(const vali_surface* frames, const vali_surface* d_frames, int n, int format,
                                       const vali_mark* d_marks, int m, const vali_surface* atlas,
                                       const vali_cvt_params* params, void* workspace, size_t ws_bytes,
                                       vali_stream_t stream);

/* ---- detections: a detector's raw head into device-held boxes in frame pixels ---------------
 *
 * boxes (n, k, 4) and scores (n, k, c), float32, float16 or bfloat16 each, with any element strides >= 0 (a transposed
 * head, a broadcast), in the coordinates of the network's input; d_rects[i] is the record vali_*_preproc_roi_tensor
 * placed frame i with.  The call issues FOUR launches whatever the data, allocates nothing and never synchronises: it
 * can be captured and replayed after boxes, scores and d_rects were rewritten in place.  The reference has no such task.
 * All arithmetic is IEEE float32, one rounding per operation, never a fused multiply-add; (float) of an integer rounds
 * to nearest; sums of two int32 are formed in 64 bits.  Per frame i, with T = max_candidates and D = max_det:
 *   1. record   src_w, src_h, dst_w or dst_h below 1: the frame has no detections.
 *   2. score    s = -inf, cls = 0; for c = 0..C-1, v = (float)scores[i][k][c]: if v > s then s = v, cls = c (the lowest
 *               class wins ties, NaN never wins).  Candidate k passes when s > score_thr.
 *   3. box      (float) of the four values; VALI_DETECT_CXCYWH: x1 = cx - w * 0.5f, x2 = cx + w * 0.5f, y likewise.
 *               Clipped to the placement: x1 = dst_x > x1 ? dst_x : x1, x2 = dst_x + dst_w < x2 ? dst_x + dst_w : x2, y
 *               likewise (a NaN stays a NaN).  Dropped unless all four are finite and x2 > x1 && y2 > y1.
 *   4. order    by s descending as floats (-0.0 equals 0.0), equal scores by k ascending; the first T go on, exactly.
 *   5. NMS      greedy in that order: j is suppressed by a KEPT earlier i when (class_agnostic || cls_i == cls_j) and
 *               inter > iou_thr * uni, with iw = max(min(x2i, x2j) - max(x1i, x1j), 0), ih likewise, inter = iw * ih,
 *               a = (x2 - x1) * (y2 - y1), uni = (a_i + a_j) - inter: no division.  A suppressed candidate suppresses
 *               nothing.  The first D kept are the frame's detections, counts[i] their number.
 *   6. pixels   sx = (float)src_w / (float)dst_w, sy likewise; X1 = floor((x1 - dst_x) * sx + src_x), X2 = ceil((x2 -
 *               dst_x) * sx + src_x), the multiply and the add rounded separately, Y likewise; clamped to [src_x, src_x +
 *               src_w] and [src_y, src_y + src_h]; x = X1, w = max(X2 - X1, 1), y and h likewise (the maximum only
 *               matters where float32 cannot tell the two edges apart); values beyond int32 saturate.
 * Outputs, int32 rows of 8, each NULL or a device array that is rewritten in full by every call:
 *   dets   (n * D) rows; row i * D + r is detection r of frame i: frame, x, y, w, h, class, the score's float32 bits, k.
 *          An unused row is -1, 0, 0, 0, 0, 0, 0, 0.
 *   counts n values.
 *   rois   (n * D) rows x, y, w, h, crop[0..3]: vali_roi records of second-stage crops whose item i * D + r has frame i as
 *          its source; an unused row is all zero (an empty item).
 *   marks  R * n * D vali_mark rows, R = 3 with label_rects and 1 without, R * n * D <= VALI_MAX_MARKS.  Row i * D + r:
 *          frame, x, y, w, h, VALI_MARK_BOX, thickness, colours[class % n_colours].  With (u, v, lw, lh) =
 *          label_rects[class], row n * D + i * D + r: frame, x, y - lh, lw, lh, VALI_MARK_FILL, 0, that colour with its
 *          alpha replaced by label_alpha; row 2 * n * D + i * D + r: frame, x, y - lh, lw, lh, VALI_MARK_STAMP,
 *          u | v << 16, text_colour.  Rows of an unused detection, and the label rows of a class >= n_labels, are all zero.
 * workspace: vali_detect_workspace_size(n, k, max_candidates) bytes of device memory, 16-byte aligned (0 for sizes outside
 * the limits); its contents need not survive between calls.
 * VALI_ERR_INVALID_ARG, before any device is touched: null in, params, d_rects, out or workspace; a null tensor pointer, a
 * dtype outside the three, a pointer not aligned to its element, a stride outside 0..2^40; n outside 1..1024, k outside
 * 1..2^20, c outside 1..4096, max_candidates outside 1..1024, max_det outside 1..max_candidates, n * max_det > 65535; a
 * score_thr or iou_thr that is not finite; an unknown box_format; a workspace that is too small or misaligned; marks
 * without colours (or n_colours < 1), with more than 4096 rows, a thickness below 1 or a label_alpha outside 0..255.
 */
#define VALI_DETECT_XYXY 0
#define VALI_DETECT_CXCYWH 1
typedef struct vali_detect_tensor {
  const void* data;                      /* element (0, 0, 0) */
  int32_t dtype;                         /* VALI_DTYPE_F32, _F16 or _BF16 */
  int32_t reserved;
  int64_t stride_n, stride_k, stride_c;  /* in elements, >= 0 */
} vali_detect_tensor;                    /* 40 bytes */
typedef struct vali_detect_in {
  vali_detect_tensor boxes, scores;      /* (n, k, 4) and (n, k, c) */
  int32_t n, k, c, reserved;
} vali_detect_in;                        /* 96 bytes */
typedef struct vali_detect_params {
  int32_t max_candidates, max_det;
  float score_thr, iou_thr;
  int32_t class_agnostic, box_format;
  int32_t crop[4];                       /* rois: the placement px, py, pw, ph of every row */
  int32_t thickness, label_alpha, text_colour, n_colours, n_labels;  /* marks */
} vali_detect_params;                    /* 60 bytes */
typedef struct vali_detect_out {
  int32_t *dets, *counts, *rois, *marks; /* device memory; each may be NULL */
  const int32_t* colours;                /* device, n_colours packed colours (marks) */
  const int32_t* label_rects;            /* device, n_labels rows u, v, w, h, or NULL (marks) */
} vali_detect_out;                       /* 48 bytes */

VALI_API size_t vali_detect_workspace_size(int n, int k, int max_candidates);
VALI_API int vali_detect_select(const vali_detect_in* in, const vali_detect_params* params, const vali_roi* d_rects,
                                const vali_detect_out* out, void* d_ws, size_t ws_bytes, vali_stream_t stream);

/* ---- instance masks: a segmentation head's prototypes and coefficients painted onto frames ---------------
 *
 * protos (n, m, hp, wp) and coeffs (n, k, m), float32, float16 or bfloat16 each (protos: x stride 1, the n, m and y
 * strides any values >= 0; coeffs: any element strides >= 0), d_dets the (n * D) rows of vali_detect_select (frame, x, y,
 * w, h, class, score bits, k; D = max_det) and d_rects[i] the record frame i was placed with.  The masks of the rows are
 * blended IN PLACE onto n frames of one format (the six of vali_annotate_batch, under its rules for frames) in TWO
 * launches whatever the data; nothing is allocated and nothing synchronises, so the call can be captured and replayed
 * after protos, coeffs, d_dets, d_rects and the frames were rewritten in place.  The reference has no such task.
 * All arithmetic is IEEE float32, one rounding per operation, never a fused multiply-add; (float) of an integer rounds
 * to nearest.  Frame i is W x H with record src_x, src_y, src_w, src_h, dst_x, dst_y, dst_w, dst_h; row i * D + r:
 *   1. skipped  when its frame field is not i, w < 1 or h < 1, k is outside 0..K-1, src_w, src_h, dst_w or dst_h is below
 *               1, or the box [x, x + w) x [y, y + h) does not meet the frame.  Every int32 value is handled;
 *               intersections are formed in 64 bits.
 *   2. logits   for every prototype pixel acc = 0; for j = 0..m-1: acc = acc + (float)coeffs[i][k][j] *
 *               (float)protos[i][j][yp][xp], the product and the sum rounded separately, in this order: L[yp][xp].
 *   3. sample   of frame pixel px: g = (((float)px + 0.5f) - (float)src_x) * ((float)dst_w / (float)src_w) + (float)dst_x,
 *               fx = g * ((float)wp / (float)net_w) - 0.5f, x0 = floorf(fx), tx = fx - x0; x0 is clamped to [-1, wp] as
 *               a float and converted; ix0 = clamp(x0, 0, wp - 1), ix1 = clamp(x0 + 1, 0, wp - 1) (edge replication).
 *               y likewise with src_y, dst_h / src_h, dst_y, hp / net_h: iy0, iy1, ty.
 *   4. inside   top = L[iy0][ix0] + tx * (L[iy0][ix1] - L[iy0][ix0]), bot the same on row iy1, v = top + ty * (bot - top):
 *               the pixel is in the mask when v > 0 (a NaN is never in): the logits are upsampled, then compared.
 *   5. extent   only frame pixels inside box ^ frame can be in the mask; the box is NOT snapped on 4:2:0 frames.
 *   6. blend    VALI_MARK_STAMP's with coverage 255 inside the mask and 0 outside: k = cov for full-resolution channels,
 *               (the four luma coverages + 2) >> 2 for a 4:2:0 chroma sample, a_eff = (k * a + 127) / 255,
 *               v = (v * (255 - a_eff) + c * a_eff + 127) / 255, c as for VALI_MARK_FILL (params->rgb2yuv for YUV
 *               formats) of the colour d_colours[class mod n_colours] (the non-negative remainder), a its alpha or, with
 *               alpha in 0..255, alpha (alpha = -1 keeps the colour's).  Samples with k = 0 stay unwritten.
 *   7. order    the rows of a frame are applied in row order: the result is bit for bit that of
 *               vali_annotate_batch_atlas for STAMP rows over an atlas holding each mask as 255 / 0.  Nothing outside a
 *               plane's image area is written; frames and tiles no mask meets are neither read nor written.
 * Limits: n 1..1024, m 1..64, hp and wp 1..1024, k 1..2^20, D 1..1024 with n * D <= 65535, net_w and net_h 1..65535.
 * d_ws: vali_mask_workspace_size(n, max_det, hp, wp) = n * max_det * hp * wp * 4 bytes of device memory, 16-byte
 * aligned (0 for sizes outside the limits); row i * D + r has the hp x wp float32 slot r of frame i, of which only the
 * range its box can sample is written and read.  Its contents need not survive between calls.
 * VALI_ERR_INVALID_ARG, before any device is touched: null frames, d_frames, in, d_dets, d_rects, d_colours or d_ws, null
 * params for a YUV format; a null tensor pointer, a dtype outside the three, a pointer not aligned to its element, a stride
 * outside 0..2^40; a limit above broken; n_colours < 1; alpha outside -1..255; d_dets, d_rects or d_colours not 4-byte
 * aligned; a workspace that is too small or not 16-byte aligned; a frame that breaks vali_annotate_batch's rules.
 * VALI_ERR_UNSUPPORTED for a format outside the six.
 */
typedef struct vali_mask_tensor {
  const void* data;                      /* element (0, 0, 0, 0) */
  int32_t dtype;                         /* VALI_DTYPE_F32, _F16 or _BF16 */
  int32_t reserved;
  int64_t stride_n, stride_m, stride_y;  /* in elements, >= 0; the x stride is 1 */
} vali_mask_tensor;                      /* 40 bytes */
typedef struct vali_mask_in {
  vali_mask_tensor protos;               /* (n, m, hp, wp) */
  vali_detect_tensor coeffs;             /* (n, k, m) */
  int32_t m, hp, wp, k;
  int32_t max_det, net_w, net_h, reserved;
} vali_mask_in;                          /* 112 bytes */

VALI_API size_t vali_mask_workspace_size(int n, int max_det, int hp, int wp);
VALI_API int vali_mask_paint(const vali_surface* frames, const vali_surface* d_frames, int n, int format,
                             const vali_mask_in* in, const int32_t* d_dets, const vali_roi* d_rects,
                             const int32_t* d_colours, int n_colours, int alpha, const vali_cvt_params* params,
                             void* d_ws, size_t ws_bytes, vali_stream_t stream);

/* ---- semantic maps: a segmentation head's class logits as a class map per frame, tinted onto the frames ---------------
 *
 * logits (n, c, hs, ws), float32, float16 or bfloat16 (x stride 1, the n, c and y strides any values >= 0: a broadcast, a
 * slice of a larger head) and d_rects[i] the record frame i was placed with.  Every frame pixel inside the record's source
 * rectangle gets the class whose bilinearly upsampled logit is largest; the classes are written to label surfaces and / or
 * blended IN PLACE onto n frames of one format (the six of vali_annotate_batch, under its rules for frames) in ONE launch
 * whatever the data; nothing is allocated and nothing synchronises, so the call can be captured and replayed after logits,
 * d_rects, d_colours and the frames were rewritten in place.  The reference has no such task.
 * All arithmetic is IEEE float32, one rounding per operation, never a fused multiply-add; (float) of an integer rounds
 * to nearest.  Frame i is W x H with record src_x, src_y, src_w, src_h, dst_x, dst_y, dst_w, dst_h:
 *   1. skipped  a record with src_w, src_h, dst_w or dst_h below 1 paints nothing on its frame; its label surface becomes
 *               all 255.
 *   2. region   only frame pixels inside frame ^ [src_x, src_x + src_w) x [src_y, src_y + src_h) are classified: the
 *               intersection is formed in 64 bits, every int32 value is handled, and the region is NOT snapped to even
 *               coordinates.  Every other pixel is left as it is and has label 255.
 *   3. sample   steps 3 and 4 of vali_mask_paint with ws / net_w and hs / net_h in place of wp / net_w and hp / net_h,
 *               on the plane L = (float)logits[i][c]: v_c for every class c.
 *   4. label    c >= 2: best = -inf, label = 0; for c ascending: if v_c > best then best = v_c, label = c (the lowest
 *               class wins ties, a NaN never wins, all NaN or all -inf gives 0).  c = 1, a binary head: label = v_0 > 0 ?
 *               1 : 0, so there are two classes.
 *   5. blend    bit for bit what vali_annotate_batch_atlas gives for one VALI_MARK_STAMP row per class, in ascending
 *               class order, over an atlas holding each class's mask as 255 / 0, in the colour d_colours[class mod
 *               n_colours], a its alpha or, with alpha in 0..255, alpha (alpha = -1 keeps the colour's).  A
 *               full-resolution sample has exactly one class: one blend with k = 255.  A 4:2:0 chroma sample blends the
 *               classes present among its four luma pixels in ascending order, each with k = (255 * count + 2) >> 2;
 *               pixels outside the region count for no class.  a_eff, the rounding and the YUV colour of an RGB triple
 *               (params->rgb2yuv) are STAMP's.  Samples whose value does not change are not stored; nothing outside a
 *               plane's image area is written; a tile no region pixel meets is not read.
 *   6. labels   labels[i][y][x] = the label, or 255 outside the region: every pixel of every label surface is rewritten
 *               by every call.
 * Limits: n 1..1024, c 1..255, hs and ws 1..4096, net_w and net_h 1..65535.
 * labels / d_labels: both NULL, or the host copy and the device array of n descriptors of VALI_FMT_Y surfaces, labels[i] of
 * the size of frames[i], at any address and pitch.  d_colours NULL: nothing is painted, only the labels are written.
 * VALI_ERR_INVALID_ARG, before any device is touched: null frames, d_frames, in or d_rects, only one of labels and d_labels,
 * neither d_labels nor d_colours, null params for a YUV format that is painted; a null tensor pointer, a dtype outside the
 * three, a pointer not aligned to its element, a stride outside 0..2^40; a limit above broken; n_colours < 1 with
 * d_colours; alpha outside -1..255; d_rects or d_colours not 4-byte aligned; a frame that breaks vali_annotate_batch's
 * rules; a label surface whose format is not Y, whose size differs from its frame's, with a null plane or a pitch shorter
 * than a row.  VALI_ERR_UNSUPPORTED for a format outside the six.
 */
typedef struct vali_semantic_in {
  vali_mask_tensor logits;               /* the (n, c, hs, ws) tensor; strides read as n, c, y */
  int32_t c, hs, ws, net_w, net_h, reserved;
} vali_semantic_in;                      /* 64 bytes */

VALI_API int vali_semantic_paint(const vali_surface* frames, const vali_surface* d_frames, int n, int format,
                                 const vali_semantic_in* in, const vali_roi* d_rects, const vali_surface* labels,
                                 const vali_surface* d_labels, const int32_t* d_colours, int n_colours, int alpha,
                                 const vali_cvt_params* params, vali_stream_t stream);

/* ---- pose skeletons: a keypoint head's points in frame pixels, drawn as limbs and joints ---------------
 *
 * kpts (n, k, p, kdim), float32, float16 or bfloat16 with any four element strides >= 0 (a transposed, unflattened head
 * slice, a broadcast): (kx, ky, conf) per keypoint in the coordinates of the network's input with kdim = 3, (kx, ky) and
 * conf = 1.0 with kdim = 2.  d_dets are the (n * D) rows of vali_detect_select (frame, x, y, w, h, class, score bits, k;
 * D = max_det), d_rects[i] the record frame i was placed with, d_limbs n_limbs pairs (a, b) of keypoint indices in device
 * memory.  The keypoints of the rows are written to `points` and drawn IN PLACE onto n frames of one format (the six of
 * vali_annotate_batch, under its rules for frames) in TWO launches whatever the data; nothing is allocated and nothing
 * synchronises, so the call can be captured and replayed after kpts, d_dets, d_rects and the frames were rewritten in
 * place.  The reference has no such task.  Float arithmetic is IEEE float32, one rounding per operation, never a fused
 * multiply-add; (float) of an integer rounds to nearest.  Frame i is W x H with record src_x, src_y, src_w, src_h, dst_x,
 * dst_y, dst_w, dst_h; row i * D + r:
 *   1. skipped  exactly as a row of vali_mask_paint (its step 1), for every int32 value: its frame field is not i, w < 1
 *               or h < 1, k is outside 0..K-1, src_w, src_h, dst_w or dst_h is below 1, or the box [x, x + w) x
 *               [y, y + h) does not meet the frame.  The p points of a skipped row are all zero.
 *   2. mapping  keypoint j of a drawn row: (kx, ky, conf) = (float)kpts[i][k][j][0..2];
 *               fx = (kx - (float)dst_x) * ((float)src_w / (float)dst_w) + (float)src_x, fy likewise with dst_y, src_h /
 *               dst_h, src_y (vali_detect_select's step 6); X = floor(fx), Y = floor(fy).
 *   3. visible  when conf > kpt_thr (a NaN never is), kx and ky are finite, -65536 <= fx < 131072 and -65536 <= fy <
 *               131072 (tested on the floats, before the conversion).  A visible keypoint is inside the frame when
 *               0 <= X < W and 0 <= Y < H.  points[(i * D + r) * p + j] = X, Y, the bits of conf as float32, flag: flag 0
 *               invisible (X = Y = 0), 1 visible, 3 visible and inside the frame.
 *   4. coverage 255 or 0 per luma pixel, decided at the pixel's integer coordinates P in exact integers.  A joint of
 *               diameter d at C covers P when 4 |P - C|^2 <= d^2.  A limb of thickness t from A to B, with e = B - A,
 *               q = P - A, L2 = e . e, s = q . e: if L2 == 0 or s <= 0, when 4 |q|^2 <= t^2; else if s >= L2, when
 *               4 |P - B|^2 <= t^2; else when 4 c^2 <= t^2 L2 with c = q.x e.y - q.y e.x.  A capsule and a disc: no
 *               float, no square root, no anti-aliasing.  A limb is drawn when both its keypoints are visible, a joint
 *               when its keypoint is; a pair with an index outside 0..p-1 draws nothing.
 *   5. order    rows ascending; within a row the limbs in table order, then the joints by ascending keypoint.
 *   6. blend    VALI_MARK_STAMP's with that coverage: k = cov for full-resolution channels, (the four luma coverages + 2)
 *               >> 2 for a 4:2:0 chroma sample (shapes are NOT snapped to even coordinates), a_eff = (k * a + 127) / 255,
 *               v = (v * (255 - a_eff) + c * a_eff + 127) / 255, c as for VALI_MARK_FILL (params->rgb2yuv for YUV
 *               formats) of the colour d_limb_colours[l mod n_limb_colours] of limb l, d_joint_colours[j mod
 *               n_joint_colours] of joint j; a its alpha or, with alpha in 0..255, alpha (alpha = -1 keeps the colour's).
 *               The result is bit for bit that of vali_annotate_batch_atlas for STAMP rows, in that order, over an atlas
 *               holding each shape's coverage as 255 / 0.  Nothing outside a plane's image area is written; frames and
 *               tiles no shape meets are neither read nor written, and only 16-byte pieces a shape changed are stored.
 * Limits: n 1..1024, k 1..2^20, p 1..64, n_limbs 0..128, D 1..1024 with n * D <= 65535, thickness and diameter 1..64.
 * d_points: NULL, or n * D * p rows of 4 int32 in device memory, 16-byte aligned, every row rewritten by every call; with
 * NULL the rows go to the workspace.  d_ws: vali_pose_workspace_size(n, max_det, p) = n * max_det * (1 + p) * 16 bytes
 * of device memory, 16-byte aligned (0 for sizes outside the limits): a box per row, then the points.  Its contents need
 * not survive between calls.
 * VALI_ERR_INVALID_ARG, before any device is touched: null frames, d_frames, in, d_dets, d_rects, style or d_ws, null
 * params for a YUV format; a null kpts, d_limbs (with n_limbs > 0) or colour pointer, a dtype outside the three, a kpts
 * pointer not aligned to its element, a stride outside 0..2^40, kdim other than 2 or 3; a limit above broken; a colour
 * count below 1; a NaN kpt_thr; alpha outside -1..255; d_dets, d_rects, d_limbs or the colours not 4-byte aligned;
 * d_points or a workspace not 16-byte aligned, a workspace that is too small; a frame that breaks vali_annotate_batch's
 * rules.  VALI_ERR_UNSUPPORTED for a format outside the six.
 */
typedef struct vali_pose_in {
  const void* kpts;                      /* element (0, 0, 0, 0) */
  int32_t dtype;                         /* VALI_DTYPE_F32, _F16 or _BF16 */
  int32_t kdim;                          /* 3: (kx, ky, conf); 2: (kx, ky), conf = 1.0 */
  int64_t stride_n, stride_k, stride_p, stride_c; /* in elements, >= 0 */
  int32_t k, p, max_det, n_limbs;
  const int32_t* d_limbs;                /* device, n_limbs pairs (a, b) */
} vali_pose_in;                          /* 72 bytes */
typedef struct vali_pose_style {
  const int32_t* d_limb_colours;         /* device, n_limb_colours packed colours */
  const int32_t* d_joint_colours;        /* device, n_joint_colours packed colours */
  int32_t n_limb_colours, n_joint_colours;
  float kpt_thr;
  int32_t thickness, diameter, alpha;
} vali_pose_style;                       /* 40 bytes */

VALI_API size_t vali_pose_workspace_size(int n, int max_det, int p);
VALI_API int vali_pose_paint(const vali_surface* frames, const vali_surface* d_frames, int n, int format,
                             const vali_pose_in* in, const int32_t* d_dets, const vali_roi* d_rects,
                             const vali_pose_style* style, int32_t* d_points, const vali_cvt_params* params,
                             void* d_ws, size_t ws_bytes, vali_stream_t stream);

/* vali_pose_paint_points (TWO launches): steps 4 to 6 above for points the CALLER holds in device memory -- those of
 * vali_kpt_decode, an earlier vali_pose_paint, or anything computed on the GPU.  d_points: n * max_det * p rows of 4 int32
 * (X, Y, any value, flag), 16-byte aligned, read only; point j of row i * max_det + r is drawn on frame i.  A point is
 * visible when flag & 1 and -65536 <= X < 131072 and -65536 <= Y < 131072; the other bits of flag and every other int32
 * value are handled and draw nothing.  The first launch copies the visible points into the workspace and forms each row's
 * box as vali_pose_paint forms it from the points it computed; the second is vali_pose_paint's.  Frames, format, d_limbs,
 * style (its kpt_thr is not read), params, the workspace (vali_pose_workspace_size(n, max_det, p)) and the limits are
 * vali_pose_paint's, and so are the refusals that concern them.
 */
VALI_API int vali_pose_paint_points(const vali_surface* frames, const vali_surface* d_frames, int n, int format,
                                    const int32_t* d_points, int p, int max_det, const int32_t* d_limbs, int n_limbs,
                                    const vali_pose_style* style, const vali_cvt_params* params, void* d_ws,
                                    size_t ws_bytes, vali_stream_t stream);

/* ---- aligned crops: affine views of frames, from the caller's matrices or fitted to keypoints, into a batch tensor -----
 *
 * The second stage that needs a rotated or aligned crop: a face onto the 112 x 112 ArcFace canvas by its five landmarks,
 * a rotated rectangle (licence plate, scene text, oriented box) to an upright crop, any per-crop transform computed on
 * the GPU.  The reference has no such task.  Slot m of an (M, 3, h, w) tensor (vali_tensor_dst: float32, float16 or
 * bfloat16, planar or channels last, addressed as for vali_nv12_preproc_roi_tensor) is one affine view of one of n frames
 * of ONE format among NV12 (even sizes), RGB, BGR and RGB_PLANAR, of any sizes, addresses and pitches, read only.
 * d_matrices: M rows of 8 int32 in device memory, (frame, a, b, c, d, e, f, status), the six middle values float32 bit
 * patterns: the caller's, or vali_warp_fit's.  Nothing is allocated, nothing synchronises, no matrix, keypoint or box
 * reaches the host: both calls can be captured and replayed after the matrices, kpts, d_dets, d_rects and the frames were
 * rewritten in place.  Float arithmetic is IEEE float32, one rounding per operation, never a fused multiply-add unless
 * written fma(); (float) of an integer is exact here.
 * Coordinates: frame and canvas positions are continuous; pixel X covers [X, X + 1) and its centre is X + 0.5 (the
 * convention in which vali_pose_paint takes X = floor(fx)).
 *
 * vali_warp_tensor (ONE launch), slot m with its row and the W x H frame `frame`:
 *   1. skipped  when frame is outside 0..n-1: the canvas is all pad, or untouched with pad == 0; no frame is read.
 *   2. position canvas pixel (x, y): u = (float)x + 0.5f, v = (float)y + 0.5f, sx = ((a * u) + (b * v)) + c,
 *               sy = ((d * u) + (e * v)) + f, per pixel as written (never stepped from a neighbour).  The pixel is inside
 *               when 0 <= sx < W and 0 <= sy < H, tested on the floats: a NaN never is, and every float32 bit pattern in
 *               a row is handled.  A pixel that is not inside is pad, or is not written.
 *   3. taps     along x: g = sx - 0.5f, x0 = floor(g), t = g - x0, indices clamp(x0, 0, W - 1) and clamp(x0 + 1, 0,
 *               W - 1) (edge replication); along y likewise.  Per 8-bit channel top = p00 + tx * (p01 - p00), bot = p10 +
 *               tx * (p11 - p10), val = top + ty * (bot - top), q = round-half-even of val to 0..255.
 *   4. colour   RGB, BGR, RGB_PLANAR: q_R, q_G, q_B by name, as in vali_rgb_preproc_roi.  NV12: Y by step 3 on the luma
 *               plane; U and V independently on the (W / 2) x (H / 2) chroma plane at sx * 0.5f and sy * 0.5f in place of
 *               sx and sy (centre-sited chroma, the same tap rule); (q_Y, q_U, q_V) then becomes q_R, q_G, q_B by the
 *               YUV444 -> RGB arithmetic of vali_convert with yuv2rgb = params->csc (oracle/vali_oracle.c).
 *   5. element  out[m, c, y, x] = convert(dtype, ((q_c / 255.0f) / div - mean[c]) / std_[c]): step 3 and the convert of
 *               vali_nv12_preproc_roi_tensor, bit for bit.  The pad colour pad_rgb goes through the same step.
 * frames is the HOST copy of the n descriptors in d_frames (the rules are checked on it); dst and params are host structs
 * that travel in the kernel arguments; for the RGB family params->csc is ignored.
 * VALI_ERR_INVALID_ARG, before any device is touched: null frames, d_frames, d_matrices, dst or params; pad without a
 * colour; n outside 1..1024; a frame of another format than `format`, of a size outside 1..65535, of odd size (NV12),
 * with a null plane or a pitch shorter than a row; everything vali_rgb_preproc_roi_tensor refuses of dst (dst->n = M is
 * 1..65535); d_frames or d_matrices not 4-byte aligned; a canvas of more than 2^31 - 1 tiles.  VALI_ERR_UNSUPPORTED for a
 * format outside the four.
 *
 * vali_warp_fit (ONE launch) writes row i * D + r of d_matrices (16-byte aligned, n * D rows, every row rewritten by every
 * call) from row i * D + r of d_dets (vali_detect_select's, D = max_det), kpts (vali_pose_paint's, with its strides and
 * dtypes), the record d_rects[i] and d_template, p pairs (u, v) of float32 in canvas coordinates in device memory:
 *   1. skipped  exactly when vali_pose_paint skips the row (its step 1).  The row is then (-1, 0, 0, 0, 0, 0, 0, 0).
 *   2. used     keypoint j maps to (fx, fy) by step 2 of vali_pose_paint; it is used when it is visible by its step 3
 *               under kpt_thr and neither u_j nor v_j is a NaN (a template pair with a NaN takes no part: a 17-point head
 *               is aligned by its eyes alone).
 *   3. fit      over the used j in ascending order: n, Su, Sv, Sfx, Sfy; mu = Su / (float)n, mv, mx, my likewise; then
 *               with du = u - mu, dv = v - mv, dx = fx - mx, dy = fy - my: A += (du * dx) + (dv * dy), B += (du * dy) -
 *               (dv * dx), Dn += (du * du) + (dv * dv); al = A / Dn, be = B / Dn.  The row is
 *               (i, al, -be, mx - ((al * mu) - (be * mv)), be, al, my - ((be * mu) + (al * mv)), n):
 *               the least-squares similarity (rotation, uniform scale, shift, no reflection) that takes the template
 *               onto the keypoints; with two points it is exact.
 *   4. skipped  as in step 1 when n < min_points, Dn == 0, or al or be is not finite.
 * VALI_ERR_INVALID_ARG, before any device is touched: null d_frames, in, d_dets, d_rects, d_matrices, kpts or d_template;
 * n outside 1..1024, k outside 1..2^20, p outside 2..64, kdim other than 2 or 3, max_det outside 1..1024, n * max_det
 * above 65535, min_points outside 2..p; a dtype outside the three, a kpts pointer not aligned to its element, a stride
 * outside 0..2^40; a NaN kpt_thr; d_frames, d_dets, d_rects or d_template not 4-byte aligned, d_matrices not 16-byte
 * aligned.
 */
typedef struct vali_warp_fit_in {
  const void* kpts;                      /* element (0, 0, 0, 0) */
  int32_t dtype;                         /* VALI_DTYPE_F32, _F16 or _BF16 */
  int32_t kdim;                          /* 3: (kx, ky, conf); 2: (kx, ky), conf = 1.0 */
  int64_t stride_n, stride_k, stride_p, stride_c; /* in elements, >= 0 */
  int32_t k, p, max_det, min_points;
  const float* d_template;               /* device, p pairs (u, v) */
  float kpt_thr;
  int32_t reserved;
} vali_warp_fit_in;                      /* 80 bytes */

VALI_API int vali_warp_fit(const vali_surface* d_frames, int n, const vali_warp_fit_in* in, const int32_t* d_dets,
                           const vali_roi* d_rects, int32_t* d_matrices, vali_stream_t stream);
VALI_API int vali_warp_tensor(const vali_surface* frames, const vali_surface* d_frames, int n, int format,
                              const int32_t* d_matrices, const vali_tensor_dst* dst, const vali_preproc_params* params,
                              int pad, const uint8_t pad_rgb[3], vali_stream_t stream);

/* ---- keypoint decode: a second-stage network's heatmaps or SimCC vectors as points in frame pixels -------------------
 *
 * The way back from a top-down pose or landmark network (HRNet, ViTPose, RTMPose, face landmarks) that ran on the crops
 * of vali_warp_tensor or vali_nv12_preproc_roi_tensor: slot m of its output holds one map per keypoint j, and the map's
 * peak becomes a point of the FRAME the crop was cut from, through the row the crop was cut with.  ONE launch, nothing
 * allocated, nothing synchronises: the call can be captured and replayed after the tensors were rewritten in place.  The
 * reference has no such task.  Float arithmetic is IEEE float32, one rounding per operation, never a fused multiply-add;
 * (float) of an integer is exact here.  Where a step yields a NaN, which NaN (sign, payload) is not defined.
 * Inputs, float32, float16 or bfloat16 in device memory, aligned to their element only:
 *   form (a)  heat (m, p, hh, wh): x stride 1, the strides of m, p and y in elements, any values >= 0 (slices, pitched
 *             rows, a broadcast).
 *   form (b)  simcc_x (m, p, wx) and simcc_y (m, p, wy), last stride 1, the others >= 0; wx goes in `wh`, wy in `hh`.
 * Mapping, exactly one of: d_matrices, m rows (frame, a, b, c, d, e, f, status) as vali_warp_tensor reads them; d_rois, m
 * = n * max_det vali_roi records as vali_detect_select writes them (source rectangle in the frame, placement on the
 * canvas), slot i * max_det + r belonging to frame i.  canvas_w x canvas_h is the size the crops were cut to; d_frames
 * are the n frames' descriptors, read for their sizes only.  Slot m, keypoint j:
 *   1. skipped  matrices: frame is outside 0..n-1; rois: src_w, src_h, dst_w or dst_h is below 1.  The slot's rows of
 *               d_points and d_kpts are all zero and no map of it is read.  Every int32 value and every float32 bit
 *               pattern in a row is handled.
 *   2. peak     over the map's elements in row-major order, converted to float32: the lowest index among the elements
 *               that compare equal to the greatest non-NaN element (-0.0 equals 0.0; +-inf are ordinary values; a NaN
 *               never wins); conf is the element at that index, xp = index % wh, yp = index / wh.  A map of NaNs only has
 *               no peak: the points row is (0, 0, the bits 0x7fc00000, 0) and the kpts row (0, 0, NaN).  Form (b): xp is
 *               the peak of the x vector with value vx, yp that of the y vector with vy, conf = vy < vx ? vy : vx; no
 *               peak in either vector is no peak.
 *   3. refine   VALI_KPT_REFINE_QUARTER, form (a) only: if 0 < xp < wh - 1, d = heat[yp][xp + 1] - heat[yp][xp - 1] and
 *               ox = 0.25 when d > 0, -0.25 when d < 0; otherwise (a NaN, a border column) ox = 0.  oy likewise along y.
 *               VALI_KPT_REFINE_NONE and form (b): ox = oy = 0.
 *   4. canvas   sx = (float)canvas_w / (float)wh.  VALI_KPT_ALIGN_CENTRE: cu = (((float)xp + 0.5f) + ox) * sx;
 *               VALI_KPT_ALIGN_INDEX: cu = (((float)xp + ox) * sx) + 0.5f (codecs that label in pixel-index coordinates).
 *               cv likewise with canvas_h and hh.
 *   5. frame    matrices: fx = ((a * cu) + (b * cv)) + c, fy = ((d * cu) + (e * cv)) + f (vali_warp_tensor's step 2).
 *               rois: fx = (cu - (float)dst_x) * ((float)src_w / (float)dst_w) + (float)src_x, fy likewise
 *               (vali_pose_paint's step 2).
 *   6. visible  by vali_pose_paint's step 3 with (cu, cv) in the place of (kx, ky): conf > kpt_thr, -65536 <= fx < 131072
 *               and -65536 <= fy < 131072.  d_points[m * p + j] = X, Y, the bits of conf, flag exactly as there (flag 3:
 *               inside the W x H frame the slot belongs to); d_kpts[m * p + j] = fx, fy, conf whether visible or not.
 * d_points: m * p rows of 4 int32, 16-byte aligned; d_kpts: NULL or m * p rows of 3 float32.  Every row of both is
 * rewritten by every call.  Limits: n 1..1024, m 1..65535, p 1..64, hh and wh 1..4096, hh * wh <= 2^20 in form (a), the
 * canvas 1..65535 a side, max_det 1..1024.
 * VALI_ERR_INVALID_ARG, before any device is touched: null d_frames, in or d_points; both or neither of d_matrices and
 * d_rois; heat together with a SimCC vector, or neither heat nor both vectors; a dtype outside the three, a tensor not
 * aligned to its element, a stride outside 0..2^40; a limit above broken; with d_rois, m other than n * max_det; an
 * unknown refine or align, a refinement in form (b); a NaN kpt_thr; d_frames, d_matrices, d_rois or d_kpts not 4-byte
 * aligned, d_points not 16-byte aligned.
 */
#define VALI_KPT_REFINE_NONE 0
#define VALI_KPT_REFINE_QUARTER 1
#define VALI_KPT_ALIGN_CENTRE 0
#define VALI_KPT_ALIGN_INDEX 1
typedef struct vali_kpt_decode_in {
  const void* heat;                      /* form (a): element (0, 0, 0, 0); NULL: form (b) */
  const void* simcc_x;                   /* form (b): element (0, 0, 0) of each; NULL in form (a) */
  const void* simcc_y;
  int32_t dtype;                         /* VALI_DTYPE_F32, _F16 or _BF16 */
  int32_t refine, align;
  int32_t max_det;                       /* with d_rois */
  int64_t stride_m, stride_p, stride_y;  /* heat, in elements, >= 0 */
  int64_t x_stride_m, x_stride_p, y_stride_m, y_stride_p; /* the vectors */
  int32_t m, p, hh, wh;
  int32_t canvas_w, canvas_h;
  float kpt_thr;
  int32_t reserved;
} vali_kpt_decode_in;                    /* 128 bytes */

VALI_API int vali_kpt_decode(const vali_surface* d_frames, int n, const vali_kpt_decode_in* in,
                             const int32_t* d_matrices, const vali_roi* d_rois, int32_t* d_points, float* d_kpts,
                             vali_stream_t stream);

/* ---- tracks: vali_detect_select's rows associated over time with tracks held in device memory ---------------
 *
 * The temporal step after vali_detect_select: a greedy IoU tracker with a constant-velocity prediction whose whole
 * state is the caller's device array `tracks`.  ONE launch whatever the data, nothing allocated, nothing synchronises:
 * the call can be captured and replayed after dets was rewritten in place.  The reference has no such task.
 * The n = streams * frames frames of a call are `streams` independent streams of `frames` consecutive frames each: stream
 * s owns frames s * F .. s * F + F - 1 in time order (F = frames), rows s * T .. s * T + T - 1 of tracks (T = max_tracks)
 * and row s of clock.  frames = 1: n live cameras; streams = 1: one file decoded in batches.  With D = max_det:
 *   dets     n * D rows of 8 int32 as vali_detect_select writes them (frame, x, y, w, h, class, score bits, k); read only.
 *   tracks   streams * T rows of 16 int32, 16-byte aligned, read and rewritten by every call; all zero: no tracks.  A row:
 *            id, class, x, y, w, h, vx bits, vy bits (float32, pixels per frame), hits, misses, age, score bits, k, 0, 0, 0.
 *            A row is LIVE when id >= 1 && w >= 1 && h >= 1; any other row is free and is written back as zeros.  hits,
 *            misses and age are read clamped to 0..2^30; values 13..15 are written as 0.
 *   clock    streams rows of 4 int32: next_id, frames seen, 0, 0; all zero at the start.  A next_id below 1 reads as 1.
 * Every int32 value in dets, tracks and clock is handled.  All float arithmetic is IEEE float32 with one rounding per
 * operation, never a fused multiply-add; divisions are correctly rounded; (float) of an integer rounds to nearest;
 * min(p, d) is d < p ? d : p and max(p, d) is d > p ? d : p, so a NaN in p stays.  For stream s, for t = 0..F-1 in this
 * order, frame i = s * F + t:
 *   1. predict  per live track, g = (float)(misses + 1): px = (float)x + vx * g, py likewise; its box is [px, px +
 *               (float)w] x [py, py + (float)h], its area pa = (float)w * (float)h.
 *   2. rows     row i * D + r is VALID when its frame value is i, w >= 1 and h >= 1; its box is [(float)x, (float)x +
 *               (float)w] x [(float)y, (float)y + (float)h], its area da = (float)w * (float)h, its score the float32
 *               whose bits it carries.
 *   3. match    the valid rows in ascending r (vali_detect_select's order: score descending).  Candidates are the tracks
 *               that were live at step 1, are not yet matched in this frame and have the row's class (any class with
 *               class_agnostic), with iw = min(px1, dx1) - max(px0, dx0), ih likewise, iw > 0 && ih > 0, inter = iw * ih,
 *               uni = (pa + da) - inter, iou = inter / uni and iou > iou_thr (a NaN never passes).  The greatest iou
 *               wins, equal values go to the lowest slot.
 *   4. update   of the matched track, with the row's values x', y', w', h': step_x = ((float)((2x' + w') - (2x + w)) *
 *               0.5f) / g, the integer difference formed in 64 bits and converted once; vx = vx + momentum * (step_x -
 *               vx); y likewise.  The box, class, score bits and k become the row's; hits + 1, misses = 0, age + 1,
 *               saturating at 2^30.
 *   5. misses   every live track that no row matched: misses + 1, age + 1 (saturating); it is freed when misses >
 *               max_age, and when hits < min_hits (a tentative track dies on its first miss).
 *   6. births   the valid rows that matched nothing and have score >= new_thr (a NaN never passes), in ascending r, each
 *               take the lowest slot that is free after step 5: id = next_id, after which next_id + 1, and 1 after
 *               2^31 - 1; hits = 1, misses = 0, age = 1, vx = vy = 0, the rest the row's.  With no free slot the row
 *               stays untracked.  (A row below new_thr continues a track and never starts one.)
 * After the last frame clock[s] = next_id, frames seen + F (wrapping as a 32-bit integer), 0, 0.
 * Outputs, int32 device arrays, every row rewritten by every call:
 *   tracked  n * D rows of 8: row i * D + r is frame, x, y, w, h, id, score bits, k -- the dets row with its track's id
 *            where the class was -- when the row was matched or born and its track now has hits >= min_hits; every other
 *            row is -1, 0, 0, 0, 0, 0, 0, 0.  It goes wherever dets goes.
 *   assoc    NULL or n * D rows of 4: id, slot (0..T-1), hits, class of the track the row was matched to or started
 *            (tentative ones too); 0, -1, 0, 0 for every other row.
 *   marks    NULL or R * n * D vali_mark rows, R = 3 with label_rects and 1 without, R * n * D <= VALI_MAX_MARKS: the
 *            rows vali_detect_select writes, taken from the tracked row, with colours[id % n_colours] as the colour and
 *            label_rects[id % n_labels] as the label; the rows of an unused tracked row are all zero.
 * One call with F frames per stream equals F calls with one frame each on the same tracks and clock, bit for bit.
 * Limits: streams 1..1024, frames >= 1, n <= 1024, max_det 1..1024, n * max_det <= 65535, max_tracks 1..256.
 * VALI_ERR_INVALID_ARG, before any device is touched: null params or io; null dets, tracks, clock or tracked; a limit
 * above broken; tracks not 16-byte aligned, any other array not 4-byte aligned; an iou_thr or new_thr that is not finite,
 * a momentum outside 0..1, min_hits < 1, max_age outside 0..2^20; marks without colours (or n_colours < 1), with more
 * than 4096 rows, a thickness below 1, a label_alpha outside 0..255 or label_rects with n_labels < 1.
 */
typedef struct vali_track_params {
  int32_t streams, frames;               /* S and F; n = S * F */
  int32_t max_det, max_tracks;           /* D and T */
  float iou_thr, new_thr, momentum;
  int32_t min_hits, max_age, class_agnostic;
  int32_t thickness, label_alpha, text_colour, n_colours, n_labels;  /* marks */
  int32_t reserved;
} vali_track_params;                     /* 64 bytes */
typedef struct vali_track_io {
  const int32_t* dets;                   /* device memory throughout */
  int32_t *tracks, *clock;               /* the state */
  int32_t *tracked, *assoc, *marks;      /* assoc and marks may be NULL */
  const int32_t* colours;                /* n_colours packed colours (marks) */
  const int32_t* label_rects;            /* n_labels rows u, v, w, h, or NULL (marks) */
} vali_track_io;                         /* 64 bytes */

VALI_API int vali_track_update(const vali_track_params* params, const vali_track_io* io, vali_stream_t stream);

/*
 * Rectangles of surfaces of ANY sizes as files, in one fixed set of launches.  Item i is rectangle rois[i] of the
 * surface d_src[i] (the same surface may stand behind any number of items); its file is byte for byte the file of
 * vali_jpeg_encode_batch for a surface that holds a copy of the rectangle: the component's last column and row are
 * replicated at the RECTANGLE's edge, and no sample outside it is read.  Rules (vali_jpeg_plan_rois checks them, with
 * the item and the rule in vali_last_error()): the rectangle lies inside its surface and is 1..65535 on a side;
 * YUV420 sources need even x, y, width, height, YUV422 even x, width; RGB, BGR, RGB_PLANAR and YUV444 take any
 * integers at every sampling.  The rectangles are host data: an image's header and its place in the output depend on
 * its size.
 *
 * vali_jpeg_plan_rois (host only) turns the rectangles into one record per item with everything the kernels look up:
 * its geometry, where its coefficients, segments and output start, and its first workgroup in each launch (the grids
 * are one-dimensional over the sum of the items' workgroups, each item padded to whole workgroups; a workgroup finds
 * its item by a binary search of these fields).  The caller copies the records to the device and passes both copies
 * to vali_jpeg_encode_rois, as vali_jpeg_decode_batch takes infos and d_infos.
 */
typedef struct vali_jpeg_roi {
  int32_t x, y, width, height; /* pixels of the surface's full-resolution grid */
} vali_jpeg_roi;               /* 16 bytes */

typedef struct vali_jpeg_item {
  int32_t x, y, width, height;        /* the rectangle                                                           */
  int32_t mcux, mcuy;                 /* MCUs per row / per column                                               */
  int32_t nblocks, nseg;              /* blocks (dummy blocks of partial MCUs included) and restart segments     */
  int32_t cw[3], ch[3], bw[3], bh[3]; /* component size in samples / real blocks                                 */
  uint32_t wg_fdct;                   /* first workgroup in k_jpeg_fdct: 256 blocks each, or whole MCUs          */
  uint32_t wg_hist;                   /* ... in k_jpeg_hist: 16 segments each                                    */
  uint32_t wg_seg;                    /* ... in k_jpeg_huff and k_jpeg_assemble: one segment each (= seg_first)  */
  uint32_t check;                     /* ties the record to the params it was planned for                       */
  uint64_t block_first;               /* coefficients: workspace + block_first * 128                             */
  uint64_t seg_first;                 /* segment lengths and offsets: entry seg_first; slots: seg_first * slot   */
  uint64_t out_offset;                /* the image's bytes: d_out + out_offset (vali_jpeg_stream_capacity apart) */
  uint64_t reserved;
} vali_jpeg_item;                     /* 128 bytes */

/* host only: checks n (0..65535) rectangles against their surfaces' sizes src_w[i] x src_h[i] and params, fills
 * items[0..n), *ws_bytes (the workspace of vali_jpeg_encode_rois) and *out_bytes (one output buffer that holds every
 * image's vali_jpeg_stream_capacity back to back).  One image's slot stays addressable with 32 bits; the offsets
 * between images are 64-bit.  n = 0: both sizes are 0.  VALI_ERR_INVALID_ARG for a broken rule, for what
 * vali_jpeg_workspace_size refuses in params and sizes, and for a batch whose flattened grids would pass 2^31 - 1
 * workgroups */
VALI_API int vali_jpeg_plan_rois(const vali_jpeg_roi* rois, const int32_t* src_w, const int32_t* src_h, int n,
                                 const vali_jpeg_params* params, vali_jpeg_item* items, size_t* ws_bytes,
                                 size_t* out_bytes);
/*
 * d_src: DEVICE array of n descriptors of params->format, item i's surface at [i].  items / d_items: the records of
 * vali_jpeg_plan_rois for these params, in host and in device memory.  Image i's bytes (entropy data, preceded with
 * optimize = 1 by its DHT, DRI and SOS) go to d_out + items[i].out_offset, their length to d_sizes[i]; the header is
 * vali_jpeg_header(items[i].width, items[i].height, params).  workspace: device memory, 256-byte aligned, ws_bytes >=
 * the plan's; out_bytes >= the plan's.  Four launches whatever n and the sizes (optimize = 1: a memset and six);
 * nothing is allocated and nothing synchronises, so the call can be captured into a graph.  VALI_ERR_INVALID_ARG,
 * before any device is touched, for null arguments, a short or misaligned workspace, a short output and items that
 * vali_jpeg_plan_rois did not make for these params.
 */
VALI_API int vali_jpeg_encode_rois(const vali_surface* d_src, const vali_jpeg_item* items,
                                   const vali_jpeg_item* d_items, int n, const vali_jpeg_params* params,
                                   void* workspace, size_t ws_bytes, uint8_t* d_out, size_t out_bytes,
                                   uint32_t* d_sizes, vali_stream_t stream);

/* ---- JPEG: baseline sequential decoder ----------------------------------------------------
 *
 * Definition: libjpeg-turbo's default decompression, bit for bit (tests/jpeg_decode_model.py restates it):
 *   - Huffman decoding; a DC prediction per component that restarts with every restart segment;
 *   - dequantisation, accurate integer IDCT (jidctint "islow"), the post-IDCT range-limit table of jdmaster
 *     including its wrap of out-of-range values (index & 1023);
 *   - RGB outputs: fancy upsampling of chroma (h2v1 / h2v2 triangle filters when the chroma width exceeds 2,
 *     replication otherwise; h1v2 triangle filter), rows replicated at the top and bottom of the image, then
 *     jdcolor's fixed-point ycc_rgb_convert.  Grayscale files give R = G = B = Y.
 * Supported input: SOF0, or SOF1 with 8-bit samples; Huffman coding; one interleaved scan of 1 or 3 components;
 * luma sampling (H, V) in {(1,1), (2,1), (1,2), (2,2)} with chroma 1x1; any restart interval; 8- or 16-bit DQT.
 * Everything else is VALI_ERR_UNSUPPORTED from vali_jpeg_parse, with the reason in vali_last_error().
 *
 * Corrupt entropy data fails the image (status != 0); it never makes a kernel read or write outside the call's
 * buffers.  Corrupt means: an invalid Huffman code, a run past coefficient 63, a code word that runs past the end
 * of its restart segment, a segment that ends before its last MCU, a byte 0xFF followed by anything but 0x00 or
 * the expected RSTn, or a number of RSTn markers other than (segments - 1).
 */
/* Huffman decode table of one component and class: a 9-bit lookahead plus maxcode / valoff for longer codes */
typedef struct vali_jpeg_huff {
  uint16_t look[512];  /* next 9 bits -> (code length << 8) | symbol; 0 = the code is longer than 9 bits        */
  int32_t maxcode[18]; /* largest code of length l (1..16), -1 when there is none; [0] and [17] unused          */
  int32_t valoff[18];  /* symbol index of code c of length l = c + valoff[l]                                   */
  uint8_t vals[256];   /* HUFFVAL                                                                              */
} vali_jpeg_huff;      /* 1424 bytes */

typedef struct vali_jpeg_info {
  int32_t width, height;
  int32_t components;       /* 1 (grayscale) or 3 (YCbCr)                                                   */
  int32_t h_samp, v_samp;   /* luma sampling factors (chroma is 1x1); 1x1 for grayscale                     */
  int32_t restart_interval; /* MCUs per restart segment from DRI; 0 = none                                  */
  int32_t mcux, mcuy;       /* MCUs per row / per column                                                    */
  int32_t blocks_per_mcu;   /* h_samp * v_samp + 2, or 1 for grayscale                                      */
  int32_t segments;         /* restart segments of the scan (1 without restart markers)                     */
  uint64_t data_offset;     /* first byte of the entropy-coded data: in the file (vali_jpeg_parse), in the
                               batch's data buffer (vali_jpeg_decode_batch -- the caller sets it)             */
  uint64_t data_len;        /* its length in bytes, restart markers included, up to the next other marker    */
  uint16_t qtable[3][64];   /* quantisation table of each component, natural order                         */
  vali_jpeg_huff dc[3], ac[3];
} vali_jpeg_info;           /* 8984 bytes */

/* host only: walks the markers of a whole file, checks them (an oversubscribed DHT and the all-ones code are
 * refused) and fills *out.  VALI_ERR_UNSUPPORTED for what the decoder does not cover, VALI_ERR_INVALID_ARG for a
 * malformed header; the reason is in vali_last_error() */
VALI_API int vali_jpeg_parse(const uint8_t* data, size_t len, vali_jpeg_info* out);
/* device workspace of a call on these n files, for every content of their entropy data */
VALI_API int vali_jpeg_decode_workspace_size(const vali_jpeg_info* infos, int n, size_t* bytes);
/*
 * Decodes n (0..65535) files of any sizes and samplings in one call.  infos: the files' infos in host memory;
 * d_infos: the same array in device memory.  d_data: device buffer holding every file's entropy-coded data at
 * its data_offset.  d_dst: DEVICE array of n destination descriptors of `format` and of each file's size:
 *   VALI_FMT_RGB, VALI_FMT_BGR, VALI_FMT_RGB_PLANAR   any file;
 *   VALI_FMT_Y                                          any file: the luma component;
 *   VALI_FMT_YUV444 / YUV422 / YUV420 / NV12            files of exactly that sampling (4:2:x: even sizes): the
 *                                                       component planes cropped to the image, no resampling.
 * d_status[i] (device int32) = 0 when file i decoded, nonzero when its entropy data is corrupt or its descriptor
 * does not match its info; then nothing of it is written.  Only the image area of each destination is written.
 * workspace: ws_bytes >= vali_jpeg_decode_workspace_size, device memory, 256-byte aligned.  A fixed number of
 * launches per format, whatever n and the data; nothing is allocated and nothing synchronises, so the call can be
 * captured into a graph and replayed on new data of the same layout.
 */
VALI_API int vali_jpeg_decode_batch(const vali_jpeg_info* infos, const vali_jpeg_info* d_infos, int n,
                                    const uint8_t* d_data, int format, const vali_surface* d_dst, void* workspace,
                                    size_t ws_bytes, int32_t* d_status, vali_stream_t stream);

/* ---- UD: chroma upsample + resize (+ YUV->RGB) in one pass ---------------------- */

/*
 * Replaces the reference's first-party launchers UD_NV12 / UD_NV12_HBD
 * (reference: src/TC/inc/ResizeUtils.hpp:30-50, src/TC/src/ResizeUtils.cu:98-176; callers
 * src/TC/src/UDSurface.cpp:84-115).  src->format: NV12 or P10; dst->format one of
 * YUV444, RGB, RGB_PLANAR, RGB_32F, RGB_32F_PLANAR (NV12) / YUV444_10BIT, RGB_32F,
 * RGB_32F_PLANAR (P10) -- the semi-planar rows of UDSurface::SupportedConversions()
 * (UDSurface.cpp:117-133); anything else returns VALI_ERR_UNSUPPORTED.
 * As in the reference the dst size alone defines the scale (no size validation).
 */
VALI_API int vali_ud_nv12(const vali_surface* src, const vali_surface* dst,
                          vali_stream_t stream);
/* (the frames of a batch share one geometry: src_width x src_height -> dst_width x dst_height) */
VALI_API int vali_ud_nv12_batch(const vali_surface* d_src, const vali_surface* d_dst, int n,
                                int src_format, int src_width, int src_height, int dst_width, int dst_height,
                                int dst_format, vali_stream_t stream);

/*
 * UD with the result written rotated by `quarter_turns` x 90 degrees (1..3; 0 = vali_ud_nv12):
 * the fused form of the chain PySurfaceUD -> PySurfaceRotator (BASELINE config 4), bit-identical
 * to vali_ud_nv12 followed by vali_rotate with the canonical quarter-turn shifts
 * (PySurfaceRotator.cpp:47-73), without the intermediate surface.  NV12 -> RGB only.
 * `dst` is the ROTATED surface: for odd quarter_turns the UD output is dst->height x dst->width.
 */
VALI_API int vali_ud_nv12_rot(const vali_surface* src, const vali_surface* dst, int quarter_turns,
                              vali_stream_t stream);
VALI_API int vali_ud_nv12_rot_batch(const vali_surface* d_src, const vali_surface* d_dst, int n,
                                    int src_format, int src_width, int src_height, int dst_width, int dst_height,
                                    int dst_format, int quarter_turns, vali_stream_t stream);

/* ---- resize: replaces nppiResize_{8u,32f}_C{1,3}R_Ctx --------------------------------- */

/* Values follow NppiInterpolationMode (NPPI_INTER_LINEAR = 2 is not used by the reference;
 * NPPI_INTER_LANCZOS = 16 is what every nppiResize call site passes; NPPI_INTER_CUBIC = 4 is the
 * "bicubic" BASELINE.json's north_star names).  All modes sample on the grid
 * src = dst * (src_size / dst_size), no half-pixel shift -- pinned by the reference fixture
 * test_small.nv12 (tests/test_oracle_resize.py). */
enum vali_interpolation {
  VALI_INTERP_LINEAR = 1,   /* bilinear: BASELINE.json config 3 */
  VALI_INTERP_CUBIC = 4,    /* 4x4 Keys / Catmull-Rom cubic convolution (a = -1/2) */
  VALI_INTERP_LANCZOS = 16  /* 6x6 interpolating Lanczos-3 (TaskResizeSurface.cpp:67,116,224,273): the reference's
                               only filter and PySurfaceResizer's default; taps + grid pinned against NPP output at a
                               non-integer ratio (tests/test_oracle_reference_pins.py) */
};

/*
 * Resize every plane of a surface in one launch (src->format == dst->format).
 * Replaces ResizeSurface and its five per-format implementations
 * (reference: src/TC/src/TaskResizeSurface.cpp:34-286; NV12 via the NV12->YUV420->resize->
 * YUV420->NV12 round trip :132-188).  Formats: Y, NV12, P10, P12, YUV420(_10BIT), YUV422,
 * YUV444(_10BIT), RGB, BGR, RGB_32F, RGB_PLANAR, RGB_32F_PLANAR.  The reference's resizer is
 * Lanczos-only (NPPI_INTER_LANCZOS, :67); bilinear is BASELINE.json's definition.
 *
 * Device memory the library owns itself: the Lanczos / bicubic forms keep per-geometry TAP TABLES (32 B per destination
 * column / row).  All tables of a device live in ONE 32 MiB arena that the first Lanczos / bicubic call of the process on
 * that device reserves (the only hipMalloc the operators ever make: once per device and process); every later call --
 * new geometries included -- allocates nothing and is asynchronous on `stream`.  Least recently used tables are evicted
 * when the arena or VALI_TUNE_TAP_MAX_TABLES is exhausted; during a graph capture, and for axes longer than 32 768 samples,
 * no table is used (the kernels compute their taps: same result).  vali_stream_destroy makes the library forget the stream.
 */
VALI_API int vali_resize(const vali_surface* src, const vali_surface* dst, int interpolation,
                         vali_stream_t stream);
VALI_API int vali_resize_batch(const vali_surface* d_src, const vali_surface* d_dst, int n,
                               int format, int src_width, int src_height, int dst_width,
                               int dst_height, int interpolation, vali_stream_t stream);

/*
 * UDPlanar: every plane of a planar 4:2:0 surface resized to the size of the matching plane of a 4:4:4
 * surface (chroma 2x up + the common scale), all three planes in ONE launch.  Replaces UDPlanar
 * (reference: src/TC/src/UDSurface.cpp:33-93, three nppiResize calls) for the planar rows of
 * UDSurface::SupportedConversions() (:117-133): YUV420 -> YUV444, YUV420_10BIT -> YUV444_10BIT; any other
 * pair returns VALI_ERR_UNSUPPORTED.  The reference passes NPPI_INTER_LANCZOS (:45,72): pass
 * VALI_INTERP_LANCZOS for its result; the other modes are accepted too.  As in the reference the
 * destination size alone defines the scale.
 */
VALI_API int vali_ud_planar(const vali_surface* src, const vali_surface* dst, int interpolation,
                            vali_stream_t stream);
VALI_API int vali_ud_planar_batch(const vali_surface* d_src, const vali_surface* d_dst, int n,
                                  int src_format, int dst_format, int src_width, int src_height,
                                  int dst_width, int dst_height, int interpolation, vali_stream_t stream);

/* ---- rotation: replaces nppiRotate_{8u,16u,32f}_{C1,C3}R_Ctx ------------------------ */

/*
 * Rotate every plane of a surface by `angle` degrees and shift (NPP model: x' = x cos a +
 * y sin a + shift_x, y' = -x sin a + y cos a + shift_y; inverse-mapped, bilinear; destination
 * pixels whose source point is outside the source plane are left untouched).
 * Reference call sites: Rot_8U_C1 ... Rot_32F_C3 via RotPlanar / RotPacked,
 * src/TC/src/RotateSurface.cpp:22-159 (one NPP call per plane; here one launch per surface
 * or per batch).  Formats: Y, RGB, BGR, RGB_32F, YUV420(_10BIT), YUV422, YUV444(_10BIT).
 * per_plane_shifts != 0 (angle must be a multiple of 90): ignore shift_x/shift_y and give
 * each plane the shifts PySurfaceRotator derives from ITS size
 * (src/python_vali/src/PySurfaceRotator.cpp:47-73) -- the exact quarter-turn permutation,
 * done as an LDS-tiled transpose for 90 / 270 degrees.
 */
VALI_API int vali_rotate(const vali_surface* src, const vali_surface* dst, double angle,
                         double shift_x, double shift_y, int per_plane_shifts,
                         vali_stream_t stream);
VALI_API int vali_rotate_batch(const vali_surface* d_src, const vali_surface* d_dst, int n,
                               int format, int src_width, int src_height, int dst_width,
                               int dst_height, double angle, double shift_x, double shift_y,
                               int per_plane_shifts, vali_stream_t stream);
/* cos/sin of the angle as the kernels use them (exact 0/+-1 for multiples of 90 degrees) */
VALI_API int vali_rotate_coeffs(double angle_deg, float* c, float* s);

/* ---- tuning switches and tracing -------------------------------------------------------------
 *
 * Every alternative kernel form the library keeps for path-coverage tests and measurements is selected
 * through this ONE table (no getenv anywhere else in the library).  Forms that only a switch could reach are
 * retired: their keys keep their numbers and are accepted without effect, and a retired value of a live key
 * selects the default form.  A switch never changes a result -- every form is bit-identical
 * (tests/test_gpu_tuning.py runs each operator under every value) -- only which kernel produces it.  Values are process-wide and may be changed at any time between calls.
 * Initial values: the default below, or the environment variable of the same name (VALI_<KEY>) read once,
 * when the library is first used.
 */
enum vali_tuning_key {
  VALI_TUNE_NV12_ROWPAIRS = 0,        /* row pairs stacked in one workgroup of the streaming converters; 0 = auto */
  VALI_TUNE_WAVES_PER_CU = 1,         /* residency cap of the streaming converters; 0 = auto                      */
  VALI_TUNE_NV12_DIRECT_STORE = 2,    /* no effect (retired: selected per-lane 48 B stores of NV12->RGB instead of the LDS
                                         strip, measured slower); the key keeps its number                         */
  VALI_TUNE_RESIZE_FORCE_GATHER = 3,  /* 1: every resize geometry through the direct-gather form                  */
  VALI_TUNE_RESIZE_POINT = 4,         /* 0: arithmetic form at integer scale factors; 2: staged point form only (default 1) */
  VALI_TUNE_UD_FORCE_GATHER = 5,      /* 1: every UD geometry through the direct-gather form, no exact-ratio kernels */
  VALI_TUNE_UD_DOWN2 = 6,             /* 0: general UD kernel also at the exact 2:1 / 1:1 width ratios; 1 (default):
                                         exact-ratio kernels for output widths that are multiples of 8; 2: for all */
  VALI_TUNE_UD_OCC5 = 7,              /* no effect since round 2 (selected a 96-register instantiation of the staged UD
                                         kernel, removed: it spilled); the key keeps its number                       */
  VALI_TUNE_ROTATE_NO_TILE = 8,       /* 1: quarter / half turns through the bilinear kernel (retired values: 2, a
                                         column-major tile walk, and 3, fused UD + quarter turn on 128-row tiles)    */
  VALI_TUNE_ROCTX = 9,                /* 1: a roctx range around every operator entry point (see below)            */
  VALI_TUNE_RESIZE_NO_SEPARABLE = 10, /* Lanczos / bicubic rows per wave: 0 by launch size, 1: few, 2: fewest (and the slot walk
                                         where the 3:2-both-ways form has a static one), 3: most (growing planes: 32-row waves), 4: growing planes on
                                         64-row waves whatever the launch size; 11 .. 42: an explicit count (rows per slot / row
                                         pairs per wave: measurements only)                                          */
  VALI_TUNE_ROWS_PER_WAVE = 11,       /* UD, bilinear / point resize, fused pre-processing: dst rows (row pairs) a wave
                                         walks: 0 by launch size (8 for batches, 4 or 2 for small launches), 2 / 4 / 8  */
  VALI_TUNE_BLOCKING_WAIT = 12,       /* vali_stream_wait: 0 completion word + spin (default), 1 hipStreamSynchronize */
  VALI_TUNE_RESIZE_ROWS = 13,         /* Lanczos / bicubic of planes that grow: 1 (default) filtered rows in registers
                                         (resize_rows.hip) where the geometry fits, exact 3:2 enlargements through their static
                                         form; 2: the same without the 3:2 form; 3: without the register form of round 4 (8-bit planes
                                         that grow along x too: row pass from registers, no LDS stage); 0: round 2's LDS-ring kernel  */
  VALI_TUNE_RESIZE_COLS = 14,         /* Lanczos / bicubic of planes that shrink, general ratios: 0 (default) a workgroup = one wave that
                                         walks the source rows + one that runs the pass along the rows (round 5), taps from per-geometry
                                         tables (tap_table.hip); 2: the same, taps computed in the kernel (retired value: 1, both
                                         passes in every wave, round 4's form)                                        */
  VALI_TUNE_ROTATE_AFFINE = 15,       /* rotation by an angle that is no canonical quarter / half turn: 0 (default) a workgroup stages the source
                                         box of its destination tile in LDS (round 6), tile shape by launch size; 1: per-pixel gathers from global
                                         memory (round 2's form, also taken for planes narrower than a staged row); tile shapes:
                                         3 = 64 x 32, 4 = 64 x 64, 5 = 64 x 128 (one-channel 8-bit planes), 6 = 32 x 32 (retired value:
                                         2, 32 x 64)                                                                  */
  VALI_TUNE_TAP_MAX_TABLES = 16,      /* tap tables (Lanczos / bicubic axes) kept per device before the least recently used is evicted; default 1024, at least 8
                                         (they share one 32 MiB arena per device, reserved by the first Lanczos / bicubic call on it)        */
  VALI_TUNE_TAP_FALLBACKS = 17,       /* COUNTER (read with vali_tuning_get, reset by setting 0): resize calls that got no tap table outside a
                                         graph capture and computed their taps in the kernel (axis > 32768 samples, nothing evictable, HIP error) */
  VALI_TUNE_TAP_EVICTIONS = 18,       /* COUNTER: tap tables evicted so far                                              */
  VALI_TUNE_COUNT = 19
};
VALI_API int vali_tuning_set(int key, int value);
VALI_API int vali_tuning_get(int key, int* value);

/*
 * Tracing: with VALI_TUNE_ROCTX = 1 (or VALI_ROCTX=1 in the environment) every operator entry point of this
 * header pushes a roctx range named after itself for the duration of the call -- the equivalent of the
 * reference's NvtxMark around every converter / resizer (src/TC/inc/Tasks.hpp:32-59, e.g.
 * TaskConvertSurface.cpp:112).  `rocprofv3 --marker-trace --kernel-trace` then shows which launch belongs to
 * which call.  The roctx library (librocprofiler-sdk-roctx / libroctx64) is dlopen'ed on first use; if it is
 * absent tracing stays off and vali_tuning_set(VALI_TUNE_ROCTX, 1) returns VALI_ERR_UNSUPPORTED.
 */

/* ---- diagnostics (used by tests only) --------------------------------------- */

/* out[i] = float->u8 quantiser of the colour kernels applied to in[i]. */
VALI_API int vali_debug_quantize_u8(const float* d_in, uint8_t* d_out, int n,
                                    vali_stream_t stream);
/* same with the instruction-independent formulation (rint, clamp, convert). */
VALI_API int vali_debug_quantize_u8_portable(const float* d_in, uint8_t* d_out, int n,
                                             vali_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VALI_HIP_H */
