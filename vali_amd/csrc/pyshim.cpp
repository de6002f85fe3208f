// _vali_shim: thin pybind11 binding of the C ABI in include/vali_hip.h.
//
// Nothing here computes anything: every function forwards plain integers
// (device pointers, stream handles) and small PODs to libvali_hip.so, the same
// way the reference's pybind11 layer forwards to its Task objects
// (reference: src/python_vali/src/*.cpp).  The host logic of the path (format
// dispatch, validation, error codes) lives in Python (vali_amd/*.py).
// The only non-forwarding code is DLPack capsule plumbing, which needs C.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <array>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "dlpack_min.h"
#include "vali_hip.h"

namespace py = pybind11;

namespace {

void check(int rc, const char* what) {
  if (rc == VALI_OK)
    return;
  std::string msg = std::string(what) + ": " + vali_last_error();
  if (rc == VALI_ERR_INVALID_ARG || rc == VALI_ERR_UNSUPPORTED)
    throw py::value_error(msg);
  throw std::runtime_error(msg);
}

inline void* P(uintptr_t v) { return reinterpret_cast<void*>(v); }

struct SurfaceDesc {
  vali_surface s;
};

struct Csc {
  vali_csc k;
};

struct CvtParams {
  vali_cvt_params p;
};

struct PreprocParams {
  vali_preproc_params p;
};

struct TensorDst {
  vali_tensor_dst t;
};

struct TensorSrc {
  vali_tensor_src t;
};

struct JpegParams {
  vali_jpeg_params p;
};

struct JpegInfo {
  vali_jpeg_info f;
};

// the host copy of a list of descriptors, as the C ABI takes it
std::vector<vali_surface> host_surfaces(const std::vector<SurfaceDesc>& descs) {
  std::vector<vali_surface> host(descs.size());
  for (size_t i = 0; i < descs.size(); ++i)
    host[i] = descs[i].s;
  return host;
}

// (ptr, dtype, stride_n, stride_k, stride_c) -> vali_detect_tensor
vali_detect_tensor detect_tensor(const std::array<int64_t, 5>& t) {
  vali_detect_tensor d;
  std::memset(&d, 0, sizeof(d));
  d.data = P((uintptr_t)t[0]);
  d.dtype = (int32_t)t[1];
  d.stride_n = t[2]; d.stride_k = t[3]; d.stride_c = t[4];
  return d;
}

// (ptr, dtype, stride_n, stride_m, stride_y) -> vali_mask_tensor
vali_mask_tensor mask_tensor(const std::array<int64_t, 5>& t) {
  vali_mask_tensor d;
  std::memset(&d, 0, sizeof(d));
  d.data = P((uintptr_t)t[0]);
  d.dtype = (int32_t)t[1];
  d.stride_n = t[2]; d.stride_m = t[3]; d.stride_y = t[4];
  return d;
}

// (ptr, dtype, stride_n, stride_k, stride_p, stride_c) and kdim into vali_pose_in / vali_warp_fit_in, which spell the
// keypoint tensor's fields alike
template <class In>
void fill_kpts(In& in, const std::array<int64_t, 6>& kpts, int kdim) {
  in.kpts = P((uintptr_t)kpts[0]);
  in.dtype = (int32_t)kpts[1];
  in.kdim = kdim;
  in.stride_n = kpts[2]; in.stride_k = kpts[3]; in.stride_p = kpts[4]; in.stride_c = kpts[5];
}

vali_roi to_roi(const std::array<int32_t, 8>& v) {
  vali_roi r;
  r.src_x = v[0]; r.src_y = v[1]; r.src_w = v[2]; r.src_h = v[3];
  r.dst_x = v[4]; r.dst_y = v[5]; r.dst_w = v[6]; r.dst_h = v[7];
  return r;
}

// ---- DLPack ------------------------------------------------------------------

struct ExportCtx {
  PyObject* owner; // keeps the producing Surface / SurfacePlane alive
  int64_t dims[8];
};

void export_deleter(DLManagedTensor* self) {
  if (!self)
    return;
  auto* ctx = static_cast<ExportCtx*>(self->manager_ctx);
  if (ctx) {
    if (ctx->owner) {
      py::gil_scoped_acquire gil;
      Py_DECREF(ctx->owner);
    }
    delete ctx;
  }
  delete self;
}

void capsule_destructor(PyObject* cap) {
  // Only un-consumed capsules still own the tensor.
  if (!PyCapsule_IsValid(cap, "dltensor"))
    return;
  auto* m = static_cast<DLManagedTensor*>(PyCapsule_GetPointer(cap, "dltensor"));
  if (m && m->deleter)
    m->deleter(m);
}

py::object dlpack_export(uintptr_t ptr, const std::vector<int64_t>& shape,
                         const std::vector<int64_t>& strides, int code, int bits,
                         int device_type, int device_id, py::object owner) {
  const size_t nd = shape.size();
  if (nd == 0 || nd > 4 || strides.size() != nd)
    throw py::value_error("dlpack_export: bad shape/strides");
  auto* ctx = new ExportCtx();
  auto* m = new DLManagedTensor();
  std::memset(m, 0, sizeof(*m));
  for (size_t i = 0; i < nd; ++i) {
    ctx->dims[i] = shape[i];
    ctx->dims[4 + i] = strides[i];
  }
  ctx->owner = owner.is_none() ? nullptr : owner.inc_ref().ptr();
  m->dl_tensor.data = P(ptr);
  m->dl_tensor.device.device_type = device_type;
  m->dl_tensor.device.device_id = device_id;
  m->dl_tensor.ndim = (int32_t)nd;
  m->dl_tensor.dtype.code = (uint8_t)code;
  m->dl_tensor.dtype.bits = (uint8_t)bits;
  m->dl_tensor.dtype.lanes = 1;
  m->dl_tensor.shape = ctx->dims;
  m->dl_tensor.strides = ctx->dims + 4;
  m->dl_tensor.byte_offset = 0;
  m->manager_ctx = ctx;
  m->deleter = export_deleter;
  PyObject* cap = PyCapsule_New(m, "dltensor", capsule_destructor);
  if (!cap) {
    export_deleter(m);
    throw py::error_already_set();
  }
  return py::reinterpret_steal<py::object>(cap);
}

// Owns an imported DLManagedTensor; the producer's deleter runs when the last
// Surface borrowing that memory goes away.
struct DLPackHolder {
  DLManagedTensor* m = nullptr;
  ~DLPackHolder() {
    if (m && m->deleter)
      m->deleter(m);
  }
};

py::tuple dlpack_import(py::object capsule) {
  PyObject* cap = capsule.ptr();
  if (!PyCapsule_CheckExact(cap))
    throw std::runtime_error("Empty capsule.");
  if (!PyCapsule_IsValid(cap, "dltensor"))
    throw std::runtime_error("Capsule doesn't contain dltensor.");
  auto* m = static_cast<DLManagedTensor*>(PyCapsule_GetPointer(cap, "dltensor"));
  if (!m)
    throw std::runtime_error("Capsule doesn't contain dltensor.");
  const DLTensor& t = m->dl_tensor;
  py::dict info;
  std::vector<int64_t> shape(t.shape, t.shape + t.ndim), strides;
  if (t.strides) {
    strides.assign(t.strides, t.strides + t.ndim);
  } else { // compact row-major
    strides.resize(t.ndim);
    int64_t acc = 1;
    for (int i = t.ndim - 1; i >= 0; --i) {
      strides[i] = acc;
      acc *= t.shape[i];
    }
  }
  info["ptr"] = (uintptr_t)t.data + t.byte_offset;
  info["shape"] = shape;
  info["strides"] = strides;
  info["code"] = (int)t.dtype.code;
  info["bits"] = (int)t.dtype.bits;
  info["lanes"] = (int)t.dtype.lanes;
  info["device_type"] = (int)t.device.device_type;
  info["device_id"] = (int)t.device.device_id;
  // consume: standard DLPack hand-over
  PyCapsule_SetName(cap, "used_dltensor");
  PyCapsule_SetDestructor(cap, nullptr);
  auto holder = std::make_unique<DLPackHolder>();
  holder->m = m;
  return py::make_tuple(info, py::cast(std::move(holder)));
}

} // namespace

PYBIND11_MODULE(_vali_shim, m) {
  m.doc() = "1:1 binding of libvali_hip.so (include/vali_hip.h)";

  m.attr("OK") = VALI_OK;
  m.attr("ERR_INVALID_ARG") = VALI_ERR_INVALID_ARG;
  m.attr("ERR_UNSUPPORTED") = VALI_ERR_UNSUPPORTED;
  m.attr("ERR_RUNTIME") = VALI_ERR_RUNTIME;
  m.attr("ERR_NO_DEVICE") = VALI_ERR_NO_DEVICE;
  m.attr("SURFACE_DESC_SIZE") = sizeof(vali_surface);
  m.attr("ROI_SIZE") = sizeof(vali_roi);

  py::class_<SurfaceDesc>(m, "SurfaceDesc")
      .def(py::init([](std::vector<uintptr_t> planes, std::vector<int> pitches, int width,
                       int height, int format) {
             SurfaceDesc d;
             std::memset(&d.s, 0, sizeof(d.s));
             for (size_t i = 0; i < planes.size() && i < 3; ++i)
               d.s.plane[i] = P(planes[i]);
             for (size_t i = 0; i < pitches.size() && i < 3; ++i)
               d.s.pitch[i] = pitches[i];
             d.s.width = width;
             d.s.height = height;
             d.s.format = format;
             return d;
           }),
           py::arg("planes"), py::arg("pitches"), py::arg("width"), py::arg("height"),
           py::arg("format"))
      .def("tobytes",
           [](const SurfaceDesc& d) { return py::bytes((const char*)&d.s, sizeof(d.s)); })
      .def_property_readonly("width", [](const SurfaceDesc& d) { return d.s.width; })
      .def_property_readonly("height", [](const SurfaceDesc& d) { return d.s.height; })
      .def_property_readonly("format", [](const SurfaceDesc& d) { return d.s.format; });

  py::class_<Csc>(m, "Csc")
      .def(py::init([](float y0, float cy, float crv, float cgu, float cgv, float cbu) {
             Csc c;
             std::memset(&c.k, 0, sizeof(c.k));
             c.k.y0 = y0; c.k.cy = cy; c.k.crv = crv; c.k.cgu = cgu; c.k.cgv = cgv; c.k.cbu = cbu;
             return c;
           }))
      .def("astuple", [](const Csc& c) {
        return py::make_tuple(c.k.y0, c.k.cy, c.k.crv, c.k.cgu, c.k.cgv, c.k.cbu);
      });

  py::class_<DLPackHolder>(m, "DLPackHolder");

  m.def("last_error", []() { return std::string(vali_last_error()); });
  // tuning switches / tracing (include/vali_hip.h: vali_tuning_key)
  for (auto kv : {std::pair<const char*, int>{"TUNE_NV12_ROWPAIRS", VALI_TUNE_NV12_ROWPAIRS},
                  {"TUNE_WAVES_PER_CU", VALI_TUNE_WAVES_PER_CU},
                  {"TUNE_NV12_DIRECT_STORE", VALI_TUNE_NV12_DIRECT_STORE},
                  {"TUNE_RESIZE_FORCE_GATHER", VALI_TUNE_RESIZE_FORCE_GATHER},
                  {"TUNE_RESIZE_POINT", VALI_TUNE_RESIZE_POINT},
                  {"TUNE_UD_FORCE_GATHER", VALI_TUNE_UD_FORCE_GATHER},
                  {"TUNE_UD_DOWN2", VALI_TUNE_UD_DOWN2},
                  {"TUNE_UD_OCC5", VALI_TUNE_UD_OCC5},
                  {"TUNE_ROTATE_NO_TILE", VALI_TUNE_ROTATE_NO_TILE},
                  {"TUNE_ROCTX", VALI_TUNE_ROCTX},
                  {"TUNE_RESIZE_NO_SEPARABLE", VALI_TUNE_RESIZE_NO_SEPARABLE},
                  {"TUNE_ROWS_PER_WAVE", VALI_TUNE_ROWS_PER_WAVE},
                  {"TUNE_BLOCKING_WAIT", VALI_TUNE_BLOCKING_WAIT},
                  {"TUNE_RESIZE_ROWS", VALI_TUNE_RESIZE_ROWS},
                  {"TUNE_RESIZE_COLS", VALI_TUNE_RESIZE_COLS},
                  {"TUNE_ROTATE_AFFINE", VALI_TUNE_ROTATE_AFFINE},
                  {"TUNE_TAP_MAX_TABLES", VALI_TUNE_TAP_MAX_TABLES},
                  {"TUNE_TAP_FALLBACKS", VALI_TUNE_TAP_FALLBACKS},
                  {"TUNE_TAP_EVICTIONS", VALI_TUNE_TAP_EVICTIONS},
                  {"TUNE_COUNT", VALI_TUNE_COUNT}})
    m.attr(kv.first) = kv.second;
  m.def("tuning_set", [](int key, int value) { return vali_tuning_set(key, value); });
  m.def("tuning_get", [](int key) {
    int v = 0;
    check(vali_tuning_get(key, &v), "vali_tuning_get");
    return v;
  });
  m.def("version", []() { return std::string(vali_version()); });
  m.def("device_count", []() {
    int n = 0;
    (void)vali_device_count(&n); // "no device" is a count of 0, not an exception
    return n;
  });
  m.def("device_set", [](int device) { check(vali_device_set(device), "device_set"); });
  m.def("device_get", []() {
    int d = -1;
    check(vali_device_get(&d), "device_get");
    return d;
  });
  m.def("ptr_device", [](uintptr_t p) {
    int d = -1;
    check(vali_ptr_device(P(p), &d), "vali_ptr_device");
    return d;
  });

  m.def("stream_create", [](int device) {
    vali_stream_t s = nullptr;
    check(vali_stream_create(device, &s), "vali_stream_create");
    return (uintptr_t)s;
  });
  m.def("stream_destroy", [](int device, uintptr_t s) {
    check(vali_stream_destroy(device, P(s)), "vali_stream_destroy");
  });
  m.def("stream_wait",
        [](int device, uintptr_t s) { check(vali_stream_wait(device, P(s)), "vali_stream_wait"); },
        py::call_guard<py::gil_scoped_release>());
  m.def("stream_sync",
        [](int device, uintptr_t s) { check(vali_stream_sync(device, P(s)), "vali_stream_sync"); },
        py::call_guard<py::gil_scoped_release>());

  m.def("event_create", [](int device) {
    vali_event_t e = nullptr;
    check(vali_event_create(device, &e), "vali_event_create");
    return (uintptr_t)e;
  });
  m.def("event_destroy", [](int device, uintptr_t e) {
    check(vali_event_destroy(device, P(e)), "vali_event_destroy");
  });
  m.def("event_record", [](int device, uintptr_t e, uintptr_t s) {
    check(vali_event_record(device, P(e), P(s)), "vali_event_record");
  });
  m.def("event_query", [](int device, uintptr_t e) {
    int done = 0;
    check(vali_event_query(device, P(e), &done), "vali_event_query");
    return done != 0;
  });
  m.def("stream_wait_event", [](int device, uintptr_t s, uintptr_t e) {
    check(vali_stream_wait_event(device, P(s), P(e)), "vali_stream_wait_event");
  });
  m.def("host_alloc", [](int device, size_t bytes) {
    void* p = nullptr;
    check(vali_host_alloc(device, bytes, &p), "vali_host_alloc");
    return (uintptr_t)p;
  });
  m.def("host_free", [](int device, uintptr_t p) { check(vali_host_free(device, P(p)), "vali_host_free"); });
  m.def("mem_info", [](int device) {
    size_t f = 0, t = 0;
    check(vali_mem_info(device, &f, &t), "vali_mem_info");
    return py::make_tuple(f, t);
  });
  m.def("device_pci_bus_id", [](int device) {
    char buf[32] = {0};
    check(vali_device_pci_bus_id(device, buf, (int)sizeof buf), "vali_device_pci_bus_id");
    return std::string(buf);
  });
  m.def("event_sync",
        [](int device, uintptr_t e) { check(vali_event_sync(device, P(e)), "vali_event_sync"); },
        py::call_guard<py::gil_scoped_release>());
  m.def("event_elapsed_ms", [](uintptr_t a, uintptr_t b) {
    float ms = 0.f;
    check(vali_event_elapsed_ms(P(a), P(b), &ms), "vali_event_elapsed_ms");
    return ms;
  });

  m.def("graph_capture_begin",
        [](int device, uintptr_t s) { check(vali_graph_capture_begin(device, P(s)), "vali_graph_capture_begin"); });
  m.def("graph_capture_end", [](int device, uintptr_t s) {
    vali_graph_t g = nullptr;
    check(vali_graph_capture_end(device, P(s), &g), "vali_graph_capture_end");
    return (uintptr_t)g;
  });
  m.def("graph_launch",
        [](int device, uintptr_t g, uintptr_t s) { check(vali_graph_launch(device, P(g), P(s)), "vali_graph_launch"); },
        py::call_guard<py::gil_scoped_release>());
  m.def("graph_destroy", [](int device, uintptr_t g) { return vali_graph_destroy(device, P(g)); });

  m.def("mem_alloc_pitch", [](int device, size_t width_bytes, size_t height) {
    void* p = nullptr;
    size_t pitch = 0;
    check(vali_mem_alloc_pitch(device, width_bytes, height, &p, &pitch), "vali_mem_alloc_pitch");
    return py::make_tuple((uintptr_t)p, pitch);
  });
  m.def("mem_alloc", [](int device, size_t bytes) {
    void* p = nullptr;
    check(vali_mem_alloc(device, bytes, &p), "vali_mem_alloc");
    return (uintptr_t)p;
  });
  m.def("mem_free", [](int device, uintptr_t p) {
    // destructor path: never throw
    return vali_mem_free(device, P(p));
  });

  m.def("memcpy2d_async",
        [](int device, uintptr_t dst, size_t dpitch, uintptr_t src, size_t spitch, size_t wbytes,
           size_t height, int kind, uintptr_t stream) {
          check(vali_memcpy2d_async(device, P(dst), dpitch, P(src), spitch, wbytes, height, kind,
                                    P(stream)),
                "vali_memcpy2d_async");
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("memset2d_async",
        [](int device, uintptr_t dst, size_t dpitch, int value, size_t wbytes, size_t height,
           uintptr_t stream) {
          check(vali_memset2d_async(device, P(dst), dpitch, value, wbytes, height, P(stream)),
                "vali_memset2d_async");
        });

  // address of a Python buffer (numpy array, bytes, bytearray) for H2D / D2H copies
  m.def("buffer_info", [](py::buffer b, bool writable) {
    py::buffer_info info = b.request(writable);
    bool contiguous = true;
    py::ssize_t expect = info.itemsize;
    for (int i = (int)info.ndim - 1; i >= 0; --i) {
      if (info.shape[i] != 1 && info.strides[i] != expect)
        contiguous = false;
      expect *= info.shape[i];
    }
    return py::make_tuple((uintptr_t)info.ptr, (size_t)(info.size * info.itemsize), contiguous);
  });

  // upload a list of descriptors into a fresh device array (blocking)
  m.def("descs_upload", [](int device, const std::vector<SurfaceDesc>& descs, uintptr_t stream) {
    if (descs.empty())
      throw py::value_error("descs_upload: empty list");
    const std::vector<vali_surface> host = host_surfaces(descs);
    const size_t bytes = host.size() * sizeof(vali_surface);
    void* d = nullptr;
    check(vali_mem_alloc(device, bytes, &d), "vali_mem_alloc");
    int rc = vali_memcpy2d_async(device, d, bytes, host.data(), bytes, bytes, 1, 0, P(stream));
    if (rc == VALI_OK)
      rc = vali_stream_sync(device, P(stream));
    if (rc != VALI_OK) {
      vali_mem_free(device, d);
      check(rc, "descs_upload");
    }
    return (uintptr_t)d;
  });

  // the same for rectangle records: a list of (src_x, src_y, src_w, src_h, dst_x, dst_y, dst_w, dst_h)
  m.def("rois_upload", [](int device, const std::vector<std::array<int32_t, 8>>& rois, uintptr_t stream) {
    if (rois.empty())
      throw py::value_error("rois_upload: empty list");
    std::vector<vali_roi> host(rois.size());
    for (size_t i = 0; i < rois.size(); ++i)
      host[i] = to_roi(rois[i]);
    const size_t bytes = host.size() * sizeof(vali_roi);
    void* d = nullptr;
    check(vali_mem_alloc(device, bytes, &d), "vali_mem_alloc");
    int rc = vali_memcpy2d_async(device, d, bytes, host.data(), bytes, bytes, 1, 0, P(stream));
    if (rc == VALI_OK)
      rc = vali_stream_sync(device, P(stream));
    if (rc != VALI_OK) {
      vali_mem_free(device, d);
      check(rc, "rois_upload");
    }
    return (uintptr_t)d;
  });

  // ---- operators: return the C status code; Python maps it to TaskExecInfo ----
  m.def("nv12_to_rgb",
        [](const SurfaceDesc& src, const SurfaceDesc& dst, const Csc& csc, uintptr_t stream) {
          return vali_nv12_to_rgb(&src.s, &dst.s, &csc.k, P(stream));
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("nv12_to_rgb_batch",
        [](uintptr_t d_src, uintptr_t d_dst, int n, int width, int height, int dst_format,
           const Csc& csc, uintptr_t stream) {
          return vali_nv12_to_rgb_batch((const vali_surface*)P(d_src),
                                        (const vali_surface*)P(d_dst), n, width, height,
                                        dst_format, &csc.k, P(stream));
        },
        py::call_guard<py::gil_scoped_release>());

  py::class_<CvtParams>(m, "CvtParams")
      .def(py::init([](const Csc* csc, const std::vector<std::vector<float>>& rgb2yuv) {
             CvtParams p;
             std::memset(&p.p, 0, sizeof(p.p));
             if (csc)
               p.p.yuv2rgb = csc->k;
             for (size_t i = 0; i < rgb2yuv.size() && i < 3; ++i)
               for (size_t j = 0; j < rgb2yuv[i].size() && j < 4; ++j)
                 p.p.rgb2yuv[i][j] = rgb2yuv[i][j];
             return p;
           }),
           py::arg("csc") = nullptr, py::arg("rgb2yuv") = std::vector<std::vector<float>>());
  m.def("convert",
        [](const SurfaceDesc& src, const SurfaceDesc& dst, const CvtParams& p, uintptr_t stream) {
          return vali_convert(&src.s, &dst.s, &p.p, P(stream));
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("convert_batch",
        [](uintptr_t d_src, uintptr_t d_dst, int n, int src_format, int dst_format, int width,
           int height, const CvtParams& p, uintptr_t stream) {
          return vali_convert_batch((const vali_surface*)P(d_src), (const vali_surface*)P(d_dst), n,
                                    src_format, dst_format, width, height, &p.p, P(stream));
        },
        py::call_guard<py::gil_scoped_release>());

  py::class_<PreprocParams>(m, "PreprocParams")
      .def(py::init([](const Csc& csc, float div, const std::vector<float>& mean,
                       const std::vector<float>& std_) {
        PreprocParams p;
        std::memset(&p.p, 0, sizeof(p.p));
        p.p.csc = csc.k;
        p.p.div = div;
        for (size_t i = 0; i < 3; ++i) {
          p.p.mean[i] = i < mean.size() ? mean[i] : 0.0f;
          p.p.std_[i] = i < std_.size() ? std_[i] : 1.0f;
        }
        return p;
      }));
  m.def("nv12_preproc",
        [](const SurfaceDesc& src, const SurfaceDesc& dst, const PreprocParams& p, uintptr_t stream) {
          return vali_nv12_preproc(&src.s, &dst.s, &p.p, P(stream));
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("nv12_preproc_batch",
        [](uintptr_t d_src, uintptr_t d_dst, int n, int src_width, int src_height, int dst_width,
           int dst_height, int dst_format, const PreprocParams& p, uintptr_t stream) {
          return vali_nv12_preproc_batch((const vali_surface*)P(d_src), (const vali_surface*)P(d_dst), n,
                                         src_width, src_height, dst_width, dst_height, dst_format, &p.p,
                                         P(stream));
        },
        py::call_guard<py::gil_scoped_release>());

  m.def("nv12_preproc_roi",
        [](const SurfaceDesc& src, const SurfaceDesc& dst, const std::array<int32_t, 8>& roi, const PreprocParams& p,
           bool pad, const std::array<uint8_t, 3>& pad_rgb, uintptr_t stream) {
          const vali_roi r = to_roi(roi);
          return vali_nv12_preproc_roi(&src.s, &dst.s, &r, &p.p, pad ? 1 : 0, pad_rgb.data(), P(stream));
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("nv12_preproc_roi_batch",
        [](uintptr_t d_src, uintptr_t d_dst, uintptr_t d_roi, int n, int dst_width, int dst_height, int dst_format,
           const PreprocParams& p, bool pad, const std::array<uint8_t, 3>& pad_rgb, uintptr_t stream) {
          return vali_nv12_preproc_roi_batch((const vali_surface*)P(d_src), (const vali_surface*)P(d_dst),
                                             (const vali_roi*)P(d_roi), n, dst_width, dst_height, dst_format, &p.p,
                                             pad ? 1 : 0, pad_rgb.data(), P(stream));
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("rgb_preproc_roi",
        [](const SurfaceDesc& src, const SurfaceDesc& dst, const std::array<int32_t, 8>& roi, const PreprocParams& p,
           bool pad, const std::array<uint8_t, 3>& pad_rgb, uintptr_t stream) {
          const vali_roi r = to_roi(roi);
          return vali_rgb_preproc_roi(&src.s, &dst.s, &r, &p.p, pad ? 1 : 0, pad_rgb.data(), P(stream));
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("rgb_preproc_roi_batch",
        [](uintptr_t d_src, uintptr_t d_dst, uintptr_t d_roi, int n, int src_format, int dst_width, int dst_height,
           int dst_format, const PreprocParams& p, bool pad, const std::array<uint8_t, 3>& pad_rgb, uintptr_t stream) {
          return vali_rgb_preproc_roi_batch((const vali_surface*)P(d_src), (const vali_surface*)P(d_dst),
                                            (const vali_roi*)P(d_roi), n, src_format, dst_width, dst_height, dst_format,
                                            &p.p, pad ? 1 : 0, pad_rgb.data(), P(stream));
        },
        py::call_guard<py::gil_scoped_release>());

  // the batch tensor of the tensor forms: (data, dtype, packed, n, width, height, stride_n, stride_c, stride_y), strides in
  // elements; the C entry points judge it
  py::class_<TensorDst>(m, "TensorDst")
      .def(py::init([](uintptr_t data, int dtype, int packed, int n, int width, int height, int64_t stride_n,
                       int64_t stride_c, int64_t stride_y) {
        TensorDst d;
        std::memset(&d.t, 0, sizeof(d.t));
        d.t.data = P(data);
        d.t.dtype = dtype; d.t.packed = packed;
        d.t.n = n; d.t.width = width; d.t.height = height;
        d.t.stride_n = stride_n; d.t.stride_c = stride_c; d.t.stride_y = stride_y;
        return d;
      }));
  m.attr("TENSOR_DST_SIZE") = sizeof(vali_tensor_dst);
  m.attr("DTYPE_F32") = (int)VALI_DTYPE_F32;
  m.attr("DTYPE_F16") = (int)VALI_DTYPE_F16;
  m.attr("DTYPE_BF16") = (int)VALI_DTYPE_BF16;
  m.attr("DTYPE_U8") = (int)VALI_DTYPE_U8;
  m.def("nv12_preproc_roi_tensor",
        [](uintptr_t d_src, uintptr_t d_roi, const TensorDst& dst, const PreprocParams& p, bool pad,
           const std::array<uint8_t, 3>& pad_rgb, uintptr_t stream) {
          return vali_nv12_preproc_roi_tensor((const vali_surface*)P(d_src), (const vali_roi*)P(d_roi), &dst.t, &p.p,
                                              pad ? 1 : 0, pad_rgb.data(), P(stream));
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("rgb_preproc_roi_tensor",
        [](uintptr_t d_src, uintptr_t d_roi, int src_format, const TensorDst& dst, const PreprocParams& p, bool pad,
           const std::array<uint8_t, 3>& pad_rgb, uintptr_t stream) {
          return vali_rgb_preproc_roi_tensor((const vali_surface*)P(d_src), (const vali_roi*)P(d_roi), src_format,
                                             &dst.t, &p.p, pad ? 1 : 0, pad_rgb.data(), P(stream));
        },
        py::call_guard<py::gil_scoped_release>());

  // ---- JPEG: host-side parameters / header / sizes, then the batched encoder -----------------------------------
  py::class_<JpegParams>(m, "JpegParams")
      .def_property_readonly("quality", [](const JpegParams& j) { return j.p.quality; })
      .def_property_readonly("format", [](const JpegParams& j) { return j.p.format; })
      .def_property_readonly("h_samp", [](const JpegParams& j) { return j.p.h_samp; })
      .def_property_readonly("v_samp", [](const JpegParams& j) { return j.p.v_samp; })
      .def_property("restart_interval", [](const JpegParams& j) { return j.p.restart_interval; },
                    [](JpegParams& j, int r) { j.p.restart_interval = r; })
      // 0 or 1; vali_jpeg_* validate it, not the shim
      .def_property("optimize", [](const JpegParams& j) { return j.p.optimize; },
                    [](JpegParams& j, int v) { j.p.optimize = v; })
      .def_property("qtable", [](const JpegParams& j) {
        std::vector<std::vector<int>> t(2, std::vector<int>(64));
        for (int i = 0; i < 2; ++i)
          for (int k = 0; k < 64; ++k)
            t[i][k] = j.p.qtable[i][k];
        return t;
      }, [](JpegParams& j, const std::array<std::array<uint8_t, 64>, 2>& t) {
        // (luma, chroma) in natural order; vali_jpeg_* validate it, not the shim
        for (int i = 0; i < 2; ++i)
          for (int k = 0; k < 64; ++k)
            j.p.qtable[i][k] = t[i][k];
      });
  m.def("jpeg_params_init", [](int quality, int format) {
    JpegParams j;
    check(vali_jpeg_params_init(quality, format, &j.p), "vali_jpeg_params_init");
    return j;
  });
  m.def("jpeg_params_init_sampled", [](int quality, int format, int h_samp, int v_samp) {
    JpegParams j;
    check(vali_jpeg_params_init_sampled(quality, format, h_samp, v_samp, &j.p), "vali_jpeg_params_init_sampled");
    return j;
  });
  m.def("jpeg_header", [](int width, int height, const JpegParams& j) {
    size_t len = 0;
    check(vali_jpeg_header(width, height, &j.p, nullptr, 0, &len), "vali_jpeg_header");
    std::string out(len, '\0');
    check(vali_jpeg_header(width, height, &j.p, (uint8_t*)&out[0], out.size(), &len), "vali_jpeg_header");
    return py::bytes(out);
  });
  m.def("jpeg_workspace_size", [](int n, int width, int height, const JpegParams& j) {
    size_t bytes = 0;
    check(vali_jpeg_workspace_size(n, width, height, &j.p, &bytes), "vali_jpeg_workspace_size");
    return bytes;
  });
  m.def("jpeg_stream_capacity", [](int width, int height, const JpegParams& j) {
    size_t bytes = 0;
    check(vali_jpeg_stream_capacity(width, height, &j.p, &bytes), "vali_jpeg_stream_capacity");
    return bytes;
  });
  m.def("jpeg_encode_batch",
        [](uintptr_t d_src, int n, int width, int height, int format, const JpegParams& j, uintptr_t workspace,
           size_t ws_bytes, uintptr_t d_out, size_t out_stride, uintptr_t d_sizes, uintptr_t stream) {
          return vali_jpeg_encode_batch((const vali_surface*)P(d_src), n, width, height, format, &j.p, P(workspace),
                                        ws_bytes, (uint8_t*)P(d_out), out_stride, (uint32_t*)P(d_sizes), P(stream));
        },
        py::call_guard<py::gil_scoped_release>());

  // regions of surfaces of any sizes: rois is an (n, 4) int32 array of (x, y, width, height), src_w / src_h int32
  // arrays of the surfaces' sizes; the records come back as one bytes blob of n * JPEG_ITEM_SIZE (numpy reads it
  // with a structured dtype), to be copied to the device and passed back as they are
  m.attr("JPEG_ITEM_SIZE") = (int)sizeof(vali_jpeg_item);
  m.def("jpeg_plan_rois", [](py::buffer rois, py::buffer src_w, py::buffer src_h, const JpegParams& j) {
    const py::buffer_info r = rois.request(), w = src_w.request(), h = src_h.request();
    const size_t n = (size_t)w.size;
    if (r.itemsize != 4 || w.itemsize != 4 || h.itemsize != 4 || (size_t)r.size != 4 * n || (size_t)h.size != n)
      throw py::value_error("jpeg_plan_rois: rois must be (n, 4) int32, src_w and src_h n int32 each");
    std::string items(n * sizeof(vali_jpeg_item), '\0');
    size_t ws = 0, out = 0;
    check(vali_jpeg_plan_rois((const vali_jpeg_roi*)r.ptr, (const int32_t*)w.ptr, (const int32_t*)h.ptr, (int)n, &j.p,
                              (vali_jpeg_item*)&items[0], &ws, &out),
          "vali_jpeg_plan_rois");
    return py::make_tuple(py::bytes(items), ws, out);
  });
  m.def("jpeg_encode_rois",
        [](uintptr_t d_src, py::buffer items, uintptr_t d_items, int n, const JpegParams& j, uintptr_t workspace,
           size_t ws_bytes, uintptr_t d_out, size_t out_bytes, uintptr_t d_sizes, uintptr_t stream) {
          const py::buffer_info it = items.request();
          if ((size_t)(it.size * it.itemsize) != (size_t)n * sizeof(vali_jpeg_item))
            throw py::value_error("jpeg_encode_rois: items must hold n records of JPEG_ITEM_SIZE bytes");
          py::gil_scoped_release rel;
          return vali_jpeg_encode_rois((const vali_surface*)P(d_src), (const vali_jpeg_item*)it.ptr,
                                       (const vali_jpeg_item*)P(d_items), n, &j.p, P(workspace), ws_bytes,
                                       (uint8_t*)P(d_out), out_bytes, (uint32_t*)P(d_sizes), P(stream));
        });

  // the batch tensor the encoder reads: the arguments of TensorDst; vali_jpeg_encode_tensor judges it
  py::class_<TensorSrc>(m, "TensorSrc")
      .def(py::init([](uintptr_t data, int dtype, int packed, int n, int width, int height, int64_t stride_n,
                       int64_t stride_c, int64_t stride_y) {
        TensorSrc d;
        std::memset(&d.t, 0, sizeof(d.t));
        d.t.data = P(data);
        d.t.dtype = dtype; d.t.packed = packed;
        d.t.n = n; d.t.width = width; d.t.height = height;
        d.t.stride_n = stride_n; d.t.stride_c = stride_c; d.t.stride_y = stride_y;
        return d;
      }));
  m.attr("TENSOR_SRC_SIZE") = sizeof(vali_tensor_src);
  m.def("jpeg_encode_tensor",
        [](const TensorSrc& src, const std::array<float, 3>& scale, const std::array<float, 3>& offset,
           const JpegParams& j, uintptr_t workspace, size_t ws_bytes, uintptr_t d_out, size_t out_stride,
           uintptr_t d_sizes, uintptr_t stream) {
          return vali_jpeg_encode_tensor(&src.t, scale.data(), offset.data(), &j.p, P(workspace), ws_bytes,
                                         (uint8_t*)P(d_out), out_stride, (uint32_t*)P(d_sizes), P(stream));
        },
        py::call_guard<py::gil_scoped_release>());

  // the same tensor into 8-bit surfaces: d_dst is a device array of descriptors (descs_upload); params may be None for
  // RGB destinations
  m.def("tensor_to_surfaces",
        [](const TensorSrc& src, const std::array<float, 3>& scale, const std::array<float, 3>& offset, int bgr,
           uintptr_t d_dst, int dst_format, const CvtParams* p, uintptr_t stream) {
          return vali_tensor_to_surfaces(&src.t, scale.data(), offset.data(), bgr, (const vali_surface*)P(d_dst),
                                         dst_format, p ? &p->p : nullptr, P(stream));
        },
        py::call_guard<py::gil_scoped_release>());

  // marks on frames: descs = the host copy of the descriptors in d_frames; d_marks = device rows of 8 int32
  m.def("annotate_workspace_size", [](const std::vector<SurfaceDesc>& descs) {
    const std::vector<vali_surface> host = host_surfaces(descs);
    size_t bytes = 0;
    check(vali_annotate_workspace_size((int)host.size(), host.data(), &bytes), "vali_annotate_workspace_size");
    return bytes;
  });
  m.def("annotate_batch",
        [](const std::vector<SurfaceDesc>& descs, uintptr_t d_frames, int format, uintptr_t d_marks, int m,
           const CvtParams* p, uintptr_t workspace, size_t ws_bytes, uintptr_t stream, const SurfaceDesc* atlas) {
          const std::vector<vali_surface> host = host_surfaces(descs);
          py::gil_scoped_release nogil;
          return vali_annotate_batch_atlas(host.data(), (const vali_surface*)P(d_frames), (int)host.size(), format,
                                           (const vali_mark*)P(d_marks), m, atlas ? &atlas->s : nullptr,
                                           p ? &p->p : nullptr, P(workspace), ws_bytes, P(stream));
        },
        py::arg("descs"), py::arg("d_frames"), py::arg("format"), py::arg("d_marks"), py::arg("m"), py::arg("params"),
        py::arg("workspace"), py::arg("ws_bytes"), py::arg("stream"), py::arg("atlas") = py::none());

  // detections: boxes / scores = (ptr, dtype, stride_n, stride_k, stride_c); everything else as in the header
  m.def("detect_workspace_size", [](int n, int k, int max_candidates) {
    return vali_detect_workspace_size(n, k, max_candidates);
  });
  m.attr("DETECT_XYXY") = (int)VALI_DETECT_XYXY;
  m.attr("DETECT_CXCYWH") = (int)VALI_DETECT_CXCYWH;
  m.def("detect_select",
        [](const std::array<int64_t, 5>& boxes, const std::array<int64_t, 5>& scores, int n, int k, int c,
           int max_candidates, int max_det, float score_thr, float iou_thr, int class_agnostic, int box_format,
           const std::array<int32_t, 4>& crop, int thickness, int label_alpha, int text_colour, int n_colours,
           int n_labels, uintptr_t d_rects, uintptr_t dets, uintptr_t counts, uintptr_t rois, uintptr_t marks,
           uintptr_t colours, uintptr_t label_rects, uintptr_t workspace, size_t ws_bytes, uintptr_t stream) {
          vali_detect_in in;
          std::memset(&in, 0, sizeof(in));
          in.boxes = detect_tensor(boxes);
          in.scores = detect_tensor(scores);
          in.n = n; in.k = k; in.c = c;
          vali_detect_params p;
          std::memset(&p, 0, sizeof(p));
          p.max_candidates = max_candidates; p.max_det = max_det;
          p.score_thr = score_thr; p.iou_thr = iou_thr;
          p.class_agnostic = class_agnostic; p.box_format = box_format;
          for (int i = 0; i < 4; ++i)
            p.crop[i] = crop[i];
          p.thickness = thickness; p.label_alpha = label_alpha; p.text_colour = text_colour;
          p.n_colours = n_colours; p.n_labels = n_labels;
          vali_detect_out o;
          o.dets = (int32_t*)P(dets); o.counts = (int32_t*)P(counts); o.rois = (int32_t*)P(rois);
          o.marks = (int32_t*)P(marks);
          o.colours = (const int32_t*)P(colours); o.label_rects = (const int32_t*)P(label_rects);
          py::gil_scoped_release nogil;
          return vali_detect_select(&in, &p, (const vali_roi*)P(d_rects), &o, P(workspace), ws_bytes, P(stream));
        });

  // tracks: dims = (streams, frames per stream, max_det, max_tracks); everything else as in the header
  m.def("track_update",
        [](const std::array<int, 4>& dims, float iou_thr, float new_thr, float momentum, int min_hits, int max_age,
           int class_agnostic, int thickness, int label_alpha, int text_colour, int n_colours, int n_labels,
           uintptr_t dets, uintptr_t tracks, uintptr_t clock, uintptr_t tracked, uintptr_t assoc, uintptr_t marks,
           uintptr_t colours, uintptr_t label_rects, uintptr_t stream) {
          vali_track_params p;
          std::memset(&p, 0, sizeof(p));
          p.streams = dims[0]; p.frames = dims[1]; p.max_det = dims[2]; p.max_tracks = dims[3];
          p.iou_thr = iou_thr; p.new_thr = new_thr; p.momentum = momentum;
          p.min_hits = min_hits; p.max_age = max_age; p.class_agnostic = class_agnostic;
          p.thickness = thickness; p.label_alpha = label_alpha; p.text_colour = text_colour;
          p.n_colours = n_colours; p.n_labels = n_labels;
          vali_track_io io;
          io.dets = (const int32_t*)P(dets);
          io.tracks = (int32_t*)P(tracks); io.clock = (int32_t*)P(clock);
          io.tracked = (int32_t*)P(tracked); io.assoc = (int32_t*)P(assoc); io.marks = (int32_t*)P(marks);
          io.colours = (const int32_t*)P(colours); io.label_rects = (const int32_t*)P(label_rects);
          py::gil_scoped_release nogil;
          return vali_track_update(&p, &io, P(stream));
        });

  // instance masks: protos = (ptr, dtype, stride_n, stride_m, stride_y), coeffs = (ptr, dtype, stride_n, stride_k,
  // stride_m); descs = the host copy of the descriptors in d_frames; everything else as in the header
  m.def("mask_workspace_size", [](int n, int max_det, int hp, int wp) {
    return vali_mask_workspace_size(n, max_det, hp, wp);
  });
  m.def("mask_paint",
        [](const std::vector<SurfaceDesc>& descs, uintptr_t d_frames, int format, const std::array<int64_t, 5>& protos,
           const std::array<int64_t, 5>& coeffs, int mm, int hp, int wp, int k, int max_det, int net_w, int net_h,
           uintptr_t d_dets, uintptr_t d_rects, uintptr_t d_colours, int n_colours, int alpha, const CvtParams* p,
           uintptr_t workspace, size_t ws_bytes, uintptr_t stream) {
          const std::vector<vali_surface> host = host_surfaces(descs);
          vali_mask_in in;
          std::memset(&in, 0, sizeof(in));
          in.protos = mask_tensor(protos);
          in.coeffs = detect_tensor(coeffs);
          in.m = mm; in.hp = hp; in.wp = wp; in.k = k;
          in.max_det = max_det; in.net_w = net_w; in.net_h = net_h;
          py::gil_scoped_release nogil;
          return vali_mask_paint(host.empty() ? nullptr : host.data(), (const vali_surface*)P(d_frames), (int)host.size(),
                                 format, &in, (const int32_t*)P(d_dets), (const vali_roi*)P(d_rects),
                                 (const int32_t*)P(d_colours), n_colours, alpha, p ? &p->p : nullptr, P(workspace),
                                 ws_bytes, P(stream));
        });

  // semantic maps: logits = (ptr, dtype, stride_n, stride_c, stride_y); descs / labels = the host copies of the
  // descriptors in d_frames / d_labels (labels empty and d_labels 0: no label surfaces); d_colours 0: labels only
  m.def("semantic_paint",
        [](const std::vector<SurfaceDesc>& descs, uintptr_t d_frames, int format, const std::array<int64_t, 5>& logits,
           int c, int hs, int ws, int net_w, int net_h, uintptr_t d_rects, const std::vector<SurfaceDesc>& labels,
           uintptr_t d_labels, uintptr_t d_colours, int n_colours, int alpha, const CvtParams* p, uintptr_t stream) {
          const std::vector<vali_surface> host = host_surfaces(descs), lab = host_surfaces(labels);
          if (!lab.empty() && lab.size() != host.size())
            throw py::value_error("semantic_paint: as many label descriptors as frames, or none");
          vali_semantic_in in;
          std::memset(&in, 0, sizeof(in));
          in.logits = mask_tensor(logits);
          in.c = c; in.hs = hs; in.ws = ws; in.net_w = net_w; in.net_h = net_h;
          py::gil_scoped_release nogil;
          return vali_semantic_paint(host.empty() ? nullptr : host.data(), (const vali_surface*)P(d_frames),
                                     (int)host.size(), format, &in, (const vali_roi*)P(d_rects),
                                     lab.empty() ? nullptr : lab.data(), (const vali_surface*)P(d_labels),
                                     (const int32_t*)P(d_colours), n_colours, alpha, p ? &p->p : nullptr, P(stream));
        });

  // pose skeletons: kpts = (ptr, dtype, stride_n, stride_k, stride_p, stride_c); descs = the host copy of the descriptors
  // in d_frames; d_points may be 0 (the rows go to the workspace); everything else as in the header
  m.def("pose_workspace_size", [](int n, int max_det, int p) { return vali_pose_workspace_size(n, max_det, p); });
  m.def("pose_paint",
        [](const std::vector<SurfaceDesc>& descs, uintptr_t d_frames, int format, const std::array<int64_t, 6>& kpts,
           int kdim, int k, int pp, int max_det, uintptr_t d_limbs, int n_limbs, uintptr_t d_dets, uintptr_t d_rects,
           uintptr_t d_limb_colours, int n_limb_colours, uintptr_t d_joint_colours, int n_joint_colours, float kpt_thr,
           int thickness, int diameter, int alpha, uintptr_t d_points, const CvtParams* p, uintptr_t workspace,
           size_t ws_bytes, uintptr_t stream) {
          const std::vector<vali_surface> host = host_surfaces(descs);
          vali_pose_in in;
          std::memset(&in, 0, sizeof(in));
          fill_kpts(in, kpts, kdim);
          in.k = k; in.p = pp; in.max_det = max_det; in.n_limbs = n_limbs;
          in.d_limbs = (const int32_t*)P(d_limbs);
          vali_pose_style st;
          std::memset(&st, 0, sizeof(st));
          st.d_limb_colours = (const int32_t*)P(d_limb_colours);
          st.d_joint_colours = (const int32_t*)P(d_joint_colours);
          st.n_limb_colours = n_limb_colours; st.n_joint_colours = n_joint_colours;
          st.kpt_thr = kpt_thr;
          st.thickness = thickness; st.diameter = diameter; st.alpha = alpha;
          py::gil_scoped_release nogil;
          return vali_pose_paint(host.empty() ? nullptr : host.data(), (const vali_surface*)P(d_frames), (int)host.size(),
                                 format, &in, (const int32_t*)P(d_dets), (const vali_roi*)P(d_rects), &st,
                                 (int32_t*)P(d_points), p ? &p->p : nullptr, P(workspace), ws_bytes, P(stream));
        });

  // ... from the caller's points (d_points: n * max_det * p rows of 4 int32)
  m.def("pose_paint_points",
        [](const std::vector<SurfaceDesc>& descs, uintptr_t d_frames, int format, uintptr_t d_points, int pp, int max_det,
           uintptr_t d_limbs, int n_limbs, uintptr_t d_limb_colours, int n_limb_colours, uintptr_t d_joint_colours,
           int n_joint_colours, int thickness, int diameter, int alpha, const CvtParams* p, uintptr_t workspace,
           size_t ws_bytes, uintptr_t stream) {
          const std::vector<vali_surface> host = host_surfaces(descs);
          vali_pose_style st;
          std::memset(&st, 0, sizeof(st));
          st.d_limb_colours = (const int32_t*)P(d_limb_colours);
          st.d_joint_colours = (const int32_t*)P(d_joint_colours);
          st.n_limb_colours = n_limb_colours; st.n_joint_colours = n_joint_colours;
          st.thickness = thickness; st.diameter = diameter; st.alpha = alpha;
          py::gil_scoped_release nogil;
          return vali_pose_paint_points(host.empty() ? nullptr : host.data(), (const vali_surface*)P(d_frames),
                                        (int)host.size(), format, (const int32_t*)P(d_points), pp, max_det,
                                        (const int32_t*)P(d_limbs), n_limbs, &st, p ? &p->p : nullptr, P(workspace),
                                        ws_bytes, P(stream));
        });

  // keypoint decode: heat = (ptr, stride_m, stride_p, stride_y) or all zero; simcc = (x ptr, x stride_m, x stride_p,
  // y ptr, y stride_m, y stride_p) or all zero; dims = (m, p, hh, wh); one of d_matrices and d_rois is 0
  m.def("kpt_decode",
        [](uintptr_t d_frames, int n, int dtype, const std::array<int64_t, 4>& heat, const std::array<int64_t, 6>& simcc,
           const std::array<int, 4>& dims, int canvas_w, int canvas_h, int refine, int align, float kpt_thr, int max_det,
           uintptr_t d_matrices, uintptr_t d_rois, uintptr_t d_points, uintptr_t d_kpts, uintptr_t stream) {
          vali_kpt_decode_in in;
          std::memset(&in, 0, sizeof(in));
          in.heat = P((uintptr_t)heat[0]);
          in.stride_m = heat[1]; in.stride_p = heat[2]; in.stride_y = heat[3];
          in.simcc_x = P((uintptr_t)simcc[0]);
          in.x_stride_m = simcc[1]; in.x_stride_p = simcc[2];
          in.simcc_y = P((uintptr_t)simcc[3]);
          in.y_stride_m = simcc[4]; in.y_stride_p = simcc[5];
          in.dtype = dtype; in.refine = refine; in.align = align; in.max_det = max_det;
          in.m = dims[0]; in.p = dims[1]; in.hh = dims[2]; in.wh = dims[3];
          in.canvas_w = canvas_w; in.canvas_h = canvas_h;
          in.kpt_thr = kpt_thr;
          py::gil_scoped_release nogil;
          return vali_kpt_decode((const vali_surface*)P(d_frames), n, &in, (const int32_t*)P(d_matrices),
                                 (const vali_roi*)P(d_rois), (int32_t*)P(d_points), (float*)P(d_kpts), P(stream));
        });

  // aligned crops: kpts as for pose_paint; descs = the host copy of the descriptors in d_frames; everything else as in the
  // header
  m.def("warp_fit",
        [](uintptr_t d_frames, int n, const std::array<int64_t, 6>& kpts, int kdim, int k, int pp, int max_det,
           int min_points, uintptr_t d_template, float kpt_thr, uintptr_t d_dets, uintptr_t d_rects, uintptr_t d_matrices,
           uintptr_t stream) {
          vali_warp_fit_in in;
          std::memset(&in, 0, sizeof(in));
          fill_kpts(in, kpts, kdim);
          in.k = k; in.p = pp; in.max_det = max_det; in.min_points = min_points;
          in.d_template = (const float*)P(d_template);
          in.kpt_thr = kpt_thr;
          py::gil_scoped_release nogil;
          return vali_warp_fit((const vali_surface*)P(d_frames), n, &in, (const int32_t*)P(d_dets),
                               (const vali_roi*)P(d_rects), (int32_t*)P(d_matrices), P(stream));
        });
  m.def("warp_tensor",
        [](const std::vector<SurfaceDesc>& descs, uintptr_t d_frames, int format, uintptr_t d_matrices,
           const TensorDst* dst, const PreprocParams* p, bool pad, const std::array<uint8_t, 3>& pad_rgb,
           uintptr_t stream) {
          const std::vector<vali_surface> host = host_surfaces(descs);
          py::gil_scoped_release nogil;
          return vali_warp_tensor(host.empty() ? nullptr : host.data(), (const vali_surface*)P(d_frames), (int)host.size(),
                                  format, (const int32_t*)P(d_matrices), dst ? &dst->t : nullptr, p ? &p->p : nullptr,
                                  pad ? 1 : 0, pad_rgb.data(), P(stream));
        });

  // ---- JPEG decoder: host-side parser and sizes, then the batched decoder --------------------------------------
  py::class_<JpegInfo>(m, "JpegInfo")
      .def_property_readonly("width", [](const JpegInfo& j) { return j.f.width; })
      .def_property_readonly("height", [](const JpegInfo& j) { return j.f.height; })
      .def_property_readonly("components", [](const JpegInfo& j) { return j.f.components; })
      .def_property_readonly("h_samp", [](const JpegInfo& j) { return j.f.h_samp; })
      .def_property_readonly("v_samp", [](const JpegInfo& j) { return j.f.v_samp; })
      .def_property_readonly("restart_interval", [](const JpegInfo& j) { return j.f.restart_interval; })
      .def_property_readonly("segments", [](const JpegInfo& j) { return j.f.segments; })
      .def_property_readonly("mcux", [](const JpegInfo& j) { return j.f.mcux; })
      .def_property_readonly("mcuy", [](const JpegInfo& j) { return j.f.mcuy; })
      .def_property("data_offset", [](const JpegInfo& j) { return j.f.data_offset; },
                    [](JpegInfo& j, uint64_t v) { j.f.data_offset = v; })
      .def_property("data_len", [](const JpegInfo& j) { return j.f.data_len; },
                    [](JpegInfo& j, uint64_t v) { j.f.data_len = v; })
      .def_property_readonly("qtable", [](const JpegInfo& j) {
        std::vector<std::vector<int>> t(3, std::vector<int>(64));
        for (int c = 0; c < 3; ++c)
          for (int k = 0; k < 64; ++k)
            t[c][k] = j.f.qtable[c][k];
        return t;
      })
      .def("copy", [](const JpegInfo& j) { return j; })
      .def("tobytes", [](const JpegInfo& j) { return py::bytes((const char*)&j.f, sizeof(j.f)); });
  m.attr("JPEG_INFO_SIZE") = (int)sizeof(vali_jpeg_info);
  m.def("jpeg_parse", [](py::buffer b) {
    py::buffer_info info = b.request();
    JpegInfo j;
    check(vali_jpeg_parse((const uint8_t*)info.ptr, (size_t)(info.size * info.itemsize), &j.f), "vali_jpeg_parse");
    return j;
  });
  // the status code itself (no exception): for tests that feed arbitrary headers
  m.def("jpeg_parse_rc", [](py::buffer b) {
    py::buffer_info info = b.request();
    JpegInfo j;
    std::memset(&j.f, 0, sizeof(j.f));
    const int rc = vali_jpeg_parse((const uint8_t*)info.ptr, (size_t)(info.size * info.itemsize), &j.f);
    return py::make_tuple(rc, j);
  });
  m.def("jpeg_decode_workspace_size", [](const std::vector<JpegInfo>& infos) {
    std::vector<vali_jpeg_info> h(infos.size());
    for (size_t i = 0; i < infos.size(); ++i)
      h[i] = infos[i].f;
    size_t bytes = 0;
    check(vali_jpeg_decode_workspace_size(h.data(), (int)h.size(), &bytes), "vali_jpeg_decode_workspace_size");
    return bytes;
  });
  m.def("jpeg_decode_batch",
        [](const std::vector<JpegInfo>& infos, uintptr_t d_infos, uintptr_t d_data, int format, uintptr_t d_dst,
           uintptr_t workspace, size_t ws_bytes, uintptr_t d_status, uintptr_t stream) {
          std::vector<vali_jpeg_info> h(infos.size());
          for (size_t i = 0; i < infos.size(); ++i)
            h[i] = infos[i].f;
          py::gil_scoped_release rel;
          return vali_jpeg_decode_batch(h.data(), (const vali_jpeg_info*)P(d_infos), (int)h.size(),
                                        (const uint8_t*)P(d_data), format, (const vali_surface*)P(d_dst),
                                        P(workspace), ws_bytes, (int32_t*)P(d_status), P(stream));
        });

  m.def("ud_nv12",
        [](const SurfaceDesc& src, const SurfaceDesc& dst, uintptr_t stream) {
          return vali_ud_nv12(&src.s, &dst.s, P(stream));
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("ud_nv12_batch",
        [](uintptr_t d_src, uintptr_t d_dst, int n, int src_format, int src_w, int src_h, int dst_w,
           int dst_h, int dst_format, uintptr_t stream) {
          return vali_ud_nv12_batch((const vali_surface*)P(d_src), (const vali_surface*)P(d_dst),
                                    n, src_format, src_w, src_h, dst_w, dst_h, dst_format, P(stream));
        },
        py::call_guard<py::gil_scoped_release>());

  m.def("ud_nv12_rot",
        [](const SurfaceDesc& src, const SurfaceDesc& dst, int quarter_turns, uintptr_t stream) {
          return vali_ud_nv12_rot(&src.s, &dst.s, quarter_turns, P(stream));
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("ud_nv12_rot_batch",
        [](uintptr_t d_src, uintptr_t d_dst, int n, int src_format, int src_w, int src_h, int dst_w,
           int dst_h, int dst_format, int quarter_turns, uintptr_t stream) {
          return vali_ud_nv12_rot_batch((const vali_surface*)P(d_src), (const vali_surface*)P(d_dst),
                                        n, src_format, src_w, src_h, dst_w, dst_h, dst_format,
                                        quarter_turns, P(stream));
        },
        py::call_guard<py::gil_scoped_release>());

  m.def("resize",
        [](const SurfaceDesc& src, const SurfaceDesc& dst, int interp, uintptr_t stream) {
          return vali_resize(&src.s, &dst.s, interp, P(stream));
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("resize_batch",
        [](uintptr_t d_src, uintptr_t d_dst, int n, int format, int src_w, int src_h, int dst_w,
           int dst_h, int interp, uintptr_t stream) {
          return vali_resize_batch((const vali_surface*)P(d_src), (const vali_surface*)P(d_dst), n,
                                   format, src_w, src_h, dst_w, dst_h, interp, P(stream));
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("ud_planar",
        [](const SurfaceDesc& src, const SurfaceDesc& dst, int interp, uintptr_t stream) {
          return vali_ud_planar(&src.s, &dst.s, interp, P(stream));
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("ud_planar_batch",
        [](uintptr_t d_src, uintptr_t d_dst, int n, int src_format, int dst_format, int src_w, int src_h,
           int dst_w, int dst_h, int interp, uintptr_t stream) {
          return vali_ud_planar_batch((const vali_surface*)P(d_src), (const vali_surface*)P(d_dst), n,
                                      src_format, dst_format, src_w, src_h, dst_w, dst_h, interp, P(stream));
        },
        py::call_guard<py::gil_scoped_release>());
  m.attr("INTERP_LINEAR") = (int)VALI_INTERP_LINEAR;
  m.attr("INTERP_CUBIC") = (int)VALI_INTERP_CUBIC;
  m.attr("INTERP_LANCZOS") = (int)VALI_INTERP_LANCZOS;

  m.def("rotate",
        [](const SurfaceDesc& src, const SurfaceDesc& dst, double angle, double shx, double shy,
           int per_plane, uintptr_t stream) {
          return vali_rotate(&src.s, &dst.s, angle, shx, shy, per_plane, P(stream));
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("rotate_batch",
        [](uintptr_t d_src, uintptr_t d_dst, int n, int format, int sw, int sh, int dw, int dh,
           double angle, double shx, double shy, int per_plane, uintptr_t stream) {
          return vali_rotate_batch((const vali_surface*)P(d_src), (const vali_surface*)P(d_dst), n,
                                   format, sw, sh, dw, dh, angle, shx, shy, per_plane, P(stream));
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("rotate_coeffs", [](double angle) {
    float c = 0, s = 0;
    check(vali_rotate_coeffs(angle, &c, &s), "vali_rotate_coeffs");
    return py::make_tuple(c, s);
  });

  m.def("debug_quantize_u8", [](uintptr_t in, uintptr_t out, int n, uintptr_t stream) {
    return vali_debug_quantize_u8((const float*)P(in), (uint8_t*)P(out), n, P(stream));
  });
  m.def("debug_quantize_u8_portable", [](uintptr_t in, uintptr_t out, int n, uintptr_t stream) {
    return vali_debug_quantize_u8_portable((const float*)P(in), (uint8_t*)P(out), n, P(stream));
  });

  m.def("dlpack_export", &dlpack_export, py::arg("ptr"), py::arg("shape"), py::arg("strides"),
        py::arg("code"), py::arg("bits"), py::arg("device_type"), py::arg("device_id"),
        py::arg("owner"));
  m.def("dlpack_import", &dlpack_import);
}
