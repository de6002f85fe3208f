"""The fused preprocessor into ONE batch tensor (float32 / float16 / bfloat16), host side (no GPU): the C declarations
and argument checks of vali_nv12_preproc_roi_tensor / vali_rgb_preproc_roi_tensor, the stride classifier as a pure
function, and what PrepareTensorBatch refuses before it touches a device."""
import ctypes
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_header_declares_tensor_entry_points(tmp_path):
    tu = tmp_path / "tu.c"
    tu.write_text(
        '#include <stddef.h>\n#include "vali_hip.h"\n'
        "int main(void) {\n"
        "  int (*nv12)(const vali_surface*, const vali_roi*, const vali_tensor_dst*, const vali_preproc_params*, int,\n"
        "              const uint8_t*, vali_stream_t) = vali_nv12_preproc_roi_tensor;\n"
        "  int (*rgb)(const vali_surface*, const vali_roi*, int, const vali_tensor_dst*, const vali_preproc_params*, int,\n"
        "             const uint8_t*, vali_stream_t) = vali_rgb_preproc_roi_tensor;\n"
        "  (void)nv12; (void)rgb;\n"
        "  return sizeof(vali_tensor_dst) == 56 && offsetof(vali_tensor_dst, dtype) == 8 &&\n"
        "         offsetof(vali_tensor_dst, stride_n) == 32 && offsetof(vali_tensor_dst, stride_y) == 48 &&\n"
        "         VALI_DTYPE_F32 == 0 && VALI_DTYPE_F16 == 1 && VALI_DTYPE_BF16 == 2 ? 0 : 1;\n"
        "}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", "-c",
                    str(tu), "-o", str(tmp_path / "tu.o")], check=True)
    # compile-only above (no library needed); the size check itself runs as a host program
    subprocess.run(["gcc", "-std=c99", f"-I{ROOT / 'include'}", str(tu), "-o", str(tmp_path / "tu"),
                    "-Wl,--unresolved-symbols=ignore-all"], check=True)
    assert subprocess.run([str(tmp_path / "tu")]).returncode == 0


class _TensorDst(ctypes.Structure):
    """include/vali_hip.h: vali_tensor_dst"""
    _fields_ = [("data", ctypes.c_void_p), ("dtype", ctypes.c_int32), ("packed", ctypes.c_int32), ("n", ctypes.c_int32),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("stride_n", ctypes.c_int64), ("stride_c", ctypes.c_int64), ("stride_y", ctypes.c_int64)]


def test_shim_tensor_dst_size(vali):
    from vali_amd._native import shim

    assert shim.TENSOR_DST_SIZE == 56 == ctypes.sizeof(_TensorDst)
    assert (shim.DTYPE_F32, shim.DTYPE_F16, shim.DTYPE_BF16) == (0, 1, 2)


def test_library_checks_tensor_arguments_without_a_gpu(vali):
    """Every refusal is decided before any HIP call: the pointers below are dummies that are never read."""
    lib = ctypes.CDLL(str(ROOT / "vali_amd" / "libvali_hip.so"))
    lib.vali_last_error.restype = ctypes.c_char_p
    params = (ctypes.c_float * 16)()
    buf = ctypes.create_string_buffer(64)
    base = ctypes.addressof(buf)
    assert base % 8 == 0
    d_any = ctypes.c_void_p(base)
    pad_rgb = (ctypes.c_uint8 * 3)(1, 2, 3)
    RGB = int(vali.RGB)

    def dst(**kw):
        t = _TensorDst()
        t.data, t.dtype, t.packed, t.n, t.width, t.height = base, 1, 0, 2, 32, 16
        t.stride_n, t.stride_c, t.stride_y = 3 * 16 * 32, 16 * 32, 32
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    def nv12(t, src=d_any, prm=params, pad=0, colour=None):
        return lib.vali_nv12_preproc_roi_tensor(src, None, ctypes.byref(t) if t is not None else None, prm, pad, colour,
                                                None)

    def rgb(t, fmt=RGB, src=d_any, prm=params, pad=0, colour=None):
        return lib.vali_rgb_preproc_roi_tensor(src, None, fmt, ctypes.byref(t) if t is not None else None, prm, pad,
                                               colour, None)

    # null arguments
    for call in (nv12, rgb):
        for kw in ({"src": None}, {"prm": None}):
            assert call(dst(), **kw) == -1
            assert b"null" in lib.vali_last_error()
        assert call(None) == -1
        assert b"null" in lib.vali_last_error()
        assert call(dst(data=None)) == -1
        assert b"null" in lib.vali_last_error()
    # source formats of the RGB entry: judged before the tensor
    for bad in (vali.NV12, vali.YUV420, vali.Y):
        assert rgb(dst(), fmt=int(bad)) == -2
        assert rgb(dst(dtype=3), fmt=int(bad)) == -2
    bad_dst = [dict(dtype=3), dict(dtype=-1), dict(packed=2), dict(packed=-1), dict(n=0), dict(n=65536),
               dict(stride_n=0), dict(stride_n=-1536), dict(stride_c=0), dict(stride_c=-512), dict(stride_y=0),
               dict(stride_y=-32), dict(stride_y=31), dict(packed=1, stride_y=95), dict(width=0), dict(height=0),
               dict(data=base + 1),                                    # an odd address with a 2-byte dtype
               dict(dtype=0, data=base + 2),                           # ... and a float32 one that is only 2-aligned
               dict(dtype=0, stride_y=1 << 29),                        # a row pitch of 2 GiB
               dict(height=4096, stride_y=1 << 19, stride_c=1 << 31, stride_n=1 << 33)]    # a plane of 4 GiB
    for kw in bad_dst:
        for call in (nv12, rgb):
            assert call(dst(**kw)) == -1, kw
    # NV12: an odd canvas; the RGB family takes it (and then needs a device, which is not asked for here)
    for kw in (dict(width=31), dict(height=15), dict(width=1, stride_y=2), dict(height=1)):
        assert nv12(dst(**kw)) == -1, kw
    # stride_c is ignored when packed
    t = dst(packed=1, stride_c=0, stride_y=95)
    assert nv12(t) == -1 and b"stride_y" in lib.vali_last_error()
    # pad without a colour
    assert nv12(dst(), pad=1) == -1 and b"pad" in lib.vali_last_error()
    assert rgb(dst(), pad=1) == -1 and b"pad" in lib.vali_last_error()
    assert pad_rgb[0] == 1


CONTIG = (2, 3, 8, 10)


def _contiguous(shape):
    n, c, h, w = shape
    return (c * h * w, h * w, w, 1)


def _channels_last(shape):
    n, c, h, w = shape
    return (h * w * c, 1, w * c, c)


def test_stride_classifier_planar_and_packed():
    from vali_amd.tasks import tensor_layout

    assert tensor_layout(CONTIG, _contiguous(CONTIG), 2, 32) == ("planar", "float32")
    assert tensor_layout(CONTIG, None, 2, 16) == ("planar", "float16")
    assert tensor_layout(CONTIG, _contiguous(CONTIG), 4, 16) == ("planar", "bfloat16")
    assert tensor_layout(CONTIG, _channels_last(CONTIG), 2, 16) == ("packed", "float16")
    # [:, :, 1:7, 1:9] of a larger tensor keeps the strides of the larger one
    view = (2, 3, 6, 8)
    assert tensor_layout(view, _contiguous(CONTIG), 2, 16)[0] == "planar"
    assert tensor_layout(view, _channels_last(CONTIG), 4, 16)[0] == "packed"
    # [::2]
    sn, sc, sy, sx = _contiguous((4, 3, 8, 10))
    assert tensor_layout(CONTIG, (2 * sn, sc, sy, sx), 2, 32)[0] == "planar"
    sn, sc, sy, sx = _channels_last((4, 3, 8, 10))
    assert tensor_layout(CONTIG, (2 * sn, sc, sy, sx), 2, 32)[0] == "packed"


def test_stride_classifier_agrees_with_torch():
    import torch
    from vali_amd.tasks import tensor_layout

    for dtype, code, bits in ((torch.float32, 2, 32), (torch.float16, 2, 16), (torch.bfloat16, 4, 16)):
        t = torch.empty(CONTIG, dtype=dtype)
        big = torch.empty((4, 3, 10, 12), dtype=dtype)
        for x in (t, big[:, :, 1:7, 1:9], big[::2]):
            assert tensor_layout(x.shape, x.stride(), code, bits)[0] == "planar"
        t = t.contiguous(memory_format=torch.channels_last)
        big = big.contiguous(memory_format=torch.channels_last)
        for x in (t, big[:, :, 1:7, 1:9], big[::2]):
            assert tensor_layout(x.shape, x.stride(), code, bits)[0] == "packed"


@pytest.mark.parametrize("shape, strides, code, bits, what", [
    ((2, 3, 10, 8), (240, 80, 1, 10), 2, 32, "transposed"),              # .transpose(2, 3) of a contiguous tensor
    ((2, 3, 10, 8), (240, 1, 3, 30), 2, 16, "transposed"),               # ... of a channels-last one
    ((2, 3, 8, 10), (240, 80, 10, -1), 2, 32, "negative"),               # flipped along x
    ((2, 3, 8, 10), (240, 80, -10, 1), 2, 32, "negative"),
    ((2, 3, 8, 10), (240, 80, 10, 2), 2, 32, "strided"),                 # [..., ::2]
    ((2, 3, 8, 10), (240, 80, 0, 1), 2, 32, "overlap"),                  # a row broadcast over y
    ((3, 8, 10), (80, 10, 1), 2, 32, "4-D"),
    ((2, 4, 8, 10), (320, 80, 10, 1), 2, 32, "C = 4"),
    ((2, 3, 8, 10), (240, 80, 10, 1), 2, 64, "dtype"),                   # float64
    ((2, 3, 8, 10), (240, 80, 10, 1), 0, 8, "dtype"),                    # int8
    ((2, 3, 8, 10), (240, 80, 10, 1), 0, 32, "dtype"),                   # int32
    ((2, 3, 8, 10), (240, 80, 10, 1), 1, 16, "dtype"),                   # uint16
    ((65536, 3, 2, 2), (12, 4, 2, 1), 2, 32, "65535"),
])
def test_stride_classifier_names_what_is_wrong(shape, strides, code, bits, what):
    from vali_amd.tasks import tensor_layout

    with pytest.raises(ValueError, match=what):
        tensor_layout(shape, strides, code, bits)


class _FakeSurface:
    """what TensorBatch reads of a Surface before it touches a device"""

    def __init__(self, fmt, w, h):
        self.Format, self.Width, self.Height, self.IsEmpty = fmt, w, h, False


class _FlippedDeviceArray:
    """a device array seen through __cuda_array_interface__ with a negative x stride (never dereferenced)"""
    __cuda_array_interface__ = {"shape": (2, 3, 8, 10), "typestr": "<f4", "data": (4096, False), "version": 3,
                                "strides": (960, 320, 40, -4)}


def _task(vali):
    """a preprocessor without its device-side parts: everything below is refused before one is needed"""
    pre = object.__new__(vali.PySurfacePreprocessor)
    pre._gpu_id, pre._stream = 0, 0
    return pre


def test_prepare_tensor_batch_refuses_malformed_tensors(vali):
    import torch

    pre = _task(vali)
    srcs = [_FakeSurface(vali.NV12, 64, 48), _FakeSurface(vali.NV12, 128, 96)]
    good = torch.empty(CONTIG, dtype=torch.float16)
    for out, what in ((good.transpose(2, 3), "transposed"),
                      (_FlippedDeviceArray(), "negative"),
                      (torch.empty((3, 8, 10), dtype=torch.float16), "4-D"),
                      (torch.empty((2, 4, 8, 10), dtype=torch.float16), "C = 4"),
                      (torch.empty(CONTIG, dtype=torch.float64), "dtype"),
                      (torch.empty(CONTIG, dtype=torch.int8), "dtype"),
                      (torch.empty(CONTIG, dtype=torch.int32), "dtype"),
                      (good, "GPU"),                                            # a CPU tensor
                      (good.contiguous(memory_format=torch.channels_last), "GPU"),
                      (object(), "__dlpack__")):
        with pytest.raises(ValueError, match=what):
            pre.PrepareTensorBatch(srcs, out)


def test_run_tensor_batch_wants_a_tensor_batch(vali):
    pre = _task(vali)
    with pytest.raises(ValueError, match="TensorBatch"):
        pre.RunTensorBatchAsync(object())


def test_the_public_surface_is_otherwise_unchanged(vali):
    import python_vali

    pairs = vali.PySurfacePreprocessor.SupportedFormats()
    srcs = (vali.NV12, vali.RGB, vali.BGR, vali.RGB_PLANAR)
    dsts = (vali.RGB_32F_PLANAR, vali.RGB_32F, vali.RGB, vali.BGR, vali.RGB_PLANAR)
    assert sorted((int(s), int(d)) for s, d in pairs) == sorted((int(s), int(d)) for s in srcs for d in dsts)
    assert python_vali.PySurfacePreprocessor.SupportedFormats() == pairs
    for name in ("PrepareTensorBatch", "RunTensorBatch", "RunTensorBatchAsync"):
        assert callable(getattr(python_vali.PySurfacePreprocessor, name))
    assert python_vali.TensorBatch is vali.TensorBatch
