"""PySurfacePostprocessor / vali_tensor_to_surfaces, host side (no GPU): the model against its independent restatement,
the BT.709 constants, the C declaration and every refusal the library and the Python class make before a device is
touched."""
import ctypes
import shutil
import subprocess
import types
from pathlib import Path

import numpy as np
import pytest

import postproc_model as pm

ROOT = Path(__file__).resolve().parent.parent


# ---- the model --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(2, 2), (6, 4), (34, 18)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["601_JPEG", "601_MPEG", "709_JPEG", "709_MPEG"])
def test_oracle_equals_the_words_of_the_definition(vali, oracle, name, size):
    w, h = size
    rows = pm.matrices()[name]
    for p in (pm.lattice(w, h), pm.noise(w, h, seed=w * 100 + h)):
        for dst in ("YUV444", "YUV420", "NV12"):
            want = pm.numpy_yuv(p, rows, dst)
            got = pm.from_rgb(oracle, p, dst, rows)
            assert got.shape == want.shape
            assert np.array_equal(got, want), (name, dst, size, np.flatnonzero(got != want)[:5])


def test_model_rgb_destinations_are_the_bytes(vali, oracle):
    p = pm.noise(7, 5, seed=1)
    assert np.array_equal(pm.from_rgb(oracle, p, "RGB", None), p.reshape(-1))
    planar = pm.from_rgb(oracle, p, "RGB_PLANAR", None).reshape(3, 5, 7)
    for c in range(3):
        assert np.array_equal(planar[c], p[..., c])


def test_model_quantiser_names_channels_after_scaling(vali):
    """scale and offset belong to the tensor's channels; BGR only renames them afterwards"""
    bits = np.array([[[10, 20, 30]]], np.uint8)
    scale, offset = (1.0, 2.0, 3.0), (0.0, 1.0, 2.0)
    assert pm.quantise(bits, "uint8", scale, offset, "RGB").tolist() == [[[10, 41, 92]]]
    assert pm.quantise(bits, "uint8", scale, offset, "BGR").tolist() == [[[92, 41, 10]]]


def test_chroma_rounding_matrix_lands_on_ties(vali, oracle):
    """the matrix of the GPU test that makes chroma rounding visible: every 2 x 2 mean of U is k / 4 + 0.5 and of V is
    k / 4 + 0.25, so ties (U) and their neighbours (V) are met, and the oracle rounds them half to even"""
    rows = ((0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.5), (1.0, 0.0, 0.0, 0.25))
    p = pm.noise(34, 18, seed=3)
    got = pm.from_rgb(oracle, p, "YUV420", rows)
    assert np.array_equal(got, pm.numpy_yuv(p, rows, "YUV420"))
    b = p[..., 2].astype(np.int64)
    s = b[0::2, 0::2] + b[0::2, 1::2] + b[1::2, 0::2] + b[1::2, 1::2]
    ties = (s % 4) == 0                                  # mean + 0.5 is k + 0.5 exactly
    assert ties.sum() > 20
    u = pm.planes_of("YUV420", got, 34, 18)[1]
    k = (s // 4)[ties]
    assert np.array_equal(u[ties], np.minimum(k + (k % 2), 255))      # k + 0.5 -> the even one of k, k + 1


# ---- the BT.709 constants ---------------------------------------------------------------------------------------------
def test_bt709_constants():
    from vali_amd import tasks

    kr, kb = 0.2126, 0.0722
    kg = 1 - kr - kb
    full = [(kr, kg, kb, 0.0), (-kr / (2 * (1 - kb)), -kg / (2 * (1 - kb)), 0.5, 128.0),
            (0.5, -kg / (2 * (1 - kr)), -kb / (2 * (1 - kr)), 128.0)]
    mpeg = [tuple(v * 219 / 255 for v in full[0][:3]) + (16.0,)] + [tuple(v * 224 / 255 for v in r[:3]) + (128.0,)
                                                                     for r in full[1:]]
    for have, want, ysum in ((tasks.RGB2YUV_BT709_JPEG, full, 1.0), (tasks.RGB2YUV_BT709_MPEG, mpeg, 219 / 255)):
        assert len(have) == 3 and all(len(r) == 4 for r in have)
        for hr, wr in zip(have, want):
            for a, b in zip(hr, wr):
                assert a == float(np.float32(b)), (a, b)            # rounded to float32 once
        assert abs(sum(have[0][:3]) - ysum) < 1e-7
        for k in (1, 2):
            assert abs(sum(have[k][:3])) < 1e-7
    # the header writes the numbers out
    text = (ROOT / "include" / "vali_hip.h").read_text()
    for m in (tasks.RGB2YUV_BT709_JPEG, tasks.RGB2YUV_BT709_MPEG):
        for row in m:
            for v in row[:3]:
                assert repr(abs(v)) in text, v


def test_cc_ctx_selects_the_matrix(vali):
    from vali_amd import tasks

    M = vali.PySurfacePostprocessor.Matrix
    C, S, R = vali.ColorspaceConversionContext, vali.ColorSpace, vali.ColorRange
    assert M(None) is tasks.RGB2YUV_NPP_YUV
    assert M(C(S.BT_601, R.JPEG)) is tasks.RGB2YUV_NPP_YUV
    assert M(C(S.BT_601, R.MPEG)) is tasks.RGB2YUV_NPP_YCBCR
    assert M(C(S.BT_709, R.JPEG)) is tasks.RGB2YUV_BT709_JPEG
    assert M(C(S.BT_709, R.MPEG)) is tasks.RGB2YUV_BT709_MPEG
    assert M(C(S.BT_709, R.UDEF)) is None and M(C(S.UNSPEC, R.JPEG)) is None and M(C()) is None


# ---- C ABI ------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported():
    lib = ctypes.CDLL(str(ROOT / "vali_amd" / "libvali_hip.so"))
    assert hasattr(lib, "vali_tensor_to_surfaces")


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_header_declares_the_entry_point(tmp_path):
    tu = tmp_path / "tu.c"
    tu.write_text(
        '#include <stddef.h>\n#include "vali_hip.h"\n'
        "int main(void) {\n"
        "  int (*f)(const vali_tensor_src*, const float*, const float*, int, const vali_surface*, int,\n"
        "           const vali_cvt_params*, vali_stream_t) = vali_tensor_to_surfaces;\n"
        "  (void)f;\n"
        "  return 0;\n"
        "}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", "-c",
                    str(tu), "-o", str(tmp_path / "tu.o")], check=True)


class _TensorSrc(ctypes.Structure):
    """include/vali_hip.h: vali_tensor_src"""
    _fields_ = [("data", ctypes.c_void_p), ("dtype", ctypes.c_int32), ("packed", ctypes.c_int32), ("n", ctypes.c_int32),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("stride_n", ctypes.c_int64), ("stride_c", ctypes.c_int64), ("stride_y", ctypes.c_int64)]


def test_library_refuses_without_a_gpu(vali):
    """Every refusal is decided before any HIP call: the pointers below are dummies that are never read."""
    lib = ctypes.CDLL(str(ROOT / "vali_amd" / "libvali_hip.so"))
    lib.vali_last_error.restype = ctypes.c_char_p
    buf = ctypes.create_string_buffer(64)
    base = ctypes.addressof(buf)
    assert base % 8 == 0
    d_any = ctypes.c_void_p(base)
    params = (ctypes.c_float * 20)()
    ones, zeros = (ctypes.c_float * 3)(255, 255, 255), (ctypes.c_float * 3)(0, 0, 0)
    NV12, YUV420, YUV444, RGB, RGBP = (int(getattr(vali, f)) for f in ("NV12", "YUV420", "YUV444", "RGB", "RGB_PLANAR"))

    def src(**kw):
        t = _TensorSrc()
        t.data, t.dtype, t.packed, t.n, t.width, t.height = base, 1, 0, 2, 32, 16
        t.stride_n, t.stride_c, t.stride_y = 3 * 16 * 32, 16 * 32, 32
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    def call(t, scale=ones, offset=zeros, bgr=0, dst=d_any, fmt=NV12, prm=params):
        return lib.vali_tensor_to_surfaces(ctypes.byref(t) if t is not None else None, scale, offset, bgr, dst, fmt,
                                           prm, None)

    def refused(rc, code=-1):
        assert rc == code, (rc, lib.vali_last_error())
        assert len(lib.vali_last_error()) > 10 and b"vali_tensor_to_surfaces" in lib.vali_last_error()

    # null arguments
    refused(call(None))
    for kw in (dict(scale=None), dict(offset=None), dict(dst=None)):
        refused(call(src(), **kw))
        assert b"null" in lib.vali_last_error()
    refused(call(src(data=None)))
    # params: needed by the YUV destinations only (an RGB call with everything right would go on to the device, so
    # the RGB cases here carry another fault and must be refused for THAT)
    for fmt in (NV12, YUV420, YUV444):
        refused(call(src(), fmt=fmt, prm=None))
        assert b"params" in lib.vali_last_error()
    for fmt in (RGB, RGBP):
        refused(call(src(), fmt=fmt, prm=None, bgr=2))
        assert b"bgr" in lib.vali_last_error()
    # what vali_jpeg_encode_tensor refuses in src
    bad_src = [dict(dtype=4), dict(dtype=-1), dict(packed=2), dict(packed=-1), dict(n=0), dict(n=65536),
               dict(stride_n=0), dict(stride_n=-1536), dict(stride_c=0), dict(stride_c=-512), dict(stride_y=0),
               dict(stride_y=-32), dict(stride_y=31), dict(packed=1, stride_y=95), dict(width=0), dict(height=0),
               dict(width=65536, stride_y=65536), dict(height=65536),
               dict(data=base + 1), dict(dtype=0, data=base + 2)]
    for kw in bad_src:
        for fmt in (NV12, RGB):
            refused(call(src(**kw), fmt=fmt))
    # ... and in scale and offset
    for bad in (float("nan"), float("inf"), float("-inf")):
        for c in range(3):
            v = (ctypes.c_float * 3)(1, 1, 1)
            v[c] = bad
            refused(call(src(), scale=v))
            assert b"finite" in lib.vali_last_error()
            refused(call(src(), offset=v))
    # bgr
    for bgr in (-1, 2, 255):
        refused(call(src(), bgr=bgr))
    # an odd size for a 4:2:0 destination
    for kw in (dict(width=31), dict(height=15), dict(width=1, stride_y=2), dict(height=1)):
        for fmt in (NV12, YUV420):
            refused(call(src(**kw), fmt=fmt))
            assert b"even" in lib.vali_last_error()
    # every other destination format
    for name in ("UNDEFINED", "Y", "BGR", "RGB_32F", "RGB_32F_PLANAR", "YUV422", "P10", "P12", "YUV444_10bit",
                 "YUV420_10bit", "GRAY12"):
        refused(call(src(), fmt=int(getattr(vali, name))), code=-2)
    refused(call(src(), fmt=99), code=-2)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_loader_table_tests_still_see_the_header():
    """tests/test_cpp_loader_table.py and tests/test_c_abi_header.py read the header: the new declaration is plain C"""
    text = (ROOT / "include" / "vali_hip.h").read_text()
    assert text.count("vali_tensor_to_surfaces(") == 1
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c",
                        str(ROOT / "include" / "vali_hip.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- Python -----------------------------------------------------------------------------------------------------------
class _FakeSurface:
    """what FrameBatch reads of a Surface before it touches a device"""

    def __init__(self, fmt, w, h, empty=False, device=0):
        self.Format, self.Width, self.Height, self.IsEmpty, self.DeviceId = fmt, w, h, empty, device


class _DeviceArray:
    """a (2, 3, 8, 10) float16 device array on GPU 0 seen through __cuda_array_interface__ (never dereferenced)"""
    device = types.SimpleNamespace(type="cuda", index=0)

    def __init__(self, shape=(2, 3, 8, 10), typestr="<f2"):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (4096, False), "version": 3}


def _task(vali):
    """a postprocessor without its device-side parts: everything below is refused before one is needed"""
    post = object.__new__(vali.PySurfacePostprocessor)
    post._gpu_id, post._stream = 0, 0
    return post


def test_prepare_refuses_surfaces_that_do_not_fit(vali):
    post = _task(vali)
    t = _DeviceArray()
    S = _FakeSurface
    good = [S(vali.NV12, 10, 8), S(vali.NV12, 10, 8)]
    for dsts, what in (([S(vali.BGR, 10, 8), S(vali.BGR, 10, 8)], "surface 0 has format"),          # wrong format
                       ([S(vali.NV12, 10, 8), S(vali.RGB_32F, 10, 8)], "surface 1 has format"),
                       ([S(vali.NV12, 10, 8), S(vali.NV12, 12, 8)], "surface 1 is 12x8"),          # wrong size
                       ([S(vali.RGB, 10, 8), S(vali.RGB, 10, 6)], "surface 1 is 10x6"),
                       (good[:1], "1 surfaces for a tensor of 2"),                                # wrong count
                       (good + good[:1], "3 surfaces for a tensor of 2"),
                       ([], "0 surfaces"),
                       ([S(vali.NV12, 10, 8), S(vali.NV12, 10, 8, empty=True)], "surface 1 is empty"),
                       ([good[0], None], "surface 1 is empty"),
                       ([S(vali.NV12, 10, 8), S(vali.YUV420, 10, 8)], "one format per batch"),    # mixed formats
                       ([S(vali.RGB, 10, 8), S(vali.RGB_PLANAR, 10, 8)], "one format per batch"),
                       ([S(vali.NV12, 10, 8), S(vali.NV12, 10, 8, device=1)], "device 1")):
        with pytest.raises(ValueError, match=what):
            post.PrepareTensorBatch(t, dsts)
    # an odd size for a 4:2:0 destination; the others take it
    odd = _DeviceArray((1, 3, 7, 10))
    for fmt in (vali.NV12, vali.YUV420):
        with pytest.raises(ValueError, match="even"):
            post.PrepareTensorBatch(odd, [S(fmt, 10, 7)])
        with pytest.raises(ValueError, match="even"):
            post.PrepareTensorBatch(_DeviceArray((1, 3, 8, 9)), [S(fmt, 9, 8)])


def test_prepare_refuses_what_is_no_tensor_of_this_gpu(vali):
    import torch

    post = _task(vali)
    dsts = [_FakeSurface(vali.NV12, 10, 8), _FakeSurface(vali.NV12, 10, 8)]
    good = torch.empty((2, 3, 8, 10), dtype=torch.float16)
    other = _DeviceArray()
    other.device = types.SimpleNamespace(type="cuda", index=1)
    for t, what in ((good, "GPU"),                                                     # a CPU tensor
                    (good.contiguous(memory_format=torch.channels_last), "GPU"),
                    (other, "device 1"),
                    (good.transpose(2, 3), "transposed"),
                    (torch.empty((2, 4, 8, 10), dtype=torch.float16), "C = 4"),
                    (torch.empty((2, 3, 8, 10), dtype=torch.float64), "dtype"),
                    (torch.empty((2, 3, 8, 10), dtype=torch.int32), "dtype"),
                    (object(), "__dlpack__")):
        with pytest.raises(ValueError, match=what):
            post.PrepareTensorBatch(t, dsts)


def test_run_refuses_bad_arguments(vali):
    post = _task(vali)
    with pytest.raises(ValueError, match="FrameBatch"):
        post.RunTensorBatchAsync(object())
    fb = object.__new__(vali.FrameBatch)                 # never reaches the device: the arguments are judged first
    fb.dtype, fb.dst_format = "float16", vali.NV12
    for channels in ("GRB", "rgb", "", None, "RGBA"):
        with pytest.raises(ValueError, match="channels"):
            post.RunTensorBatchAsync(fb, channels=channels)
    for kw in (dict(scale=float("nan")), dict(scale=(255.0, float("inf"), 255.0)), dict(offset=float("-inf")),
               dict(scale=1e39), dict(offset=(0.0, float("nan"), 0.0))):
        with pytest.raises(ValueError, match="finite"):
            post.RunTensorBatchAsync(fb, **kw)
    for kw in (dict(scale=(1.0, 2.0)), dict(offset="x"), dict(scale=[[1.0]])):
        with pytest.raises(ValueError, match="three numbers"):
            post.RunTensorBatchAsync(fb, **kw)
    # an unsupported colour context: the converter's status, and nothing is launched (fb has no device parts)
    C, S, R = vali.ColorspaceConversionContext, vali.ColorSpace, vali.ColorRange
    for cc in (C(S.BT_709, R.UDEF), C(S.UNSPEC, R.JPEG), C()):
        assert post.RunTensorBatchAsync(fb, cc_ctx=cc) == (False, vali.TaskExecInfo.UNSUPPORTED_FMT_CONV_PARAMS)


def test_public_surface(vali):
    import python_vali

    fmts = vali.PySurfacePostprocessor.SupportedFormats()
    assert fmts == [vali.NV12, vali.YUV420, vali.YUV444, vali.RGB, vali.RGB_PLANAR]
    assert python_vali.PySurfacePostprocessor is vali.PySurfacePostprocessor
    assert python_vali.FrameBatch is vali.FrameBatch
    for name in ("PrepareTensorBatch", "RunTensorBatch", "RunTensorBatchAsync", "SupportedFormats"):
        assert callable(getattr(python_vali.PySurfacePostprocessor, name))
    # the preprocessor's table is what it was
    pairs = vali.PySurfacePreprocessor.SupportedFormats()
    srcs = (vali.NV12, vali.RGB, vali.BGR, vali.RGB_PLANAR)
    dsts = (vali.RGB_32F_PLANAR, vali.RGB_32F, vali.RGB, vali.BGR, vali.RGB_PLANAR)
    assert sorted((int(s), int(d)) for s, d in pairs) == sorted((int(s), int(d)) for s in srcs for d in dsts)
