"""JPEG straight from a float32 / float16 / bfloat16 / uint8 tensor, host side (no GPU): the numpy model of the quantiser
(tests/jpeg_tensor_model.py) against the torch chain it replaces, the layout helper as a pure function, and the C
declarations and argument checks of vali_jpeg_encode_tensor."""
import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jpeg_tensor_model as tm

ROOT = Path(__file__).resolve().parent.parent


# ---- the quantiser ------------------------------------------------------------------------------------------------------
def _inputs(dtype):
    if dtype == "float32":
        return tm.float32_edges().view(np.uint32)
    return tm.all_patterns(dtype)


@pytest.mark.parametrize("pair", range(len(tm.SCALE_OFFSETS)))
@pytest.mark.parametrize("dtype", ["float16", "bfloat16", "float32"])
def test_model_equals_the_torch_chain(dtype, pair):
    """every float16 / bfloat16 bit pattern, and the float32 edge set, in each of the three channels"""
    scale, offset = tm.SCALE_OFFSETS[pair]
    bits = np.repeat(_inputs(dtype)[:, None], 3, axis=1)            # (K, 3): channels last
    want = tm.torch_chain(tm.torch_tensor(bits, dtype), scale, offset).numpy()
    got = tm.quantise(tm.as_float32(bits, dtype), scale, offset)
    bad = np.nonzero(got != want)
    assert bad[0].size == 0, (dtype, scale, offset, bits[bad][:8], got[bad][:8], want[bad][:8])


def test_model_on_uint8_is_the_identity_by_default_and_equals_torch():
    bits = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    assert np.array_equal(tm.quantise(tm.as_float32(bits, "uint8"), 1.0, 0.0), bits)
    for scale, offset in tm.SCALE_OFFSETS:
        want = tm.torch_chain(tm.torch_tensor(bits, "uint8"), scale, offset).numpy()
        assert np.array_equal(tm.quantise(tm.as_float32(bits, "uint8"), scale, offset), want)


def test_float32_set_holds_what_it_promises():
    e = tm.float32_edges()
    b = e.view(np.uint32)
    assert 0x00000000 in b and 0x80000000 in b                                      # +-0
    assert np.isposinf(e).any() and np.isneginf(e).any() and np.isnan(e).any()
    sub = (b & 0x7F800000 == 0) & (b & 0x007FFFFF != 0)
    assert (sub & (e > 0)).any() and (sub & (e < 0)).any()                          # subnormals
    # with (1, 0) the inputs are the values themselves: every tie and a value on either side of it
    for k in range(-1, 257):
        t = np.float32(k + 0.5)
        assert t in e and np.nextafter(t, np.float32(-np.inf)) in e and np.nextafter(t, np.float32(np.inf)) in e, k
    # with every other pair at least the exact ties that exist are hit from both sides
    for scale, offset in tm.SCALE_OFFSETS:
        with np.errstate(all="ignore"):
            v = e * np.float32(scale[1]) + np.float32(offset[1])
        frac = v[np.isfinite(v) & (v > -1) & (v < 257)] % 1
        assert (frac == 0.5).any() and ((frac > 0.49) & (frac < 0.5)).any() and ((frac > 0.5) & (frac < 0.51)).any()


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_sets_hold_inputs_a_fused_multiply_add_would_quantise_differently(dtype):
    """the definition is two roundings; a kernel that contracted them would fail on these -- they must be in the sets
    the host test above and the GPU test of the quantiser use"""
    scale, offset = tm.SCALE_OFFSETS[3]
    for bits in (_inputs(dtype), tm.edge_bits(dtype)):
        e = tm.as_float32(bits, dtype)
        diff = tm.fma_differs(e[:, None], scale, offset)
        assert diff.any(), dtype
        # one of them again, in exact arithmetic: the product and the sum as rationals
        from fractions import Fraction

        i, c = np.argwhere(diff)[0]
        s32, o32 = np.float32(scale[c]), np.float32(offset[c])
        exact = Fraction(float(e[i])) * Fraction(float(s32)) + Fraction(float(o32))
        two = np.float32(np.float32(e[i] * s32) + o32)
        assert Fraction(float(two)) != exact                       # the two-step sum lost what the fused one keeps
        fused = np.float32(float(exact)) if abs(exact) < 2 ** 60 else None
        assert fused is not None and int(np.clip(np.rint(fused), 0, 255)) != int(tm.quantise(e[i], s32, o32))


def test_the_encoders_own_numpy_quantiser_equals_the_model(vali):
    """backend="cpu" quantises with numpy (vali_amd.codecs._quantise_tensor): the same pixels as the model"""
    from vali_amd.codecs import _quantise_tensor

    for dtype in tm.DTYPES:
        bits = tm.edge_bits(dtype) if dtype != "uint8" else np.arange(256, dtype=np.uint8)
        bits = np.repeat(bits[:, None], 3, axis=1)
        raw = bits.view(np.float32) if dtype == "float32" else bits
        for scale, offset in tm.SCALE_OFFSETS:
            assert np.array_equal(_quantise_tensor(raw, dtype, scale, offset),
                                  tm.quantise(tm.as_float32(bits, dtype), scale, offset)), (dtype, scale)


# ---- the layout helper ----------------------------------------------------------------------------------------------------
DLPACK = {"float32": (2, 32), "float16": (2, 16), "bfloat16": (4, 16), "uint8": (1, 8)}


def _torch_dtype(name):
    import torch

    return getattr(torch, name)


@pytest.mark.parametrize("dtype", tm.DTYPES)
def test_layout_helper_accepts_every_accepted_view(dtype):
    import torch
    from vali_amd.tasks import tensor_src_layout

    code, bits = DLPACK[dtype]
    t = torch.zeros((2, 3, 8, 10), dtype=_torch_dtype(dtype))
    big = torch.zeros((4, 3, 10, 14), dtype=_torch_dtype(dtype))
    for x in (t, big[:, :, 1:9, 3:13], big[::2], t[:1], t[:, :, :1], t[:, :, :, :1]):
        assert tensor_src_layout(x.shape, x.stride(), code, bits) == ("planar", dtype), x.stride()
    assert tensor_src_layout((2, 3, 8, 10), None, code, bits) == ("planar", dtype)
    t = t.contiguous(memory_format=torch.channels_last)
    big = big.contiguous(memory_format=torch.channels_last)
    for x in (t, big[:, :, 1:9, 3:13], big[::2]):
        assert tensor_src_layout(x.shape, x.stride(), code, bits) == ("packed", dtype), x.stride()


@pytest.mark.parametrize("shape, strides, code, bits, what", [
    ((2, 3, 10, 8), (240, 80, 1, 10), 2, 32, "transposed"),
    ((2, 3, 10, 8), (240, 1, 3, 30), 1, 8, "transposed"),
    ((2, 3, 8, 10), (240, 80, 10, -1), 1, 8, "negative"),
    ((2, 3, 8, 10), (240, 80, -10, 1), 2, 16, "negative"),
    ((2, 3, 8, 10), (240, 80, 10, 2), 1, 8, "strided"),
    ((2, 3, 8, 10), (240, 80, 0, 1), 4, 16, "overlap"),
    ((3, 8, 10), (80, 10, 1), 1, 8, "4-D"),
    ((2, 1, 8, 10), (80, 80, 10, 1), 1, 8, "C = 1"),
    ((2, 4, 8, 10), (320, 80, 10, 1), 2, 32, "C = 4"),
    ((2, 3, 8, 10), (240, 80, 10, 1), 2, 64, "dtype"),
    ((2, 3, 8, 10), (240, 80, 10, 1), 0, 8, "dtype"),                    # int8
    ((2, 3, 8, 10), (240, 80, 10, 1), 1, 16, "dtype"),                   # uint16
    ((2, 3, 8, 10), (240, 80, 10, 1), 6, 8, "dtype"),                    # bool
    ((0, 3, 8, 10), (240, 80, 10, 1), 1, 8, "empty"),
    ((65536, 3, 2, 2), (12, 4, 2, 1), 1, 8, "65535"),
])
def test_layout_helper_names_what_is_wrong(shape, strides, code, bits, what):
    from vali_amd.tasks import tensor_src_layout

    with pytest.raises(ValueError, match=what) as err:
        tensor_src_layout(shape, strides, code, bits)
    assert str(err.value).startswith("tensor: ")


def test_destination_helper_still_refuses_uint8():
    from vali_amd.tasks import tensor_layout

    with pytest.raises(ValueError, match="out: the dtype must be float32, float16 or bfloat16"):
        tensor_layout((2, 3, 8, 10), (240, 80, 10, 1), 1, 8)
    assert tensor_layout((2, 3, 8, 10), (240, 80, 10, 1), 2, 16) == ("planar", "float16")


class _FlippedDeviceArray:
    __cuda_array_interface__ = {"shape": (2, 3, 8, 10), "typestr": "|u1", "data": (4096, False), "version": 3,
                                "strides": (240, 80, 10, -1)}


class _OnAnotherDevice:
    """says it lives on GPU 1; the encoder below is on GPU 0"""
    import types
    device = types.SimpleNamespace(type="cuda", index=1)
    __cuda_array_interface__ = {"shape": (1, 3, 8, 8), "typestr": "<f2", "data": (4096, False), "version": 3}


class _Float64DeviceArray:
    __cuda_array_interface__ = {"shape": (2, 3, 8, 10), "typestr": "<f8", "data": (4096, False), "version": 3}


def _encoder(vali):
    """an encoder without its device-side parts: everything below is refused before one is needed"""
    enc = object.__new__(vali.PyNvJpegEncoder)
    enc._backend, enc._gpu_id, enc._stream = "hip", 0, 0
    return enc


def test_run_tensor_refuses_what_is_no_device_tensor(vali):
    import torch

    enc = _encoder(vali)
    ctx = vali.PyNvJpegEncoder.Context(enc, 90, vali.RGB, subsampling="420")
    good = torch.zeros((2, 3, 8, 10), dtype=torch.float16)
    for t, what in ((good, "GPU"),                                              # a CPU tensor
                    (good.to(torch.uint8), "GPU"),
                    (good.transpose(2, 3), "transposed"),
                    (good.flip(3).numpy(), "__dlpack__|negative|GPU|strides"),  # numpy: never a device tensor
                    (_FlippedDeviceArray(), "negative"),
                    (_Float64DeviceArray(), "dtype"),
                    (_OnAnotherDevice(), "device 1"),
                    (torch.zeros((3, 8, 10)), "4-D"),
                    (torch.zeros((2, 1, 8, 10)), "C = 1"),
                    (torch.zeros((2, 3, 8, 10), dtype=torch.float64), "dtype"),
                    (torch.zeros((2, 3, 8, 10), dtype=torch.int8), "dtype"),
                    (object(), "__dlpack__")):
        with pytest.raises(ValueError, match=what):
            enc.RunTensor(ctx, t)
    for kw, what in ((dict(scale=float("nan")), "scale"), (dict(scale=(1.0, float("inf"), 1.0)), "scale"),
                     (dict(offset=float("-inf")), "offset"), (dict(scale=1e39), "scale"),
                     (dict(scale=(1.0, 2.0)), "scale"), (dict(offset="x"), "offset")):
        with pytest.raises(ValueError, match=what):
            enc.RunTensor(ctx, good, **kw)


def test_python_vali_reexports_run_tensor(vali):
    import python_vali

    assert python_vali.PyNvJpegEncoder.RunTensor is vali.PyNvJpegEncoder.RunTensor


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_header_declares_the_tensor_encoder(tmp_path):
    tu = tmp_path / "tu.c"
    tu.write_text(
        '#include <stddef.h>\n#include "vali_hip.h"\n'
        "int main(void) {\n"
        "  int (*enc)(const vali_tensor_src*, const float*, const float*, const vali_jpeg_params*, void*, size_t,\n"
        "             uint8_t*, size_t, uint32_t*, vali_stream_t) = vali_jpeg_encode_tensor;\n"
        "  (void)enc;\n"
        "  return sizeof(vali_tensor_src) == 56 && sizeof(vali_tensor_src) == sizeof(vali_tensor_dst) &&\n"
        "         offsetof(vali_tensor_src, dtype) == 8 && offsetof(vali_tensor_src, packed) == 12 &&\n"
        "         offsetof(vali_tensor_src, n) == 16 && offsetof(vali_tensor_src, height) == 24 &&\n"
        "         offsetof(vali_tensor_src, stride_n) == 32 && offsetof(vali_tensor_src, stride_y) == 48 &&\n"
        "         VALI_DTYPE_U8 == 3 ? 0 : 1;\n"
        "}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", "-c",
                    str(tu), "-o", str(tmp_path / "tu.o")], check=True)
    subprocess.run(["gcc", "-std=c99", f"-I{ROOT / 'include'}", str(tu), "-o", str(tmp_path / "tu"),
                    "-Wl,--unresolved-symbols=ignore-all"], check=True)
    assert subprocess.run([str(tmp_path / "tu")]).returncode == 0


class _TensorSrc(ctypes.Structure):
    """include/vali_hip.h: vali_tensor_src (and vali_tensor_dst)"""
    _fields_ = [("data", ctypes.c_void_p), ("dtype", ctypes.c_int32), ("packed", ctypes.c_int32), ("n", ctypes.c_int32),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("stride_n", ctypes.c_int64), ("stride_c", ctypes.c_int64), ("stride_y", ctypes.c_int64)]


class _JpegParams(ctypes.Structure):
    """include/vali_hip.h: vali_jpeg_params"""
    _fields_ = [("quality", ctypes.c_int32), ("format", ctypes.c_int32), ("h_samp", ctypes.c_int32),
                ("v_samp", ctypes.c_int32), ("restart_interval", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3),
                ("qtable", (ctypes.c_uint8 * 64) * 2)]


def test_shim_tensor_src_size(vali):
    from vali_amd._native import shim

    assert shim.TENSOR_SRC_SIZE == 56 == ctypes.sizeof(_TensorSrc)
    assert shim.DTYPE_U8 == 3


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(str(ROOT / "vali_amd" / "libvali_hip.so"))
    lib.vali_last_error.restype = ctypes.c_char_p
    assert hasattr(lib, "vali_jpeg_encode_tensor"), "vali_jpeg_encode_tensor is not exported"
    lib.vali_jpeg_encode_tensor.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                            ctypes.c_void_p, ctypes.c_void_p]
    lib.vali_jpeg_workspace_size.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.vali_jpeg_stream_capacity.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def test_library_checks_tensor_encoder_arguments_without_a_gpu(vali, lib):
    """Every refusal is decided before any HIP call: the pointers below are dummies that are never read."""
    assert ctypes.sizeof(_JpegParams) == 160
    W, H, N = 32, 16, 2

    def params(fmt=vali.RGB, hs=2, vs=2):
        p = _JpegParams()
        assert lib.vali_jpeg_params_init_sampled(90, int(fmt), hs, vs, ctypes.byref(p)) == 0
        return p

    def sizes(p, n=N, w=W, h=H):
        ws, cap = ctypes.c_size_t(0), ctypes.c_size_t(0)
        if lib.vali_jpeg_workspace_size(n, w, h, ctypes.byref(p), ctypes.byref(ws)) != 0:
            return 1 << 30, 1 << 30                         # params that are refused anyway: sizes that cannot be why
        assert lib.vali_jpeg_stream_capacity(w, h, ctypes.byref(p), ctypes.byref(cap)) == 0
        return ws.value, cap.value

    buf = ctypes.create_string_buffer(1024)
    base = (ctypes.addressof(buf) + 255) & ~255             # stands in for every device pointer, 256-byte aligned
    three = ctypes.c_float * 3

    def src(**kw):
        t = _TensorSrc()
        t.data, t.dtype, t.packed, t.n, t.width, t.height = base, 1, 0, N, W, H
        t.stride_n, t.stride_c, t.stride_y = 3 * H * W, H * W, W
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    def call(t, p=None, scale=(255.0,) * 3, offset=(0.0,) * 3, ws=base, ws_bytes=None, out=base, stride=None,
             d_sizes=base, null=()):
        p = params() if p is None else p
        need, cap = sizes(p, t.n if 1 <= t.n <= 65535 else N, t.width if 1 <= t.width <= 65535 else W,
                          t.height if 1 <= t.height <= 65535 else H)
        s, o = three(*scale), three(*offset)                # live until the call returns
        args = dict(src=ctypes.addressof(t), scale=ctypes.addressof(s), offset=ctypes.addressof(o),
                    params=ctypes.addressof(p), ws=ws, ws_bytes=need if ws_bytes is None else ws_bytes, out=out,
                    stride=cap if stride is None else stride, d_sizes=d_sizes)
        for k in null:
            args[k] = None
        return lib.vali_jpeg_encode_tensor(args["src"], args["scale"], args["offset"], args["params"], args["ws"],
                                           args["ws_bytes"], args["out"], args["stride"], args["d_sizes"], None)

    INVALID, UNSUPPORTED = -1, -2
    # null arguments
    for name in ("src", "scale", "offset", "params", "ws", "out", "d_sizes"):
        assert call(src(), null=(name,)) == INVALID, name
        assert b"null" in lib.vali_last_error(), name
    assert call(src(data=None)) == INVALID and b"null" in lib.vali_last_error()
    # the tensor
    bad = [dict(dtype=4), dict(dtype=-1), dict(packed=2), dict(packed=-1), dict(n=0), dict(n=65536), dict(n=-1),
           dict(width=0), dict(height=0), dict(width=65536), dict(height=65536), dict(width=-3),
           dict(stride_n=0), dict(stride_n=-1536), dict(stride_c=0), dict(stride_c=-512), dict(stride_y=0),
           dict(stride_y=-32), dict(stride_y=W - 1), dict(packed=1, stride_y=3 * W - 1),
           dict(data=base + 1),                                    # an odd address with a 2-byte dtype
           dict(dtype=2, data=base + 1),
           dict(dtype=0, data=base + 2)]                           # a float32 one that is only 2-aligned
    for kw in bad:
        assert call(src(**kw)) == INVALID, kw
    assert call(src(stride_y=W - 1)) == INVALID and b"stride_y" in lib.vali_last_error()
    assert call(src(dtype=4)) == INVALID and b"dtype" in lib.vali_last_error()
    # non-finite scale / offset
    for c in range(3):
        for v in (float("nan"), float("inf"), float("-inf")):
            s = [255.0] * 3
            s[c] = v
            assert call(src(), scale=s) == INVALID and b"finite" in lib.vali_last_error()
            o = [0.0] * 3
            o[c] = v
            assert call(src(), offset=o) == INVALID and b"finite" in lib.vali_last_error()
    # formats: what cannot name three full-size channels
    for fmt in (vali.YUV420, vali.YUV422):
        p = params(fmt, 2, 2 if fmt == vali.YUV420 else 1)
        assert call(src(), p=p) == UNSUPPORTED, fmt
    p = params()
    for fmt in (vali.NV12, vali.Y, vali.RGB_32F, vali.RGB_32F_PLANAR):
        p.format = int(fmt)
        assert call(src(), p=p) == UNSUPPORTED, fmt
    # what vali_jpeg_encode_batch checks on params, workspace and out_stride
    p = params(vali.YUV444, 1, 1)
    p.h_samp = 2
    assert call(src(), p=p) == INVALID and b"sampling" in lib.vali_last_error()
    p = params()
    p.restart_interval = 0
    assert call(src(), p=p) == INVALID and b"restart" in lib.vali_last_error()
    p = params()
    p.restart_interval = 11                                # 4:2:0: at most 10 MCUs of 6 blocks
    assert call(src(), p=p) == INVALID and b"restart" in lib.vali_last_error()
    p = params()
    p.qtable[1][63] = 0
    assert call(src(), p=p) == INVALID and b"quantisation" in lib.vali_last_error()
    p = params()
    need, cap = sizes(p)
    assert call(src(), ws=base + 16) == INVALID and b"aligned" in lib.vali_last_error()
    assert call(src(), ws_bytes=need - 1) == INVALID and b"workspace" in lib.vali_last_error()
    assert call(src(), stride=cap - 1) == INVALID and b"out_stride" in lib.vali_last_error()
    assert buf.raw == bytes(1024)                          # nothing was written through the dummies


def test_preprocessor_tensor_forms_still_refuse_dtype_3(vali):
    lib = ctypes.CDLL(str(ROOT / "vali_amd" / "libvali_hip.so"))
    lib.vali_last_error.restype = ctypes.c_char_p
    buf = ctypes.create_string_buffer(64)
    base = ctypes.addressof(buf)
    params = (ctypes.c_float * 16)()
    t = _TensorSrc()
    t.data, t.dtype, t.packed, t.n, t.width, t.height = base, 3, 0, 2, 32, 16
    t.stride_n, t.stride_c, t.stride_y = 3 * 16 * 32, 16 * 32, 32
    assert lib.vali_nv12_preproc_roi_tensor(ctypes.c_void_p(base), None, ctypes.byref(t), params, 0, None, None) == -1
    assert b"dtype" in lib.vali_last_error()
    assert lib.vali_rgb_preproc_roi_tensor(ctypes.c_void_p(base), None, int(vali.RGB), ctypes.byref(t), params, 0, None,
                                           None) == -1
    assert b"dtype" in lib.vali_last_error()
    t.dtype = 1
    # the same struct with a dtype they know is not refused for its dtype
    rc = lib.vali_nv12_preproc_roi_tensor(None, None, ctypes.byref(t), params, 0, None, None)
    assert rc == -1 and b"null" in lib.vali_last_error()


def test_host_and_code_object_agree_on_the_kernel_names():
    """k_jpeg_fdct's signature depends on its template arguments; were anything in it mangled differently by the host
    and the device pass (an unnamed enum was), a launch would abort for want of the symbol.  The names the host object
    registers against the names in the compiler's device-side resource report."""
    import re

    nm = shutil.which("nm") or shutil.which("llvm-nm")
    if nm is None:
        pytest.skip("no nm to list the host object's symbols")
    obj = ROOT / "vali_amd" / "csrc" / "_obj"
    # the build's own products (vali_amd/build.py keeps both next to each other): without them this guard would be gone
    assert (obj / "jpeg.o").exists() and (obj / "jpeg.resources.txt").exists(), \
        "the build left no vali_amd/csrc/_obj/jpeg.o or jpeg.resources.txt to compare"
    host = set(re.findall(r"\b(_ZN\S*k_jpeg_fdctI\S*)", subprocess.run([nm, str(obj / "jpeg.o")], check=True,
                                                                     capture_output=True, text=True).stdout))
    host = {h for h in host if "__device_stub__" not in h}
    device = set(re.findall(r"Function Name: (\S*k_jpeg_fdctI\S*)", (obj / "jpeg.resources.txt").read_text()))
    assert len(device) == 10 + 32, len(device)
    assert host == device, sorted(host ^ device)[:4]
