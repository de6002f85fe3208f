"""Baseline JPEG encoder, host side (no GPU): the numpy model (tests/jpeg_model.py) is pinned byte for byte to Pillow's
libjpeg, and the host-only C entry points (vali_jpeg_params_init / vali_jpeg_header / sizes) are checked against it."""
import ctypes
import io
from pathlib import Path

import numpy as np
import pytest

import jpeg_model as jm

PIL = pytest.importorskip("PIL.Image")

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
SIZES = [(1, 1), (7, 9), (16, 16), (17, 33), (424, 232), (1920, 1080)]
QUALITIES = [1, 50, 75, 90, 100]
CONTENTS = ["noise", "flat", "frame"]
FMT_NAMES = {jm.RGB: "RGB", jm.BGR: "BGR", jm.RGB_PLANAR: "RGB_PLANAR", jm.YUV444: "YUV444", jm.YUV422: "YUV422",
             jm.YUV420: "YUV420"}


@pytest.fixture(scope="module")
def frame():
    return np.asarray(PIL.open(GOLDEN / "frame_0.jpg").convert("RGB"))


def legal(fmt, w, h):
    """the size rule of the library: 4:2:0 even width and height, 4:2:2 even width"""
    if fmt == jm.YUV420:
        return w + (w & 1), h + (h & 1)
    if fmt == jm.YUV422:
        return w + (w & 1), h
    return w, h


def _cases():
    out = []
    for fmt in (jm.RGB, jm.YUV420, jm.YUV422, jm.YUV444):
        for (w, h) in SIZES:
            for content in CONTENTS:
                # 1080p noise through plain-Python Huffman coding takes seconds: one quality per format and content
                qs = QUALITIES if (w, h) != (1920, 1080) else [90 if content != "noise" else 50]
                for q in qs:
                    out.append(pytest.param(fmt, *legal(fmt, w, h), q, content,
                                            id=f"{FMT_NAMES[fmt]}-{w}x{h}-q{q}-{content}"))
    return out


@pytest.mark.parametrize("fmt, w, h, q, content", _cases())
def test_model_entropy_data_equals_pillow(fmt, w, h, q, content, frame):
    host = jm.make_host(fmt, w, h, content, seed=w * 7 + h + q, frame=frame)
    want = jm.entropy_of_file(jm.pillow_encode(fmt, host, w, h, q))
    assert jm.entropy(fmt, host, w, h, q, R=0) == want


@pytest.mark.parametrize("fmt", [jm.BGR, jm.RGB_PLANAR])
def test_model_reads_every_rgb_layout_as_rgb(fmt, frame):
    w, h = 40, 24
    rgb = jm.make_host(jm.RGB, w, h, "frame", frame=frame)
    other = jm.make_host(fmt, w, h, "frame", frame=frame)
    assert jm.entropy(fmt, other, w, h, 75) == jm.entropy(jm.RGB, rgb, w, h, 75)


def test_model_file_with_restarts_decodes_like_pillow(frame):
    """restart markers change the bytes, not the picture"""
    w, h = 424, 232
    for fmt in (jm.RGB, jm.YUV422, jm.YUV420):
        host = jm.make_host(fmt, w, h, "frame", frame=frame)
        ours = np.asarray(PIL.open(io.BytesIO(jm.encode(fmt, host, w, h, 90))))
        theirs = np.asarray(PIL.open(io.BytesIO(jm.pillow_encode(fmt, host, w, h, 90))))
        assert np.array_equal(ours, theirs)


def test_restart_interval_keeps_a_segment_within_a_wave():
    assert [jm.restart_interval(f) for f in (jm.RGB, jm.YUV422, jm.YUV420)] == [21, 16, 10]


def test_quantisation_trick_is_exact_everywhere():
    """the kernel's (|x| + corr) * recip >> shift (jcdctmgr's reciprocal, 32-bit unsigned) equals |x| / 8q rounded
    half away from zero for every divisor the tables can hold and every |x| < 2^15"""
    x = np.arange(1 << 15, dtype=np.uint64)
    for q in range(1, 256):
        recip, corr, shift = jm.quant_recip(8 * q)
        prod = (x + np.uint64(corr)) * np.uint64(recip)
        assert int(prod.max()) < 1 << 32, q                    # fits the kernel's u32 multiply
        got = prod >> np.uint64(shift)
        assert np.array_equal(got, (x + np.uint64(4 * q)) // np.uint64(8 * q)), q


# ---- the C ABI, host-only entry points ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    from vali_amd._native import shim

    return shim


@pytest.mark.parametrize("q", QUALITIES + [0, -5, 101, 1000])
def test_params_tables_equal_pillow_quantization(shim, q):
    p = shim.jpeg_params_init(q, jm.RGB)
    qc = max(1, min(100, q))
    img = PIL.fromarray(np.zeros((8, 8, 3), np.uint8))
    b = io.BytesIO()
    img.save(b, format="JPEG", quality=qc, subsampling=0)
    pil_q = PIL.open(io.BytesIO(b.getvalue())).quantization
    assert p.quality == qc
    assert p.qtable[0] == list(pil_q[0]) and p.qtable[1] == list(pil_q[1])
    assert [list(t) for t in jm.quant_tables(q)] == p.qtable


@pytest.mark.parametrize("fmt", jm.FORMATS)
def test_params_sampling_and_restart_interval(shim, fmt):
    p = shim.jpeg_params_init(90, fmt)
    assert (p.h_samp, p.v_samp) == jm.sampling(fmt) and p.restart_interval == jm.restart_interval(fmt)
    assert p.format == fmt


@pytest.mark.parametrize("fmt", jm.FORMATS)
@pytest.mark.parametrize("w, h", [(1, 1), (16, 16), (424, 232), (1919, 1081), (65535, 8)])
def test_header_equals_model_and_parses(shim, fmt, w, h):
    w, h = legal(fmt, w, h)
    if w > 65535:
        w -= 2
    p = shim.jpeg_params_init(75, fmt)
    hdr = shim.jpeg_header(w, h, p)
    assert hdr == jm.header(w, h, fmt, 75)
    # a parser reads the header: size, sampling and tables
    body = jm.entropy(fmt, jm.make_host(fmt, 16, 16, "flat"), 16, 16, 75) if (w, h) == (16, 16) else None
    if body is not None:
        img = PIL.open(io.BytesIO(hdr + body + b"\xff\xd9"))
        img.load()
        assert img.size == (16, 16)
        assert img.quantization[0] == list(p.qtable[0])
    else:
        img = PIL.open(io.BytesIO(hdr + b"\xff\xd9"))
        assert img.size == (w, h) and img.format == "JPEG"


def test_sizes_are_worst_case(shim):
    p = shim.jpeg_params_init(90, jm.RGB)
    # 1920x1080: 240 x 135 MCUs of 3 blocks, 21 MCUs per segment, 2 x 208 bytes per block
    nseg = -(-240 * 135 // 21)
    assert shim.jpeg_stream_capacity(1920, 1080, p) == nseg * (2 * 63 * 208 + 2)
    assert shim.jpeg_workspace_size(2, 1920, 1080, p) > 2 * 240 * 135 * 3 * 128 + 2 * nseg * 2 * 63 * 208
    assert shim.jpeg_workspace_size(2, 1920, 1080, p) < shim.jpeg_workspace_size(3, 1920, 1080, p)


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(str(ROOT / "vali_amd" / "libvali_hip.so"))
    lib.vali_last_error.restype = ctypes.c_char_p
    return lib


class Params(ctypes.Structure):
    _fields_ = [("quality", ctypes.c_int32), ("format", ctypes.c_int32), ("h_samp", ctypes.c_int32),
                ("v_samp", ctypes.c_int32), ("restart_interval", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3),
                ("qtable", (ctypes.c_uint8 * 64) * 2)]


def test_bad_arguments_are_refused_without_a_device(lib):
    assert ctypes.sizeof(Params) == 160
    p = Params()
    assert lib.vali_jpeg_params_init(90, 2, None) == -1
    assert lib.vali_jpeg_params_init(90, 3, ctypes.byref(p)) == -2              # NV12 cannot be encoded
    assert lib.vali_jpeg_params_init(90, 4, ctypes.byref(p)) == 0
    n = ctypes.c_size_t(0)
    buf = (ctypes.c_uint8 * 1024)()
    assert lib.vali_jpeg_header(16, 16, ctypes.byref(p), buf, 1024, ctypes.byref(n)) == 0 and n.value > 600
    assert lib.vali_jpeg_header(16, 16, ctypes.byref(p), buf, 10, ctypes.byref(n)) == -1
    assert lib.vali_jpeg_header(15, 16, ctypes.byref(p), buf, 1024, ctypes.byref(n)) == -1    # 4:2:0: odd width
    assert b"even" in lib.vali_last_error()
    assert lib.vali_jpeg_header(0, 16, ctypes.byref(p), buf, 1024, ctypes.byref(n)) == -1
    assert lib.vali_jpeg_header(65536, 16, ctypes.byref(p), buf, 1024, ctypes.byref(n)) == -1
    assert lib.vali_jpeg_header(16, 16, None, buf, 1024, ctypes.byref(n)) == -1
    assert lib.vali_jpeg_stream_capacity(16, 16, ctypes.byref(p), None) == -1
    assert lib.vali_jpeg_workspace_size(-1, 16, 16, ctypes.byref(p), ctypes.byref(n)) == -1
    bad = Params.from_buffer_copy(p)
    bad.restart_interval = 11                                                   # 11 MCUs of 6 blocks > 64
    assert lib.vali_jpeg_stream_capacity(16, 16, ctypes.byref(bad), ctypes.byref(n)) == -1
    bad = Params.from_buffer_copy(p)
    bad.qtable[1][5] = 0
    assert lib.vali_jpeg_stream_capacity(16, 16, ctypes.byref(bad), ctypes.byref(n)) == -1
    bad = Params.from_buffer_copy(p)
    bad.h_samp = 1
    assert lib.vali_jpeg_stream_capacity(16, 16, ctypes.byref(bad), ctypes.byref(n)) == -1
    # the encoder checks everything before touching a device: null pointers, a foreign format, short buffers
    fake = ctypes.c_void_p(256)
    enc = lib.vali_jpeg_encode_batch
    enc.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                    ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                    ctypes.c_void_p]
    assert lib.vali_jpeg_workspace_size(1, 16, 16, ctypes.byref(p), ctypes.byref(n)) == 0
    ws = n.value
    assert lib.vali_jpeg_stream_capacity(16, 16, ctypes.byref(p), ctypes.byref(n)) == 0
    cap = n.value
    args = [fake, 1, 16, 16, 4, ctypes.addressof(p), fake, ws, fake, cap, fake, None]
    for i, bad_value in [(0, None), (5, None), (6, None), (8, None), (10, None), (4, 2), (7, ws - 1), (9, cap - 1),
                         (1, -1), (1, 65536), (2, 15), (6, ctypes.c_void_p(257))]:
        a = list(args)
        a[i] = bad_value
        assert enc(*a) == -1, (i, bad_value)
