"""Per-image optimised Huffman tables, without a GPU: the numpy model (tests/jpeg_optimize_model.py) against Pillow's
libjpeg-turbo (save(optimize=True, restart_marker_blocks=R)) table for table and byte for byte, then the host-side C
ABI (vali_jpeg_params.optimize: header, sizes, refusals) and the Python surface (Context(..., optimize=...))."""
import ctypes
import io
from pathlib import Path

import numpy as np
import pytest

import jpeg_model as jm
import jpeg_optimize_model as om
import jpeg_subsample_model as sm

PIL = pytest.importorskip("PIL.Image")

ROOT = Path(__file__).resolve().parent.parent
SIZES = [(8, 8), (16, 16), (17, 9), (33, 17), (97, 51), (200, 40)]
QUALITIES = [1, 50, 90, 100]
# (format, sampling): RGB at the three samplings, the YUV planes with their own
SOURCES = [(jm.RGB, "444"), (jm.RGB, "422"), (jm.RGB, "420"), (jm.YUV444, None), (jm.YUV422, None), (jm.YUV420, None)]
IDS = ["RGB-444", "RGB-422", "RGB-420", "YUV444", "YUV422", "YUV420"]


def fits(fmt, w, h):
    """planar YUV 4:2:0 needs an even width and height, 4:2:2 an even width"""
    return not ((fmt == jm.YUV420 and (w | h) & 1) or (fmt == jm.YUV422 and w & 1))


def assert_equals_pillow(fmt, host, w, h, q, samp, R, what):
    tables, data, _ = om.analyse(fmt, host, w, h, q, samp, R)
    theirs = om.pillow_encode(fmt, host, w, h, q, samp, R)
    in_file = om.tables_of_file(theirs)
    assert sorted(in_file) == sorted(om.DHT_ORDER), what
    for cls_id, (bits, vals) in zip(om.DHT_ORDER, tables):
        assert in_file[cls_id] == (list(bits), list(vals)), (what, hex(cls_id))
    assert data == jm.entropy_of_file(theirs), what
    return tables


# ---- the model is libjpeg's optimize_coding ------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt, samp", SOURCES, ids=IDS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_model_tables_and_entropy_data_equal_pillow(fmt, samp, size):
    w, h = size
    if not fits(fmt, w, h):
        w, h = w + (w & 1), h + (h & 1)                     # 17x9 -> 18x10, 33x17 -> 34x18, 97x51 -> 98x52
    default = sm.restart_interval(om.samp_of(fmt, samp))
    for content in ("noise", "smooth", "flat"):
        for q in QUALITIES:
            host = om.make_host(fmt, w, h, content, seed=w * h + q)
            for R in (1, default):
                tables = assert_equals_pillow(fmt, host, w, h, q, samp, R, (IDS[SOURCES.index((fmt, samp))], w, h,
                                                                            content, q, R))
            if content == "flat":                           # one used symbol: that symbol at length 1
                for bits, vals in tables[1::2]:
                    assert (list(bits), list(vals)) == ([1] + [0] * 15, [0x00])


def test_lengths_above_16_are_limited_as_pillow_does():
    """the 512 x 512 grey picture whose AC luma code lengths pass 16 before limiting; its chroma tables hold one symbol"""
    w = h = 512
    host = om.long_code_host(w, h)
    coefs, comp, bpm = om.scan_blocks(jm.RGB, host, w, h, 100, "444")
    counts = om.symbol_counts(coefs, comp, bpm, 21)
    longest = [max(om.code_sizes(c)) for c in counts]
    print("\nunlimited code lengths (DC luma, AC luma, DC chroma, AC chroma):", longest,
          "symbols:", [int((c > 0).sum()) for c in counts])
    assert longest[1] > 16 and max(longest) <= 32
    assert [int((c > 0).sum()) for c in counts[2:]] == [1, 1]
    tables = assert_equals_pillow(jm.RGB, host, w, h, 100, "444", 21, "long codes")
    assert max(i + 1 for i, n in enumerate(tables[1][0]) if n) == 16


def test_counts_cover_dummy_blocks_and_restart_with_the_segment():
    """17 x 9 at 4:2:0 is two MCUs of six blocks; the second one's right luma column is dummy blocks, which are coded
    and so counted: a DC symbol and an EOB each.  The DC counts change with the restart interval, because prediction
    restarts; the AC counts do not"""
    host = om.make_host(jm.RGB, 17, 9, "noise", seed=1)
    coefs, comp, bpm = om.scan_blocks(jm.RGB, host, 17, 9, 50, "420")
    assert len(coefs) == 2 * 6 and bpm == 6
    counts = om.symbol_counts(coefs, comp, bpm, 10)
    assert counts[0].sum() == 8 and counts[2].sum() == 4
    assert counts[1][0x00] >= 2                              # the two dummy blocks have no AC coefficient
    host = om.make_host(jm.RGB, 64, 8, "noise", seed=2)
    coefs, comp, bpm = om.scan_blocks(jm.RGB, host, 64, 8, 50, "444")
    a, b = om.symbol_counts(coefs, comp, bpm, 1), om.symbol_counts(coefs, comp, bpm, 21)
    assert a[0].sum() == b[0].sum() == 8 and not np.array_equal(a[0], b[0])
    assert np.array_equal(a[1], b[1])


def test_model_file_decodes_to_the_pixels_of_the_plain_file():
    w, h = 97, 51
    host = om.make_host(jm.RGB, w, h, "smooth", seed=5)
    for samp in ("444", "420"):
        ours = om.encode(jm.RGB, host, w, h, 75, samp)
        plain = sm.encode(jm.RGB, host, w, h, 75, samp)
        assert len(ours) < len(plain)
        assert ours.startswith(om.fixed_header(w, h, jm.RGB, 75, samp))
        assert np.array_equal(np.asarray(PIL.open(io.BytesIO(ours))), np.asarray(PIL.open(io.BytesIO(plain))))


# ---- the C ABI, host-only entry points ----------------------------------------------------------------------------------
class Params(ctypes.Structure):
    _fields_ = [("quality", ctypes.c_int32), ("format", ctypes.c_int32), ("h_samp", ctypes.c_int32),
                ("v_samp", ctypes.c_int32), ("restart_interval", ctypes.c_int32), ("optimize", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 2), ("qtable", (ctypes.c_uint8 * 64) * 2)]


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(str(ROOT / "vali_amd" / "libvali_hip.so"))
    lib.vali_jpeg_header.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                     ctypes.c_void_p]
    lib.vali_jpeg_workspace_size.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.vali_jpeg_stream_capacity.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.vali_jpeg_encode_batch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                           ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    lib.vali_jpeg_encode_tensor.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                            ctypes.c_void_p, ctypes.c_void_p]
    return lib


def header_of(lib, w, h, p):
    buf, n = (ctypes.c_uint8 * 1024)(), ctypes.c_size_t(0)
    assert lib.vali_jpeg_header(w, h, ctypes.byref(p), buf, 1024, ctypes.byref(n)) == 0
    return bytes(buf[:n.value])


def sizes_of(lib, n, w, h, p):
    ws, cap = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.vali_jpeg_workspace_size(n, w, h, ctypes.byref(p), ctypes.byref(ws)) == 0
    assert lib.vali_jpeg_stream_capacity(w, h, ctypes.byref(p), ctypes.byref(cap)) == 0
    return ws.value, cap.value


def test_params_keep_their_size_and_init_leaves_optimize_off(lib):
    assert ctypes.sizeof(Params) == 160 and Params.optimize.offset == 20 and Params.qtable.offset == 32
    p = Params()
    for fmt in jm.FORMATS:
        p.optimize = 7
        assert lib.vali_jpeg_params_init(90, fmt, ctypes.byref(p)) == 0
        assert p.optimize == 0 and list(p.reserved) == [0, 0]
    p.optimize = 7
    assert lib.vali_jpeg_params_init_sampled(90, jm.RGB, 2, 2, ctypes.byref(p)) == 0
    assert p.optimize == 0 and list(p.reserved) == [0, 0]


@pytest.mark.parametrize("samp", ["444", "422", "420"])
def test_header_stops_after_sof0_and_sizes_grow(lib, samp):
    H, V = sm.SAMPLINGS[samp]
    p = Params()
    assert lib.vali_jpeg_params_init_sampled(75, jm.RGB, H, V, ctypes.byref(p)) == 0
    for w, h in [(1, 1), (17, 9), (1920, 1080)]:
        plain = header_of(lib, w, h, p)
        ws0, cap0 = sizes_of(lib, 3, w, h, p)
        assert plain == sm.header(w, h, 75, samp)
        p.optimize = 1
        fixed = header_of(lib, w, h, p)
        ws1, cap1 = sizes_of(lib, 3, w, h, p)
        p.optimize = 0
        assert header_of(lib, w, h, p) == plain and sizes_of(lib, 3, w, h, p) == (ws0, cap0)
        # a strict prefix, up to and including SOF0: the next marker of the plain header is DHT
        assert fixed == om.fixed_header(w, h, jm.RGB, 75, samp)
        assert plain.startswith(fixed) and plain[len(fixed):len(fixed) + 2] == b"\xff\xc4"
        assert fixed[-19:-17] == b"\xff\xc0"
        # DHT + DRI + SOS at their worst, three images' histograms, code tables and DHT parts
        assert cap1 == cap0 + om.PREFIX_MAX
        assert ws1 >= ws0 + 3 * (2 * 4 * 256 * 4 + 4 * (17 + 256) + 4 * 4)


def test_any_other_value_of_optimize_is_refused_before_a_device_is_touched(lib):
    p = Params()
    assert lib.vali_jpeg_params_init(90, jm.RGB, ctypes.byref(p)) == 0
    n = ctypes.c_size_t(0)
    buf = (ctypes.c_uint8 * 1024)()
    fake = ctypes.c_void_p(256)                 # never read: the parameters are judged first
    scale = (ctypes.c_float * 3)(255, 255, 255)
    offset = (ctypes.c_float * 3)(0, 0, 0)

    class TensorSrc(ctypes.Structure):
        _fields_ = [("data", ctypes.c_void_p), ("dtype", ctypes.c_int32), ("packed", ctypes.c_int32),
                    ("n", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                    ("reserved", ctypes.c_int32), ("stride_n", ctypes.c_int64), ("stride_c", ctypes.c_int64),
                    ("stride_y", ctypes.c_int64)]
    src = TensorSrc(256, 0, 0, 1, 16, 16, 0, 768, 256, 16)
    for bad in (2, -1, 256, 1 << 30):
        p.optimize = bad
        assert lib.vali_jpeg_header(16, 16, ctypes.byref(p), buf, 1024, ctypes.byref(n)) == -1, bad
        assert lib.vali_jpeg_stream_capacity(16, 16, ctypes.byref(p), ctypes.byref(n)) == -1, bad
        assert lib.vali_jpeg_workspace_size(1, 16, 16, ctypes.byref(p), ctypes.byref(n)) == -1, bad
        assert lib.vali_jpeg_encode_batch(fake, 1, 16, 16, jm.RGB, ctypes.byref(p), fake, 1 << 30, fake, 1 << 30, fake,
                                          None) == -1, bad
        assert lib.vali_jpeg_encode_tensor(ctypes.byref(src), scale, offset, ctypes.byref(p), fake, 1 << 30, fake,
                                           1 << 30, fake, None) == -1, bad
    lib.vali_last_error.restype = ctypes.c_char_p
    assert b"optimize" in lib.vali_last_error()


def test_shim_params_expose_optimize():
    from vali_amd._native import shim

    p = shim.jpeg_params_init_sampled(90, jm.RGB, 2, 2)
    assert p.optimize == 0
    plain, cap0 = shim.jpeg_header(64, 48, p), shim.jpeg_stream_capacity(64, 48, p)
    p.optimize = 1
    assert p.optimize == 1
    assert shim.jpeg_header(64, 48, p) == om.fixed_header(64, 48, jm.RGB, 90, "420") and plain.startswith(shim.jpeg_header(64, 48, p))
    assert shim.jpeg_stream_capacity(64, 48, p) == cap0 + om.PREFIX_MAX
    p.optimize = 2
    with pytest.raises(Exception):
        shim.jpeg_header(64, 48, p)


# ---- the Python surface -----------------------------------------------------------------------------------------------
def test_context_takes_and_reports_optimize():
    import vali_amd as vali

    assert vali.NvJpegEncodeContext(90, vali.RGB).Optimize() is False
    assert vali.NvJpegEncodeContext(90, vali.RGB, "420").Optimize() is False            # positional callers as before
    assert vali.NvJpegEncodeContext(90, vali.RGB, optimize=True).Optimize() is True
    ctx = vali.NvJpegEncodeContext(75, vali.BGR, "420", True)
    assert (ctx.Compression(), ctx.Format(), ctx.Subsampling(), ctx.Optimize()) == (75, vali.BGR, "420", True)
    assert vali.NvJpegEncodeContext(90, vali.YUV420, optimize=True).Subsampling() == "420"
    for bad in (1, 0, "yes", None, 1.0, [True]):
        with pytest.raises(ValueError):
            vali.NvJpegEncodeContext(90, vali.RGB, optimize=bad)
    with pytest.raises(ValueError):
        vali.NvJpegEncodeContext(90, vali.NV12, optimize=True)                         # NV12 sources stay refused
    import python_vali

    assert python_vali.NvJpegEncodeContext(90, python_vali.PixelFormat.RGB, "420", True).Optimize() is True
