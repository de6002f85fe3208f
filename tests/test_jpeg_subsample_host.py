"""RGB, BGR and RGB_PLANAR surfaces coded 4:2:2 and 4:2:0, without a GPU: the numpy model of the chroma downsampling
(tests/jpeg_subsample_model.py) against Pillow's libjpeg-turbo byte for byte, then the host-side C ABI
(vali_jpeg_params_init_sampled, header, sizes) and the Python surface (Context(..., subsampling=...))."""
import ctypes
import io
from pathlib import Path

import numpy as np
import pytest

import jpeg_model as jm
import jpeg_subsample_model as sm

PIL = pytest.importorskip("PIL.Image")

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
# 17x16, 20x20, 33x31, 50x7, 130x70: a chroma sample past the component's width is an average of replicated pixels with
# its own bias (a model that replicates the downsampled plane fails there); 16x17, 33x31, 15x9: an odd last row
SIZES = [(16, 16), (17, 16), (16, 17), (1, 1), (15, 9), (20, 20), (33, 31), (19, 22), (48, 34), (50, 7), (7, 50),
         (130, 70), (424, 232)]
QUALITIES = [1, 50, 90, 100]
RGB_FORMATS = {jm.RGB: "RGB", jm.BGR: "BGR", jm.RGB_PLANAR: "RGB_PLANAR"}
YUV_OWN = {jm.YUV444: (1, 1), jm.YUV422: (2, 1), jm.YUV420: (2, 2)}


@pytest.fixture(scope="module")
def frame():
    return np.asarray(PIL.open(GOLDEN / "frame_0.jpg").convert("RGB"))


# ---- the model is libjpeg-turbo's default downsampler ------------------------------------------------------------------
@pytest.mark.parametrize("samp", ["420", "422"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_model_entropy_data_equals_pillow(samp, size, frame):
    w, h = size
    contents = ["frame"] if (w, h) == (424, 232) else ["noise", "flat", "checker"]
    for content in contents:
        for q in QUALITIES:
            host = sm.make_host(jm.RGB, w, h, content, seed=w * h + q, frame=frame)
            ours = sm.entropy(jm.RGB, host, w, h, q, samp, R=0)
            theirs = sm.pillow_encode(jm.RGB, host, w, h, q, samp)
            assert ours == jm.entropy_of_file(theirs), (samp, w, h, q, content)


def test_the_checkerboard_leaves_every_chroma_sample_to_the_bias():
    """the two colours' Cb and Cr sums are odd: a 2x1 sum has remainder 1, a 2x2 sum remainder 2, so the alternating
    bias (0, 1 / 1, 2) alone decides whether each sample rounds down or up"""
    host = sm.make_host(jm.RGB, 16, 16, "checker")
    _, cb, cr = jm.rgb_to_ycc(host.reshape(16, 16, 3))
    for p in (cb, cr):
        assert (int(p[0, 0]) + int(p[0, 1])) & 1
        for V, lo in ((1, (int(p[0, 0]) + int(p[0, 1])) >> 1), (2, (2 * (int(p[0, 0]) + int(p[0, 1]))) >> 2)):
            d = sm.downsample(p, 2, V)
            assert (d[:, 0::2] == lo).all() and (d[:, 1::2] == lo + 1).all()


def test_model_edges_are_not_symmetric():
    """20 x 20: chroma column 10 of the 16 wide block averages pixel column 19 with itself under the bias of an even
    column, column 11 under that of an odd one; replicating chroma column 9 would give neither"""
    rng = np.random.default_rng(3)
    p = rng.integers(0, 256, (20, 20), dtype=np.uint8)
    d = sm.downsample(p, 2, 2)
    assert d.shape == (16, 16)
    e = p[:, 19].astype(int)
    want = (2 * (e[0::2] + e[1::2]))
    assert np.array_equal(d[:10, 10], (want + 1) >> 2) and np.array_equal(d[:10, 11], (want + 2) >> 2)
    assert np.array_equal(d[10:], np.broadcast_to(d[9], (6, 16)))        # below ch the downsampled rows repeat
    d = sm.downsample(p[:19], 2, 2)                                      # odd height: row 18 pairs with itself
    assert np.array_equal(d[9, :10], (2 * (p[18, 0::2].astype(int) + p[18, 1::2]) + 1 + (np.arange(10) & 1)) >> 2)


@pytest.mark.parametrize("fmt", list(RGB_FORMATS), ids=RGB_FORMATS.get)
def test_model_reads_every_rgb_layout_as_rgb(fmt, frame):
    w, h = 50, 22
    want = sm.entropy(jm.RGB, jm.make_host(jm.RGB, w, h, "frame", frame=frame), w, h, 90, "420")
    assert sm.entropy(fmt, jm.make_host(fmt, w, h, "frame", frame=frame), w, h, 90, "420") == want


def test_model_at_444_is_the_existing_model(frame):
    host = jm.make_host(jm.RGB, 50, 22, "frame", frame=frame)
    assert sm.encode(jm.RGB, host, 50, 22, 75, "444") == jm.encode(jm.RGB, host, 50, 22, 75)


@pytest.mark.parametrize("samp", ["420", "422"])
def test_model_file_with_restarts_decodes_like_pillow(samp, frame):
    w, h = 130, 70
    host = jm.make_host(jm.RGB, w, h, "frame", frame=frame)
    ours = PIL.open(io.BytesIO(sm.encode(jm.RGB, host, w, h, 90, samp)))
    theirs = PIL.open(io.BytesIO(sm.pillow_encode(jm.RGB, host, w, h, 90, samp)))
    assert np.array_equal(np.asarray(ours), np.asarray(theirs))


# ---- the C ABI, host-only entry points ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    from vali_amd._native import shim

    return shim


@pytest.mark.parametrize("fmt", list(RGB_FORMATS), ids=RGB_FORMATS.get)
@pytest.mark.parametrize("samp, R", [("444", 21), ("422", 16), ("420", 10)])
def test_params_sampling_interval_and_tables(shim, fmt, samp, R):
    H, V = sm.SAMPLINGS[samp]
    for q in (1, 50, 90, 100, 0, 101):
        p, base = shim.jpeg_params_init_sampled(q, fmt, H, V), shim.jpeg_params_init(q, fmt)
        assert (p.h_samp, p.v_samp, p.restart_interval, p.format) == (H, V, R, fmt)
        assert R == sm.restart_interval(samp) and R * (H * V + 2) <= 64 < (R + 1) * (H * V + 2)
        assert p.qtable == base.qtable and p.quality == base.quality == max(1, min(100, q))
    assert (base.h_samp, base.v_samp, base.restart_interval) == (1, 1, 21)       # the old entry point is as it was


@pytest.mark.parametrize("fmt", list(YUV_OWN))
def test_params_of_a_yuv_format_take_its_own_sampling_only(shim, fmt):
    H, V = YUV_OWN[fmt]
    p, base = shim.jpeg_params_init_sampled(75, fmt, H, V), shim.jpeg_params_init(75, fmt)
    assert (p.h_samp, p.v_samp, p.restart_interval, p.qtable) == (H, V, base.restart_interval, base.qtable)
    for other in set(YUV_OWN.values()) - {(H, V)}:
        with pytest.raises(Exception):
            shim.jpeg_params_init_sampled(75, fmt, *other)


class Params(ctypes.Structure):
    _fields_ = [("quality", ctypes.c_int32), ("format", ctypes.c_int32), ("h_samp", ctypes.c_int32),
                ("v_samp", ctypes.c_int32), ("restart_interval", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3),
                ("qtable", (ctypes.c_uint8 * 64) * 2)]


def test_accepted_and_refused_combinations_without_a_device():
    lib = ctypes.CDLL(str(ROOT / "vali_amd" / "libvali_hip.so"))
    init = lib.vali_jpeg_params_init_sampled
    assert ctypes.sizeof(Params) == 160
    p = Params()
    n = ctypes.c_size_t(0)
    samplings = [(h, v) for h in range(0, 5) for v in range(0, 5)]
    for fmt in jm.FORMATS:
        ok = {(1, 1), (2, 1), (2, 2)} if fmt in RGB_FORMATS else {YUV_OWN[fmt]}
        for h, v in samplings:
            rc = init(90, fmt, h, v, ctypes.byref(p))
            assert rc == (0 if (h, v) in ok else -1), (fmt, h, v, rc)
            if rc == 0:
                assert (p.format, p.h_samp, p.v_samp) == (fmt, h, v)
                assert lib.vali_jpeg_stream_capacity(16, 16, ctypes.byref(p), ctypes.byref(n)) == 0
    assert init(90, jm.RGB, 2, 2, None) == -1
    for fmt in (3, 0, 1, 99):                                            # NV12, Y, ...: cannot be encoded at all
        assert init(90, fmt, 1, 1, ctypes.byref(p)) == -2, fmt
        assert init(90, fmt, 2, 2, ctypes.byref(p)) == -2, fmt
    # jpeg_geom applies the same rule to a params block made by hand
    assert init(90, jm.RGB, 2, 2, ctypes.byref(p)) == 0
    for h, v, want in [(1, 2, -1), (4, 1, -1), (2, 4, -1), (0, 0, -1), (2, 1, 0), (1, 1, 0), (2, 2, 0)]:
        p.h_samp, p.v_samp, p.restart_interval = h, v, 1
        assert lib.vali_jpeg_stream_capacity(16, 16, ctypes.byref(p), ctypes.byref(n)) == want, (h, v)
    assert lib.vali_jpeg_params_init(90, jm.YUV420, ctypes.byref(p)) == 0
    p.h_samp = 1
    assert lib.vali_jpeg_stream_capacity(16, 16, ctypes.byref(p), ctypes.byref(n)) == -1
    # the even-size rule belongs to the source format: RGB at 4:2:0 takes odd sizes, the restart interval is bounded
    assert init(90, jm.RGB, 2, 2, ctypes.byref(p)) == 0
    buf = (ctypes.c_uint8 * 1024)()
    for w, h in [(15, 9), (1, 1), (65535, 15)]:
        assert lib.vali_jpeg_header(w, h, ctypes.byref(p), buf, 1024, ctypes.byref(n)) == 0 and n.value > 600
    p.restart_interval = 11                                             # 66 blocks: more than a wave codes
    assert lib.vali_jpeg_header(16, 16, ctypes.byref(p), buf, 1024, ctypes.byref(n)) == -1


@pytest.mark.parametrize("samp", ["420", "422"])
@pytest.mark.parametrize("w, h", [(1, 1), (16, 16), (15, 9), (424, 232), (1919, 1081), (65535, 7)])
def test_header_equals_model_and_parses(shim, samp, w, h):
    H, V = sm.SAMPLINGS[samp]
    p = shim.jpeg_params_init_sampled(75, jm.RGB, H, V)
    hdr = shim.jpeg_header(w, h, p)
    assert hdr == sm.header(w, h, 75, samp)
    if w * h > 100000:
        img = PIL.open(io.BytesIO(hdr + b"\xff\xd9"))
    else:
        img = PIL.open(io.BytesIO(hdr + sm.entropy(jm.RGB, sm.make_host(jm.RGB, w, h, "noise"), w, h, 75, samp) + b"\xff\xd9"))
        img.load()
    assert img.size == (w, h) and img.format == "JPEG"
    assert img.layer[0][1:3] == (H, V) and img.layer[1][1:3] == (1, 1) and img.layer[2][1:3] == (1, 1)
    assert img.quantization[0] == list(p.qtable[0])


def test_sizes_are_worst_case(shim):
    p = shim.jpeg_params_init_sampled(90, jm.RGB, 2, 2)
    # 1920x1080 at 4:2:0: 120 x 68 MCUs of 6 blocks, 10 MCUs per segment, 2 x 208 bytes per block
    nmcu, slot = 120 * 68, 2 * 60 * 208
    nseg = -(-nmcu // 10)
    assert shim.jpeg_stream_capacity(1920, 1080, p) == nseg * (slot + 2)

    def a256(v):
        return (v + 255) & ~255
    for n in (1, 2, 16):
        want = a256(n * nmcu * 6 * 128) + 2 * a256(n * nseg * 4) + n * nseg * slot
        assert shim.jpeg_workspace_size(n, 1920, 1080, p) == want
    # half the blocks of 4:4:4
    p444 = shim.jpeg_params_init(90, jm.RGB)
    assert shim.jpeg_workspace_size(1, 1920, 1080, p) < 0.55 * shim.jpeg_workspace_size(1, 1920, 1080, p444)
    p422 = shim.jpeg_params_init_sampled(90, jm.RGB, 2, 1)
    assert shim.jpeg_stream_capacity(1920, 1080, p422) == -(-120 * 135 // 16) * (2 * 64 * 208 + 2)


# ---- the Python surface -----------------------------------------------------------------------------------------------
def test_context_takes_and_reports_the_subsampling():
    import vali_amd as vali

    for ctx_of in (vali.NvJpegEncodeContext,):       # PyNvJpegEncoder.Context: tests/test_gpu_jpeg_subsample.py
        for fmt in (vali.RGB, vali.BGR, vali.RGB_PLANAR):
            assert ctx_of(90, fmt).Subsampling() == "444"
            assert ctx_of(90, fmt, None).Subsampling() == "444"
            for samp in ("444", "422", "420"):
                ctx = ctx_of(90, fmt, subsampling=samp)
                assert (ctx.Subsampling(), ctx.Format(), ctx.Compression()) == (samp, fmt, 90)
        for fmt, own in ((vali.YUV444, "444"), (vali.YUV422, "422"), (vali.YUV420, "420")):
            assert ctx_of(90, fmt).Subsampling() == own and ctx_of(90, fmt, own).Subsampling() == own
            for samp in {"444", "422", "420"} - {own}:
                with pytest.raises(ValueError):
                    ctx_of(90, fmt, samp)
        for bad in ("440", "411", "4:2:0", "", 420, 2, (2, 2)):
            with pytest.raises(ValueError):
                ctx_of(90, vali.RGB, bad)
        with pytest.raises(ValueError):
            ctx_of(90, vali.NV12, "420")                                # NV12 sources stay refused
    import python_vali

    assert python_vali.NvJpegEncodeContext(90, python_vali.PixelFormat.RGB, "420").Subsampling() == "420"
