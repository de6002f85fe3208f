"""Baseline JPEG on the GPU (PyNvJpegEncoder(backend="hip"), vali_jpeg_encode_batch): every file is byte-identical to
the numpy model of tests/jpeg_model.py (itself pinned to Pillow's libjpeg by tests/test_jpeg_host.py), and decodes to
what the CPU backend's file decodes to."""
import io
from pathlib import Path

import numpy as np
import pytest

import jpeg_model as jm

PIL = pytest.importorskip("PIL.Image")
GOLDEN = Path(__file__).resolve().parent / "golden"

pytestmark = pytest.mark.gpu

NAMES = {jm.RGB: "RGB", jm.BGR: "BGR", jm.RGB_PLANAR: "RGB_PLANAR", jm.YUV444: "YUV444", jm.YUV422: "YUV422",
         jm.YUV420: "YUV420"}
# odd sizes, single-MCU images, MCU counts that R does not divide (21 / 16 / 10 MCUs per segment), 1080p
SIZES = [(1, 1), (7, 9), (17, 33), (62, 30), (424, 232), (1920, 1080)]
QUALITIES = [1, 50, 75, 90, 100]


def legal(fmt, w, h):
    if fmt == jm.YUV420:
        return w + (w & 1), h + (h & 1)
    if fmt == jm.YUV422:
        return w + (w & 1), h
    return w, h


@pytest.fixture(scope="module")
def frame():
    return np.asarray(PIL.open(GOLDEN / "frame_0.jpg").convert("RGB"))


def upload(vali, gpu, fmt, host, w, h):
    s = vali.Surface.Make(vali.PixelFormat(fmt), w, h, gpu)
    assert s.HostSize == host.size
    ok, info = vali.PyFrameUploader(gpu).Run(host, s)
    assert ok, info
    return s


def encode(vali, gpu, fmt, q, surfaces, backend="hip"):
    enc = vali.PyNvJpegEncoder(gpu, backend=backend)
    out, info = enc.Run(enc.Context(q, vali.PixelFormat(fmt)), surfaces)
    assert info == vali.TaskExecInfo.SUCCESS
    return [bytes(b.tobytes()) for b in out]


@pytest.mark.parametrize("fmt", list(NAMES), ids=NAMES.get)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_file_equals_model(vali, gpu, frame, fmt, size):
    w, h = legal(fmt, *size)
    content = "frame" if w > 64 else "noise"
    host = jm.make_host(fmt, w, h, content, seed=w + h, frame=frame)
    s = upload(vali, gpu, fmt, host, w, h)
    qs = QUALITIES if (w, h) != (1920, 1080) else [90]
    for q in qs:
        got = encode(vali, gpu, fmt, q, [s])[0]
        want = jm.encode(fmt, host, w, h, q)
        assert got == want, (NAMES[fmt], w, h, q, len(got), len(want))


@pytest.mark.parametrize("fmt", list(NAMES), ids=NAMES.get)
def test_decodes_like_the_cpu_backend(vali, gpu, frame, fmt):
    w, h = 424, 232
    host = jm.make_host(fmt, w, h, "frame", frame=frame)
    s = upload(vali, gpu, fmt, host, w, h)
    for q in (50, 90):
        ours = encode(vali, gpu, fmt, q, [s])[0]
        theirs = encode(vali, gpu, fmt, q, [s], backend="cpu")[0]
        a, b = PIL.open(io.BytesIO(ours)), PIL.open(io.BytesIO(theirs))
        assert a.mode == b.mode and np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("fmt", [jm.RGB, jm.YUV420], ids=NAMES.get)
def test_batch_equals_single_frames(vali, gpu, frame, fmt):
    """a call with frames of two sizes: one launch per size, every result as if encoded alone"""
    sizes = [(424, 232), (424, 232), (96, 64), (424, 232), (96, 64)]
    hosts = [jm.make_host(fmt, w, h, ["noise", "frame", "flat"][i % 3], seed=i, frame=frame)
             for i, (w, h) in enumerate(sizes)]
    surfs = [upload(vali, gpu, fmt, hst, w, h) for hst, (w, h) in zip(hosts, sizes)]
    batch = encode(vali, gpu, fmt, 75, surfs)
    for i, s in enumerate(surfs):
        assert batch[i] == encode(vali, gpu, fmt, 75, [s])[0], i
        assert batch[i] == jm.encode(fmt, hosts[i], *sizes[i], 75), i


def test_pitched_dlpack_surface_and_a_view(vali, gpu, frame):
    import torch

    w, h = 200, 120
    host = jm.make_host(jm.RGB, w, h, "frame", frame=frame).reshape(h, 3 * w)
    want = jm.encode(jm.RGB, host, w, h, 90)
    big = torch.zeros((2 * h + 8, 3 * w + 160), dtype=torch.uint8, device=f"cuda:{gpu}")
    big[:h, :3 * w] = torch.from_numpy(host).to(big.device)
    big[h + 5:2 * h + 5, 7:7 + 3 * w] = torch.from_numpy(host).to(big.device)    # a view that starts off alignment
    torch.cuda.synchronize()
    pitched = vali.Surface.from_dlpack(torch.utils.dlpack.to_dlpack(big[:h, :3 * w]))
    view = vali.Surface.from_dlpack(torch.utils.dlpack.to_dlpack(big[h + 5:2 * h + 5, 7:7 + 3 * w]))
    assert pitched.Pitch == 3 * w + 160 and (pitched.Width, pitched.Height) == (w, h)
    assert encode(vali, gpu, jm.RGB, 90, [pitched])[0] == want
    assert encode(vali, gpu, jm.RGB, 90, [view])[0] == want


def test_worst_case_noise_stays_in_its_slot(vali, gpu):
    """noise at q = 100 is the most bits and the most stuffed bytes; nothing is written past the image's bytes"""
    from vali_amd._native import shim

    w, h, n = 256, 128, 2
    hosts = [jm.make_host(jm.RGB, w, h, "noise", seed=50 + i) for i in range(n)]
    surfs = [upload(vali, gpu, jm.RGB, hst, w, h) for hst in hosts]
    p = shim.jpeg_params_init(100, jm.RGB)
    cap = shim.jpeg_stream_capacity(w, h, p)
    wsb = shim.jpeg_workspace_size(n, w, h, p)
    stream = vali.HipResMgr.Instance().GetStream(gpu)
    tail = 4096
    ws, out, sizes = shim.mem_alloc(gpu, wsb), shim.mem_alloc(gpu, n * cap + tail), shim.mem_alloc(gpu, 4 * n)
    d_src = shim.descs_upload(gpu, [s.desc() for s in surfs], stream)
    try:
        shim.memset2d_async(gpu, out, n * cap + tail, 0xA5, n * cap + tail, 1, stream)
        assert shim.jpeg_encode_batch(d_src, n, w, h, jm.RGB, p, ws, wsb, out, cap, sizes, stream) == 0
        got = np.zeros(n * cap + tail, np.uint8)
        lens = np.zeros(n, np.uint32)
        shim.memcpy2d_async(gpu, got.ctypes.data, got.size, out, got.size, got.size, 1, 1, stream)
        shim.memcpy2d_async(gpu, lens.ctypes.data, 4 * n, sizes, 4 * n, 4 * n, 1, 1, stream)
        shim.stream_sync(gpu, stream)
    finally:
        for ptr in (d_src, ws, out, sizes):
            shim.mem_free(gpu, ptr)
    for i in range(n):
        body = jm.entropy(jm.RGB, hosts[i], w, h, 100)
        assert int(lens[i]) == len(body) and body.count(b"\xff\x00") > 100
        assert bytes(got[i * cap: i * cap + len(body)]) == body
        assert np.all(got[i * cap + len(body): (i + 1) * cap] == 0xA5), i     # sentinel after the image's bytes
    assert np.all(got[n * cap:] == 0xA5)


@pytest.mark.parametrize("fmt", ["RGB", "YUV420", "RGB_PLANAR", "YUV444"])
def test_reference_psnr_check(vali, gpu, fmt):
    """reference tests/test_PyNvJpegEncoder.py:150-222 (test_codecs.test_jpeg_encoder_cpu_fallback) on the GPU
    backend: NV12 -> dst format -> JPEG q100; the decoded RGB image is within 42 dB of the raw surface"""
    w, h = 424, 232
    raw = np.fromfile(GOLDEN / "test_small_2frames.nv12", np.uint8).reshape(2, -1)
    src = vali.Surface.Make(vali.NV12, w, h, gpu)
    assert vali.PyFrameUploader(gpu).Run(raw[0], src)[0]
    dst_fmt = vali.PixelFormat[fmt]
    cvt = vali.PySurfaceConverter(gpu)
    if fmt in ("RGB", "YUV420"):
        dst = vali.Surface.Make(dst_fmt, w, h, gpu)
        assert cvt.Run(src, dst)[0]
    else:
        mid = vali.Surface.Make(vali.RGB, w, h, gpu)
        dst = vali.Surface.Make(dst_fmt, w, h, gpu)
        assert cvt.Run(src, mid)[0] and cvt.Run(mid, dst)[0]
    enc = vali.PyNvJpegEncoder(gpu_id=gpu, backend="hip")
    ctx = enc.Context(compression=100, pixel_format=dst_fmt)
    buffers, info = enc.Run(ctx, [dst, dst])
    assert info == vali.TaskExecInfo.SUCCESS and len(buffers) == 2 and buffers[0].dtype == np.uint8
    assert buffers[0].size > 1000 and np.array_equal(buffers[0], buffers[1])
    img = PIL.open(io.BytesIO(buffers[0].tobytes()))
    assert img.size == (w, h)
    if fmt == "RGB":
        host = np.zeros(dst.HostSize, np.uint8)
        assert vali.PySurfaceDownloader(gpu).Run(dst, host)[0]
        d = np.asarray(img).astype(np.float64).reshape(-1) - host
        assert 10 * np.log10(255.0 ** 2 / np.mean(d * d)) >= 42.0


def test_all_or_nothing(vali, gpu):
    w, h = 64, 32
    enc = vali.PyNvJpegEncoder(gpu, backend="hip")
    ctx = enc.Context(90, vali.RGB)
    good = upload(vali, gpu, jm.RGB, jm.make_host(jm.RGB, w, h), w, h)
    other = vali.Surface.Make(vali.BGR, w, h, gpu)
    assert enc.Run(ctx, [good, other]) == ([], vali.TaskExecInfo.FAIL)
    assert enc.Run(ctx, [good, None]) == ([], vali.TaskExecInfo.FAIL)
    assert enc.Run(ctx, [good, vali.Surface(vali.RGB)]) == ([], vali.TaskExecInfo.FAIL)
    odd = vali.Surface.Make(vali.YUV420, 33, 32, gpu)                  # 4:2:0 needs an even width
    ctx420 = enc.Context(90, vali.YUV420)
    assert enc.Run(ctx420, [odd]) == ([], vali.TaskExecInfo.FAIL)
    out, info = enc.Run(ctx, [good])
    assert info == vali.TaskExecInfo.SUCCESS and len(out) == 1
    with pytest.raises(ValueError):
        vali.PyNvJpegEncoder(gpu, backend="nvjpeg")


def test_graph_capture_replays_the_same_bytes(vali, gpu, frame):
    """the encode path neither allocates nor synchronises: captured once, replayed on new pixels"""
    from vali_amd._native import shim

    w, h, n = 160, 96, 3
    fmt = jm.YUV420
    hosts = [jm.make_host(fmt, w, h, "frame", seed=i, frame=np.roll(frame, 37 * i, 1)) for i in range(n)]
    surfs = [upload(vali, gpu, fmt, hst, w, h) for hst in hosts]
    p = shim.jpeg_params_init(80, fmt)
    cap = shim.jpeg_stream_capacity(w, h, p)
    wsb = shim.jpeg_workspace_size(n, w, h, p)
    stream = shim.stream_create(gpu)
    ws, out, sizes = shim.mem_alloc(gpu, wsb), shim.mem_alloc(gpu, n * cap), shim.mem_alloc(gpu, 4 * n)
    d_src = shim.descs_upload(gpu, [s.desc() for s in surfs], stream)
    try:
        capture = vali.StreamCapture(stream, gpu)
        with capture:
            assert shim.jpeg_encode_batch(d_src, n, w, h, fmt, p, ws, wsb, out, cap, sizes, stream) == 0

        def read():
            lens = np.zeros(n, np.uint32)
            shim.memcpy2d_async(gpu, lens.ctypes.data, 4 * n, sizes, 4 * n, 4 * n, 1, 1, stream)
            shim.stream_sync(gpu, stream)
            res = []
            for i in range(n):
                b = np.zeros(int(lens[i]), np.uint8)
                shim.memcpy2d_async(gpu, b.ctypes.data, b.size, out + i * cap, b.size, b.size, 1, 1, stream)
                res.append(b)
            shim.stream_sync(gpu, stream)
            return [bytes(b.tobytes()) for b in res]

        capture.Launch()
        first = read()
        for i in range(n):
            assert first[i] == jm.entropy(fmt, hosts[i], w, h, 80), i
        # new pixels in the same surfaces, replay
        hosts2 = hosts[1:] + hosts[:1]
        for s, hst in zip(surfs, hosts2):
            assert vali.PyFrameUploader(gpu).Run(hst, s)[0]
        capture.Launch()
        second = read()
        assert second == first[1:] + first[:1]
        del capture
    finally:
        for ptr in (d_src, ws, out, sizes):
            shim.mem_free(gpu, ptr)
        shim.stream_destroy(gpu, stream)
