"""Baseline JPEG decode on the GPU (PyNvJpegDecoder, vali_jpeg_decode_batch): every output is bit-identical to the
numpy model of tests/jpeg_decode_model.py, itself pinned to Pillow by tests/test_jpeg_decode_host.py."""
import io
from pathlib import Path

import numpy as np
import pytest

import jpeg_decode_files as jf
import jpeg_decode_model as dm
import jpeg_model as jm

PIL = pytest.importorskip("PIL.Image")
GOLDEN = Path(__file__).resolve().parent / "golden"

pytestmark = pytest.mark.gpu

# output format -> the samplings it accepts
FORMATS = {"RGB": jf.SAMPLINGS, "BGR": jf.SAMPLINGS, "RGB_PLANAR": jf.SAMPLINGS, "Y": jf.SAMPLINGS,
           "YUV444": ("444",), "YUV422": ("422",), "YUV420": ("420",), "NV12": ("420",)}
SIZES = [(1, 1), (7, 9), (17, 33), (96, 64)]
QUALITIES = [1, 50, 90, 100]


@pytest.fixture(scope="module")
def frame():
    return np.asarray(PIL.open(GOLDEN / "frame_0.jpg").convert("RGB"))


def legal(fmt, w, h):
    if fmt in ("YUV420", "NV12"):
        return w + (w & 1), h + (h & 1)
    if fmt == "YUV422":
        return w + (w & 1), h
    return w, h


def download(vali, gpu, surfaces):
    out = []
    for s in surfaces:
        host = np.zeros(s.HostSize, np.uint8)
        ok, info = vali.PySurfaceDownloader(gpu).Run(s, host)
        assert ok, info
        out.append(host)
    return out


def decode(vali, gpu, files, fmt, dec=None):
    dec = dec or vali.PyNvJpegDecoder(gpu)
    surfaces, info = dec.Run(files, vali.PixelFormat[fmt])
    assert info == vali.TaskExecInfo.SUCCESS, (info, dec.last_status)
    return download(vali, gpu, surfaces)


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_every_format_and_sampling_equals_the_model(vali, gpu, frame, fmt):
    dec = vali.PyNvJpegDecoder(gpu)
    for sampling in FORMATS[fmt]:
        for size in SIZES:
            w, h = legal(fmt, *size)
            files = [jf.make_file(sampling, w, h, q, "noise" if q == 100 else "frame", seed=q + w, frame=frame,
                                  restart=r) for q in QUALITIES for r in (False, True)]
            got = decode(vali, gpu, files, fmt, dec)
            for k, (f, g) in enumerate(zip(files, got)):
                assert np.array_equal(g, dm.surface_bytes(f, fmt)), (fmt, sampling, w, h, k)


def test_1080p_420_equals_pillow_and_the_model(vali, gpu, frame):
    rgb = jf.picture(1920, 1080, "frame", 3, frame)
    plain = jf.pillow_file(rgb, "420", 90)
    rst = jf.pillow_file(rgb, "420", 90, restart_blocks=12)
    got = decode(vali, gpu, [plain, rst], "RGB")
    for f, g in zip((plain, rst), got):
        assert np.array_equal(g.reshape(1080, 1920, 3), np.asarray(PIL.open(io.BytesIO(f)).convert("RGB")))
    nv12 = decode(vali, gpu, [plain], "NV12")[0]
    assert np.array_equal(nv12, dm.surface_bytes(plain, "NV12"))


def test_frame0_equals_pillow(vali, gpu):
    data = (GOLDEN / "frame_0.jpg").read_bytes()
    dec = vali.PyNvJpegDecoder(gpu)
    info = dec.Info(data)
    assert (info.width, info.height, info.sampling, info.restart_interval) == (848, 464, "444", 0)
    got = decode(vali, gpu, [data], "RGB", dec)[0].reshape(464, 848, 3)
    assert np.array_equal(got, np.asarray(PIL.open(GOLDEN / "frame_0.jpg").convert("RGB")))


@pytest.mark.parametrize("fmt", [jm.RGB, jm.YUV420, jm.YUV422], ids=["RGB", "YUV420", "YUV422"])
def test_round_trip_through_both_encoders(vali, gpu, frame, fmt):
    w, h = 424, 232
    host = jm.make_host(fmt, w, h, "frame", frame=frame)
    s = vali.Surface.Make(vali.PixelFormat(fmt), w, h, gpu)
    assert vali.PyFrameUploader(gpu).Run(host, s)[0]
    files = []
    for backend in ("hip", "cpu"):
        enc = vali.PyNvJpegEncoder(gpu, backend=backend)
        out, info = enc.Run(enc.Context(85, vali.PixelFormat(fmt)), [s])
        assert info == vali.TaskExecInfo.SUCCESS
        files.append(out[0].tobytes())
    for f, g in zip(files, decode(vali, gpu, files, "RGB")):
        assert np.array_equal(g.reshape(h, w, 3), np.asarray(PIL.open(io.BytesIO(f)).convert("RGB")))


def test_mixed_batch_equals_single_calls(vali, gpu, frame):
    """different sizes and samplings in one call, as if each were decoded alone"""
    specs = [("420", 424, 232, 90, False), ("444", 17, 33, 75, True), ("gray", 96, 64, 50, False),
             ("440", 64, 48, 90, True), ("422", 300, 200, 100, False), ("420", 8, 8, 1, True)]
    files = [jf.make_file(s, w, h, q, "frame", seed=i, frame=frame, restart=r) for i, (s, w, h, q, r) in enumerate(specs)]
    dec = vali.PyNvJpegDecoder(gpu)
    for fmt in ("RGB", "Y"):
        batch = decode(vali, gpu, files, fmt, dec)
        for i, f in enumerate(files):
            assert np.array_equal(batch[i], decode(vali, gpu, [f], fmt, dec)[0]), (fmt, i)
            assert np.array_equal(batch[i], dm.surface_bytes(f, fmt)), (fmt, i)


def test_slow_synchronising_streams(vali, gpu, frame):
    """q = 100 noise (long code words), 1-MCU restart intervals and images smaller than one subsequence"""
    rgb = jf.picture(512, 384, "noise", 5)
    files = [jf.pillow_file(rgb, "444", 100), jf.pillow_file(rgb, "420", 100),
             jf.model_file(jf.picture(200, 120, "frame", 1, frame), 2, 2, 100, R=1),
             jf.model_file(jf.picture(9, 7, "noise", 2), 1, 1, 100, R=1),
             jf.pillow_file(jf.picture(3, 2, "noise", 3), "420", 95)]
    for f, g in zip(files, decode(vali, gpu, files, "RGB")):
        assert np.array_equal(g, dm.surface_bytes(f, "RGB"))


def test_pitched_dlpack_and_offset_views_leave_the_arena_alone(vali, gpu, frame):
    import torch

    w, h = 200, 120
    f = jf.make_file("420", w, h, 90, "frame", frame=frame)
    want = dm.surface_bytes(f, "RGB").reshape(h, 3 * w)
    big = torch.full((2 * h + 16, 3 * w + 160), 0x5A, dtype=torch.uint8, device=f"cuda:{gpu}")
    torch.cuda.synchronize()
    pitched = vali.Surface.from_dlpack(torch.utils.dlpack.to_dlpack(big[:h, :3 * w]))
    view = vali.Surface.from_dlpack(torch.utils.dlpack.to_dlpack(big[h + 5:2 * h + 5, 7:7 + 3 * w]))
    ok, info = vali.PyNvJpegDecoder(gpu).RunInto([f, f], [pitched, view])
    assert ok, info
    torch.cuda.synchronize()
    got = big.cpu().numpy()
    assert np.array_equal(got[:h, :3 * w], want)
    assert np.array_equal(got[h + 5:2 * h + 5, 7:7 + 3 * w], want)
    mask = np.ones_like(got, bool)
    mask[:h, :3 * w] = False
    mask[h + 5:2 * h + 5, 7:7 + 3 * w] = False
    assert np.all(got[mask] == 0x5A)


def corrupt_cases(frame):
    """(name, file) pairs: a truncated scan, a wrong RSTn, a run past 63 (all corrupt for the model) and seeded
    flipped bits in the entropy data (the model says which of them are corrupt)"""
    base = jf.make_file("420", 160, 96, 90, "frame", frame=frame)
    rst = jf.make_file("420", 160, 96, 90, "frame", seed=1, frame=frame, restart=True)
    start = len(base) - len(jm.entropy_of_file(base)) - 2
    cases = [("truncated", base[:start + (len(base) - start) // 2])]
    i = rst.index(b"\xff\xd1")
    cases.append(("wrong RSTn", rst[:i] + b"\xff\xd5" + rst[i + 2:]))
    # one gray 8 x 8 block whose AC symbols are ZRL x 3 (k = 49) and then a run of 15: coefficient 64
    hdr = jm.header(8, 8, jm.YUV444, 90, 0)
    dc, ac = jm.huff_codes(jm.DC_LUMA), jm.huff_codes(jm.AC_LUMA)
    bits = jm._Bits()
    bits.put(*dc[0])
    for _ in range(3):
        bits.put(*ac[0xF0])
    bits.put(*ac[0xF1])
    bits.put(1, 1)
    bits.flush()
    sof1 = hdr.index(b"\xff\xc0")
    gray = hdr[:sof1] + b"\xff\xc0\x00\x0b\x08\x00\x08\x00\x08\x01\x01\x11\x00" + hdr[sof1 + 19:]
    sos = gray.index(b"\xff\xda")
    gray = gray[:sos] + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00"
    cases.append(("run past 63", gray + bytes(bits.out) + b"\xff\xd9"))
    for seed in range(6):
        rng = np.random.default_rng(seed)
        b = bytearray(base)
        k = int(rng.integers(start, len(base) - 2))
        b[k] ^= 1 << int(rng.integers(0, 8))
        cases.append((f"flip {seed}", bytes(b)))
    return cases


def test_corrupt_files_fail_and_leave_the_destination_alone(vali, gpu, frame):
    import torch

    dec = vali.PyNvJpegDecoder(gpu)
    cases = corrupt_cases(frame)
    verdicts = {name: dm.surface_bytes(f, "RGB") for name, f in cases}
    assert all(verdicts[n] is None for n in ("truncated", "wrong RSTn", "run past 63"))
    for name, f in cases:
        try:
            info = dec.Info(f)
        except ValueError:
            continue                            # a flip that breaks the marker structure is refused on the host
        want = verdicts[name]
        w, h = info.width, info.height
        big = torch.full((h + 8, 3 * w + 64), 0xC3, dtype=torch.uint8, device=f"cuda:{gpu}")
        torch.cuda.synchronize()
        view = vali.Surface.from_dlpack(torch.utils.dlpack.to_dlpack(big[4:4 + h, 16:16 + 3 * w]))
        ok, res = dec.RunInto([f], [view])
        torch.cuda.synchronize()
        got = big.cpu().numpy()
        mask = np.ones_like(got, bool)
        mask[4:4 + h, 16:16 + 3 * w] = False
        assert np.all(got[mask] == 0xC3), name
        if want is None:
            assert not ok and res == vali.TaskExecInfo.FAIL, name
            assert np.all(got == 0xC3), name
        else:
            assert ok, (name, dec.last_status)
            assert np.array_equal(got[4:4 + h, 16:16 + 3 * w].reshape(-1), want), name


def test_unsupported_and_mismatched_requests(vali, gpu, frame):
    dec = vali.PyNvJpegDecoder(gpu)
    prog = (GOLDEN / "frame_0_90_deg.jpg").read_bytes()
    with pytest.raises(ValueError):
        dec.Info(prog)
    assert dec.Run([prog]) == ([], vali.TaskExecInfo.FAIL)
    f444 = jf.make_file("444", 64, 48, 90, frame=frame)
    assert dec.Run([f444], vali.NV12)[1] != vali.TaskExecInfo.SUCCESS           # no resampling
    s = vali.Surface.Make(vali.RGB, 32, 48, gpu)
    assert dec.RunInto([f444], [s]) == (False, vali.TaskExecInfo.INVALID_INPUT)


def test_graph_capture_replays_on_new_entropy_bytes(vali, gpu, frame):
    """the decode path neither allocates nor synchronises: captured once, replayed with new data of one layout"""
    from vali_amd._native import shim

    w, h = 160, 96
    # flat pictures of two grey levels whose DC differences code to the same number of bits: one layout
    flat = [jm.encode(jm.RGB, np.full(w * h * 3, level, np.uint8), w, h, 80, 0) for level in range(100, 128)]
    a = flat[0]
    b = next(c for c in flat[1:] if len(c) == len(a))
    info = shim.jpeg_parse(a)
    assert shim.jpeg_parse(b).data_len == info.data_len
    dev = info.copy()
    dev.data_offset = 0
    off, ln = int(info.data_offset), int(info.data_len)
    stream = shim.stream_create(gpu)
    surf = vali.Surface.Make(vali.RGB, w, h, gpu)
    wsb = shim.jpeg_decode_workspace_size([dev])
    ws, d_infos, d_data, d_status = (shim.mem_alloc(gpu, x) for x in (wsb, shim.JPEG_INFO_SIZE, ln + 16, 4))
    d_dst = shim.descs_upload(gpu, [surf.desc()], stream)
    blob = np.frombuffer(dev.tobytes(), np.uint8).copy()
    try:
        shim.memcpy2d_async(gpu, d_infos, blob.size, blob.ctypes.data, blob.size, blob.size, 1, 0, stream)
        shim.stream_sync(gpu, stream)

        def put(f):
            body = np.frombuffer(f, np.uint8)[off:off + ln].copy()
            shim.memcpy2d_async(gpu, d_data, ln, body.ctypes.data, ln, ln, 1, 0, stream)
            shim.stream_sync(gpu, stream)

        def get():
            shim.stream_sync(gpu, stream)
            host = np.zeros(surf.HostSize, np.uint8)
            assert vali.PySurfaceDownloader(gpu).Run(surf, host)[0]
            st = np.zeros(1, np.int32)
            shim.memcpy2d_async(gpu, st.ctypes.data, 4, d_status, 4, 4, 1, 1, stream)
            shim.stream_sync(gpu, stream)
            return host, int(st[0])

        put(a)
        capture = vali.StreamCapture(stream, gpu)
        with capture:
            assert shim.jpeg_decode_batch([dev], d_infos, d_data, int(vali.RGB), d_dst, ws, wsb, d_status, stream) == 0
        capture.Launch()
        got, st = get()
        assert st == 0 and np.array_equal(got, dm.surface_bytes(a, "RGB"))
        put(b)
        capture.Launch()
        got, st = get()
        assert st == 0 and np.array_equal(got, dm.surface_bytes(b, "RGB"))
        del capture
    finally:
        for ptr in (ws, d_infos, d_data, d_status, d_dst):
            shim.mem_free(gpu, ptr)
        shim.stream_destroy(gpu, stream)
