"""PyNvJpegEncoder(backend="hip") with Context(..., optimize=True): every file, its DHT included, equals the numpy model
(tests/jpeg_optimize_model.py, pinned to Pillow's optimize=True by tests/test_jpeg_optimize_host.py) byte for byte, and
decodes to the pixels of the plain file."""
import io
from pathlib import Path

import numpy as np
import pytest

import jpeg_model as jm
import jpeg_optimize_model as om
import jpeg_subsample_model as sm

PIL = pytest.importorskip("PIL.Image")
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"

gpu_test = pytest.mark.gpu

NAMES = {jm.RGB: "RGB", jm.BGR: "BGR", jm.RGB_PLANAR: "RGB_PLANAR", jm.YUV444: "YUV444", jm.YUV422: "YUV422",
         jm.YUV420: "YUV420"}
RGB_FORMATS = (jm.RGB, jm.BGR, jm.RGB_PLANAR)
# 8x8: one block per component; 16x16: one MCU at 4:2:0; 17x9, 33x17: partial MCUs, whose dummy blocks are counted;
# 200x40, 640x48: many segments, 640x48 more than one histogram workgroup per image at every sampling
SIZES = [(8, 8), (16, 16), (17, 9), (33, 17), (200, 40), (640, 48)]
# (format, sampling): the three RGB layouts at the three samplings, the YUV planes with their own
SOURCES = [(f, s) for f in RGB_FORMATS for s in ("444", "422", "420")] + [(jm.YUV444, None), (jm.YUV422, None),
                                                                          (jm.YUV420, None)]


def source_id(src):
    return NAMES[src[0]] + ("-" + src[1] if src[1] else "")


@pytest.fixture(scope="module")
def frame():
    return np.asarray(PIL.open(GOLDEN / "frame_0.jpg").convert("RGB"))


@pytest.fixture(scope="module")
def enc(vali, gpu):
    return vali.PyNvJpegEncoder(gpu, backend="hip")


def upload(vali, gpu, fmt, host, w, h):
    s = vali.Surface.Make(vali.PixelFormat(fmt), w, h, gpu)
    assert s.HostSize == host.size
    ok, info = vali.PyFrameUploader(gpu).Run(host, s)
    assert ok, info
    return s


def run(vali, enc, fmt, q, surfaces, samp, optimize=True):
    ctx = enc.Context(q, vali.PixelFormat(fmt), subsampling=samp, optimize=optimize)
    assert ctx.Optimize() is optimize
    out, info = enc.Run(ctx, surfaces)
    assert info == vali.TaskExecInfo.SUCCESS
    return [bytes(b.tobytes()) for b in out]


def even(fmt, w, h):
    """planar YUV 4:2:0 takes an even width and height only, 4:2:2 an even width: 17x9 -> 18x10, 33x17 -> 34x18"""
    if fmt == jm.YUV420:
        return w + (w & 1), h + (h & 1)
    return (w + (w & 1), h) if fmt == jm.YUV422 else (w, h)


def pixels(data):
    return np.asarray(PIL.open(io.BytesIO(data)))


# ---- whole files against the model ---------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("src", SOURCES, ids=source_id)
def test_file_equals_model(vali, gpu, enc, frame, src):
    """all sizes in one call (one launch per size)"""
    fmt, samp = src
    sizes = [even(fmt, w, h) for w, h in SIZES]
    contents = ["noise", "smooth", "noise", "frame", "smooth", "frame"]
    hosts = [om.make_host(fmt, w, h, c, seed=w + h, frame=frame) for (w, h), c in zip(sizes, contents)]
    surfs = [upload(vali, gpu, fmt, hst, w, h) for hst, (w, h) in zip(hosts, sizes)]
    for q in (50, 90) if fmt in (jm.RGB, jm.YUV420) else (90,):
        got = run(vali, enc, fmt, q, surfs, samp)
        for g, hst, (w, h) in zip(got, hosts, sizes):
            want = om.encode(fmt, hst, w, h, q, samp)
            assert g == want, (source_id(src), w, h, q, len(g), len(want), om.tables_of_file(g) == om.tables_of_file(want))


@gpu_test
@pytest.mark.parametrize("samp", ["444", "420"])
def test_flat_picture_has_single_symbol_tables(vali, gpu, enc, samp):
    w, h = 33, 17
    host = jm.make_host(jm.RGB, w, h, "flat", seed=4)
    got = run(vali, enc, jm.RGB, 90, [upload(vali, gpu, jm.RGB, host, w, h)], samp)[0]
    assert got == om.encode(jm.RGB, host, w, h, 90, samp)
    tables = om.tables_of_file(got)
    assert tables[0x10] == tables[0x11] == ([1] + [0] * 15, [0x00])


@gpu_test
def test_code_lengths_above_16_are_limited(vali, gpu, enc):
    """the 512 x 512 grey picture whose AC luma lengths pass 16 before limiting (tests/test_jpeg_optimize_host.py shows
    that on the model and pins the model's tables to Pillow's)"""
    w = h = 512
    host = om.long_code_host(w, h)
    coefs, comp, bpm = om.scan_blocks(jm.RGB, host, w, h, 100, "444")
    counts = om.symbol_counts(coefs, comp, bpm, 21)
    assert max(om.code_sizes(counts[1])) > 16
    tables = om.tables_of(counts)
    want = (om.fixed_header(w, h, jm.RGB, 100) + om.prefix(tables, 21) + om.huffman(coefs, comp, bpm, 21, tables)
            + b"\xff\xd9")
    got = run(vali, enc, jm.RGB, 100, [upload(vali, gpu, jm.RGB, host, w, h)], "444")[0]
    assert om.tables_of_file(got) == om.tables_of_file(want)
    assert got == want


@gpu_test
@pytest.mark.parametrize("samp", ["444", "420"])
def test_pitched_dlpack_surface_and_a_view(vali, gpu, enc, frame, samp):
    """a pitched surface and a view whose rows start 7 bytes off a dword"""
    import torch

    w, h = 200, 121
    host = jm.make_host(jm.RGB, w, h, "frame", frame=frame).reshape(h, 3 * w)
    want = om.encode(jm.RGB, host, w, h, 90, samp)
    big = torch.zeros((2 * h + 8, 3 * w + 161), dtype=torch.uint8, device=f"cuda:{gpu}")
    big[:h, :3 * w] = torch.from_numpy(host).to(big.device)
    big[h + 5:2 * h + 5, 7:7 + 3 * w] = torch.from_numpy(host).to(big.device)
    torch.cuda.synchronize()
    pitched = vali.Surface.from_dlpack(torch.utils.dlpack.to_dlpack(big[:h, :3 * w]))
    view = vali.Surface.from_dlpack(torch.utils.dlpack.to_dlpack(big[h + 5:2 * h + 5, 7:7 + 3 * w]))
    assert pitched.Pitch == 3 * w + 161 and (pitched.Width, pitched.Height) == (w, h)
    assert run(vali, enc, jm.RGB, 90, [pitched], samp)[0] == want
    assert run(vali, enc, jm.RGB, 90, [view], samp)[0] == want


# ---- batches -------------------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("samp", ["444", "420"])
def test_every_image_of_a_batch_gets_its_own_tables(vali, gpu, enc, samp):
    w, h = 97, 51
    hosts = [om.make_host(jm.BGR, w, h, c, seed=i) for i, c in enumerate(("noise", "smooth", "flat"))]
    surfs = [upload(vali, gpu, jm.BGR, hst, w, h) for hst in hosts]
    got = run(vali, enc, jm.BGR, 75, surfs, samp)
    dhts = []
    for g, hst in zip(got, hosts):
        assert g == om.encode(jm.BGR, hst, w, h, 75, samp)
        at = g.index(b"\xff\xc4")
        dhts.append(g[at:at + 2 + int.from_bytes(g[at + 2:at + 4], "big")])
    assert len(set(dhts)) == 3
    # and in another order: nothing is left over from the call before
    again = run(vali, enc, jm.BGR, 75, surfs[::-1], samp)
    assert again == got[::-1]


@gpu_test
def test_batch_of_mixed_sizes_equals_single_frames(vali, gpu, enc, frame):
    sizes = [(130, 70), (130, 70), (33, 31), (130, 70), (33, 31)]
    hosts = [om.make_host(jm.RGB, w, h, ["noise", "frame", "flat"][i % 3], seed=i, frame=frame)
             for i, (w, h) in enumerate(sizes)]
    surfs = [upload(vali, gpu, jm.RGB, hst, w, h) for hst, (w, h) in zip(hosts, sizes)]
    batch = run(vali, enc, jm.RGB, 75, surfs, "420")
    for i, s in enumerate(surfs):
        assert batch[i] == run(vali, enc, jm.RGB, 75, [s], "420")[0], i
        assert batch[i] == om.encode(jm.RGB, hosts[i], *sizes[i], 75, "420"), i


# ---- tensors -----------------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("layout", ["contiguous", "channels_last"])
@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16", "uint8"])
def test_run_tensor_equals_run_on_surfaces_of_the_same_pixels(vali, gpu, enc, dtype, layout):
    import torch

    n, w, h = 2, 50, 23
    rng = np.random.default_rng(5)
    p = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    p[1] = p[1] // 16 * 16                                                          # other statistics, other tables
    x = torch.from_numpy(p).permute(0, 3, 1, 2).to(f"cuda:{gpu}").to(getattr(torch, dtype))  # 0..255: exact in all four
    x = x.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else x.contiguous()
    torch.cuda.synchronize()
    ctx = enc.Context(90, vali.RGB, subsampling="420", optimize=True)
    out, info = enc.RunTensor(ctx, x, 1.0, 0.0)
    assert info == vali.TaskExecInfo.SUCCESS
    surfs = [upload(vali, gpu, jm.RGB, np.ascontiguousarray(p[i]).reshape(-1), w, h) for i in range(n)]
    want = run(vali, enc, jm.RGB, 90, surfs, "420")
    assert [bytes(b.tobytes()) for b in out] == want
    assert want[0] == om.encode(jm.RGB, p[0].reshape(-1), w, h, 90, "420")
    assert om.tables_of_file(want[0]) != om.tables_of_file(want[1])


# ---- decoding -----------------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("src", [(jm.RGB, "444"), (jm.RGB, "420"), (jm.RGB_PLANAR, "422"), (jm.YUV420, None)],
                         ids=source_id)
def test_decodes_to_the_pixels_of_the_plain_file(vali, gpu, enc, frame, src):
    import jpeg_decode_model as dm

    fmt, samp = src
    dec = vali.PyNvJpegDecoder(gpu)
    cpu = vali.PyNvJpegEncoder(gpu, backend="cpu")
    for (w, h), content in (((200, 40), "frame"), ((34, 18), "noise"), ((16, 16), "flat")):
        host = om.make_host(fmt, w, h, content, seed=3, frame=frame)
        s = upload(vali, gpu, fmt, host, w, h)
        ours, plain = run(vali, enc, fmt, 90, [s], samp)[0], run(vali, enc, fmt, 90, [s], samp, optimize=False)[0]
        assert len(ours) != len(plain)
        assert np.array_equal(pixels(ours), pixels(plain))
        surfs, status = dec.Run([ours, plain], vali.RGB)
        assert status == vali.TaskExecInfo.SUCCESS
        got = []
        for d in surfs:
            a = np.zeros(d.HostSize, np.uint8)
            assert vali.PySurfaceDownloader(gpu).Run(d, a)[0]
            got.append(a)
        assert np.array_equal(got[0], got[1])
        assert np.array_equal(got[0], dm.surface_bytes(ours, "RGB"))
        # the cpu backend's optimised file: Pillow's, and the same pixels
        out, info = cpu.Run(cpu.Context(90, vali.PixelFormat(fmt), subsampling=samp, optimize=True), [s])
        assert info == vali.TaskExecInfo.SUCCESS
        theirs = bytes(out[0].tobytes())
        assert theirs == om.pillow_encode(fmt, host, w, h, 90, samp, R=0)
        assert np.array_equal(pixels(theirs), pixels(plain))


# ---- contract ----------------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("src", [(jm.RGB, "420"), (jm.BGR, None), (jm.YUV422, None)], ids=source_id)
def test_optimize_false_is_the_file_of_a_context_without_the_argument(vali, gpu, enc, frame, src):
    fmt, samp = src
    w, h = 130, 70
    host = jm.make_host(fmt, w, h, "frame", frame=frame)
    s = upload(vali, gpu, fmt, host, w, h)
    out, info = enc.Run(enc.Context(90, vali.PixelFormat(fmt), samp), [s])
    assert info == vali.TaskExecInfo.SUCCESS
    plain = bytes(out[0].tobytes())
    want = sm.encode(fmt, host, w, h, 90, samp) if samp else jm.encode(fmt, host, w, h, 90)
    assert plain == want
    # before and after an optimised call: the cached parameters and headers are keyed on the flag
    assert run(vali, enc, fmt, 90, [s], samp, optimize=False)[0] == plain
    assert run(vali, enc, fmt, 90, [s], samp)[0] != plain
    assert run(vali, enc, fmt, 90, [s], samp, optimize=False)[0] == plain


@gpu_test
def test_statuses_are_all_or_nothing(vali, gpu, enc):
    ctx = enc.Context(90, vali.RGB, optimize=True)
    good = vali.Surface.Make(vali.RGB, 64, 32, gpu)
    assert enc.Run(ctx, [good, vali.Surface.Make(vali.BGR, 64, 32, gpu)]) == ([], vali.TaskExecInfo.FAIL)
    assert enc.Run(ctx, [good, None]) == ([], vali.TaskExecInfo.FAIL)
    assert enc.Run(ctx, [good, vali.Surface(vali.RGB)]) == ([], vali.TaskExecInfo.FAIL)
    assert enc.Run(enc.Context(90, vali.YUV420, optimize=True), [vali.Surface.Make(vali.YUV420, 33, 32, gpu)]) == (
        [], vali.TaskExecInfo.FAIL)
    out, info = enc.Run(ctx, [good])
    assert info == vali.TaskExecInfo.SUCCESS and len(out) == 1
    with pytest.raises(ValueError):
        enc.Context(90, vali.RGB, optimize=1)


@gpu_test
def test_graph_capture_replays_on_new_pixels(vali, gpu, frame):
    """the optimised path neither allocates nor synchronises either: captured once (the clearing of the histograms
    included), replayed on new pixels"""
    from vali_amd._native import shim

    w, h, n = 160, 96, 3
    fmt = jm.YUV420
    hosts = [jm.make_host(fmt, w, h, "frame", seed=i, frame=np.roll(frame, 37 * i, 1)) for i in range(n)]
    surfs = [upload(vali, gpu, fmt, hst, w, h) for hst in hosts]
    p = shim.jpeg_params_init(80, fmt)
    p.optimize = 1
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
        fixed = om.fixed_header(w, h, fmt, 80)
        for i in range(n):
            assert fixed + first[i] + b"\xff\xd9" == om.encode(fmt, hosts[i], w, h, 80), i
        hosts2 = hosts[1:] + hosts[:1]
        for s, hst in zip(surfs, hosts2):
            assert vali.PyFrameUploader(gpu).Run(hst, s)[0]
        capture.Launch()
        assert read() == first[1:] + first[:1]
        del capture
    finally:
        for ptr in (d_src, ws, out, sizes):
            shim.mem_free(gpu, ptr)
        shim.stream_destroy(gpu, stream)


# ---- a photograph ----------------------------------------------------------------------------------------------------------
@gpu_test
def test_a_photograph_gets_smaller_by_what_the_model_says(vali, gpu, enc, frame):
    w = h = 256
    host = jm.make_host(jm.RGB, w, h, "frame", frame=frame)
    s = upload(vali, gpu, jm.RGB, host, w, h)
    ours = run(vali, enc, jm.RGB, 90, [s], "420")[0]
    plain = run(vali, enc, jm.RGB, 90, [s], "420", optimize=False)[0]
    want = om.encode(jm.RGB, host, w, h, 90, "420")
    print(f"\njpeg_optimize photograph 256x256 q90 4:2:0: plain {len(plain)} bytes, optimised {len(ours)} bytes, "
          f"ratio {len(ours) / len(plain):.3f}")
    assert len(ours) < len(plain)
    assert len(ours) == len(want) and ours == want
