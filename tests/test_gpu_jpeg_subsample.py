"""PyNvJpegEncoder(backend="hip") with Context(..., subsampling="420" / "422") on RGB, BGR and RGB_PLANAR surfaces: every
file equals the numpy model (tests/jpeg_subsample_model.py, pinned to Pillow's libjpeg-turbo by
tests/test_jpeg_subsample_host.py) byte for byte."""
import io
import re
from pathlib import Path

import numpy as np
import pytest

import jpeg_model as jm
import jpeg_subsample_model as sm

PIL = pytest.importorskip("PIL.Image")
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"

gpu_test = pytest.mark.gpu

NAMES = {jm.RGB: "RGB", jm.BGR: "BGR", jm.RGB_PLANAR: "RGB_PLANAR"}
# 20x20, 50x7, 130x70: chroma columns past the component's width (the horizontal rule); 16x17, 33x31: an odd last row (the
# vertical rule); 15x9, 7x50, 1x1: dummy luma blocks; 130x70: several restart segments and a partial last one
SIZES = [(1, 1), (16, 16), (17, 16), (16, 17), (15, 9), (20, 20), (33, 31), (50, 7), (7, 50), (130, 70), (424, 232)]


@pytest.fixture(scope="module")
def frame():
    return np.asarray(PIL.open(GOLDEN / "frame_0.jpg").convert("RGB"))


def upload(vali, gpu, fmt, host, w, h):
    s = vali.Surface.Make(vali.PixelFormat(fmt), w, h, gpu)
    assert s.HostSize == host.size
    ok, info = vali.PyFrameUploader(gpu).Run(host, s)
    assert ok, info
    return s


def encode(vali, gpu, fmt, q, surfaces, samp, backend="hip"):
    enc = vali.PyNvJpegEncoder(gpu, backend=backend)
    ctx = enc.Context(q, vali.PixelFormat(fmt), subsampling=samp)
    if samp is not None:
        assert ctx.Subsampling() == samp
    out, info = enc.Run(ctx, surfaces)
    assert info == vali.TaskExecInfo.SUCCESS
    return [bytes(b.tobytes()) for b in out]


@gpu_test
@pytest.mark.parametrize("samp", ["420", "422"])
@pytest.mark.parametrize("fmt", list(NAMES), ids=NAMES.get)
def test_file_equals_model(vali, gpu, frame, fmt, samp):
    """all sizes in one call (one launch per size); the qualities the host test pins to Pillow"""
    hosts = [jm.make_host(fmt, w, h, "frame" if w > 64 else "noise", seed=w + h, frame=frame) for w, h in SIZES]
    surfs = [upload(vali, gpu, fmt, hst, w, h) for hst, (w, h) in zip(hosts, SIZES)]
    for q in (50, 90) if fmt == jm.RGB else (90,):
        got = encode(vali, gpu, fmt, q, surfs, samp)
        for g, hst, (w, h) in zip(got, hosts, SIZES):
            want = sm.encode(fmt, hst, w, h, q, samp)
            assert g == want, (NAMES[fmt], samp, w, h, q, len(g), len(want))


@gpu_test
@pytest.mark.parametrize("samp", ["420", "422"])
def test_decodes_like_the_cpu_backend(vali, gpu, frame, samp):
    for w, h in [(424, 232), (33, 31)]:
        host = jm.make_host(jm.RGB, w, h, "frame", frame=frame)
        s = upload(vali, gpu, jm.RGB, host, w, h)
        ours = encode(vali, gpu, jm.RGB, 90, [s], samp)[0]
        theirs = encode(vali, gpu, jm.RGB, 90, [s], samp, backend="cpu")[0]
        assert theirs == sm.pillow_encode(jm.RGB, host, w, h, 90, samp)
        a, b = PIL.open(io.BytesIO(ours)), PIL.open(io.BytesIO(theirs))
        assert a.layer[0][1:3] == b.layer[0][1:3] == sm.SAMPLINGS[samp]
        assert a.mode == b.mode and np.array_equal(np.asarray(a), np.asarray(b))


@gpu_test
def test_batch_of_mixed_sizes_equals_single_frames(vali, gpu, frame):
    sizes = [(130, 70), (130, 70), (33, 31), (130, 70), (33, 31)]
    hosts = [jm.make_host(jm.BGR, w, h, ["noise", "frame", "flat"][i % 3], seed=i, frame=frame)
             for i, (w, h) in enumerate(sizes)]
    surfs = [upload(vali, gpu, jm.BGR, hst, w, h) for hst, (w, h) in zip(hosts, sizes)]
    batch = encode(vali, gpu, jm.BGR, 75, surfs, "420")
    for i, s in enumerate(surfs):
        assert batch[i] == encode(vali, gpu, jm.BGR, 75, [s], "420")[0], i
        assert batch[i] == sm.encode(jm.BGR, hosts[i], *sizes[i], 75, "420"), i


@gpu_test
@pytest.mark.parametrize("samp", ["420", "422"])
def test_pitched_dlpack_surface_and_a_view(vali, gpu, frame, samp):
    """a pitched surface (aligned dword loads in the interior, byte loads at the edge) and a view whose rows start 7
    bytes off a dword (byte loads everywhere)"""
    import torch

    w, h = 200, 121
    host = jm.make_host(jm.RGB, w, h, "frame", frame=frame).reshape(h, 3 * w)
    want = sm.encode(jm.RGB, host, w, h, 90, samp)
    big = torch.zeros((2 * h + 8, 3 * w + 161), dtype=torch.uint8, device=f"cuda:{gpu}")
    big[:h, :3 * w] = torch.from_numpy(host).to(big.device)
    big[h + 5:2 * h + 5, 7:7 + 3 * w] = torch.from_numpy(host).to(big.device)
    torch.cuda.synchronize()
    pitched = vali.Surface.from_dlpack(torch.utils.dlpack.to_dlpack(big[:h, :3 * w]))
    view = vali.Surface.from_dlpack(torch.utils.dlpack.to_dlpack(big[h + 5:2 * h + 5, 7:7 + 3 * w]))
    assert pitched.Pitch == 3 * w + 161 and (pitched.Width, pitched.Height) == (w, h)
    assert encode(vali, gpu, jm.RGB, 90, [pitched], samp)[0] == want
    assert encode(vali, gpu, jm.RGB, 90, [view], samp)[0] == want


@gpu_test
@pytest.mark.parametrize("samp", ["420", "422"])
@pytest.mark.parametrize("content", ["checker", "binary"])
def test_checkerboard_and_binary_noise(vali, gpu, content, samp):
    """the one-pixel checkerboard leaves every chroma sample to the alternating bias; binary noise at q 100 is the
    longest codes"""
    for fmt, (w, h) in ((jm.RGB, (50, 39)), (jm.RGB_PLANAR, (64, 48))):
        host = sm.make_host(fmt, w, h, content, seed=11)
        s = upload(vali, gpu, fmt, host, w, h)
        for q in (100, 1):
            assert encode(vali, gpu, fmt, q, [s], samp)[0] == sm.encode(fmt, host, w, h, q, samp), (w, h, q)


@gpu_test
@pytest.mark.parametrize("fmt", list(NAMES) + [jm.YUV420], ids=lambda f: NAMES.get(f, "YUV420"))
def test_444_and_the_own_sampling_equal_no_argument(vali, gpu, frame, fmt):
    w, h = 130, 70
    host = jm.make_host(fmt, w, h, "frame", frame=frame)
    s = upload(vali, gpu, fmt, host, w, h)
    own = "420" if fmt == jm.YUV420 else "444"
    for backend in ("hip", "cpu"):
        a = encode(vali, gpu, fmt, 90, [s], None, backend)[0]
        b = encode(vali, gpu, fmt, 90, [s], own, backend)[0]
        assert a == b
        if backend == "hip":
            assert a == jm.encode(fmt, host, w, h, 90)


@gpu_test
def test_round_trip_into_nv12(vali, gpu, frame):
    """a "420" file of an even-sized RGB surface decodes with PyNvJpegDecoder to the NV12 surface the decoder model
    gives: the file our own encoder writes that PySurfacePreprocessor takes"""
    import jpeg_decode_model as dm

    w, h = 424, 232
    host = jm.make_host(jm.RGB, w, h, "frame", frame=frame)
    data = encode(vali, gpu, jm.RGB, 90, [upload(vali, gpu, jm.RGB, host, w, h)], "420")[0]
    dec = vali.PyNvJpegDecoder(gpu)
    info = dec.Info(data)
    assert (info.width, info.height, info.sampling, info.restart_interval) == (w, h, "420", 10)
    surfs, status = dec.Run([data], vali.NV12)
    assert status == vali.TaskExecInfo.SUCCESS and surfs[0].Format == vali.NV12
    got = np.zeros(surfs[0].HostSize, np.uint8)
    assert vali.PySurfaceDownloader(gpu).Run(surfs[0], got)[0]
    assert np.array_equal(got, dm.surface_bytes(data, "NV12"))


def test_new_instantiations_use_no_scratch():
    """the compiler's resource remarks of the build (tests/test_kernel_resources.py reads them the same way): the six
    subsampled forms of k_jpeg_fdct exist, and none uses scratch or spills"""
    report = ROOT / "vali_amd" / "csrc" / "_obj" / "jpeg.resources.txt"
    kernels, name = {}, None
    for line in report.read_text().splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (-?\d+)", line)
        if m and name:
            kernels[name][m.group(1).strip()] = int(m.group(2))
    for src in (1, 2, 3):                   # SRC_RGB, SRC_BGR, SRC_RGB_PLANAR
        for cs in (0, 1, 2):                # 4:4:4, 4:2:2, 4:2:0
            hits = [r for n, r in kernels.items() if f"k_jpeg_fdctILi{src}ELi{cs}EE" in n]
            assert len(hits) == 1, (src, cs, sorted(kernels))
            r = hits[0]
            assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (src, cs, r)
            assert r["Occupancy"] >= 2, (src, cs, r)            # 4:4:4 has always had two waves per SIMD
    assert [n for n in kernels if "k_jpeg_fdctILi0ELi0EE" in n]                     # planar YUV: one form
    assert not [n for n in kernels if re.search(r"k_jpeg_fdctILi0ELi[12]EE", n)]
