"""Frames -> network input -> a semantic head -> painter -> JPEG on one small batch: NV12 frames are letterboxed by
PySurfacePreprocessor.RunTensorBatch, a synthetic head turns the network input into class logits on the device,
PySemanticPainter labels and tints the frames through the records the batch was placed with, and the frames are encoded.
The frames and labels equal tests/semantic_model.py fed with the logits read back afterwards, and the JPEG files those of
the model's frames."""
import numpy as np
import pytest

import postproc_model as pm
import semantic_model as sm
from test_gpu_annotate import download, make_frames

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SIZES = [(96, 80), (70, 50), (96, 80)]
NET = (64, 64)
C = 6


def head(x):
    """a stand-in for a segmentation network: (N, 3, 64, 64) -> (N, C, 16, 16) float16 logits, smooth functions of the
    picture so that classes form regions"""
    import torch.nn.functional as F

    pooled = F.avg_pool2d(x.float(), 4)
    g = torch.Generator(device="cpu").manual_seed(3)
    mix = (torch.randn((C, 3), generator=g) * 6).to(x.device)
    yy, xx = torch.meshgrid(torch.arange(16, device=x.device) / 16.0, torch.arange(16, device=x.device) / 16.0, indexing="ij")
    waves = torch.stack([torch.sin(6.283 * ((k % 3 + 1) * 0.5 * xx + (k // 3 + 0.5) * yy) + k) for k in range(C)])
    return (torch.einsum("cj,njyx->ncyx", mix, pooled) + 2 * waves[None]).half()


def jpegs(vali, gpu, frames):
    cvt, enc = vali.PySurfaceConverter(gpu), vali.PyNvJpegEncoder(gpu, backend="hip")
    jcc = vali.ColorspaceConversionContext(vali.ColorSpace.BT_601, vali.ColorRange.JPEG)
    planar = [vali.Surface.Make(vali.PixelFormat.YUV420, f.Width, f.Height, gpu) for f in frames]
    for src, dst in zip(frames, planar):
        assert cvt.Run(src, dst, jcc)[0]
    files, info = enc.Run(enc.Context(90, vali.PixelFormat.YUV420), planar)
    assert info == vali.TaskExecInfo.SUCCESS, info
    return [np.asarray(f).tobytes() for f in files]


def test_frames_to_jpeg_through_a_semantic_head(vali, gpu):
    dev = f"cuda:{gpu}"
    frames, hosts = make_frames(vali, gpu, "NV12", SIZES, seed=41)
    labels = [vali.Surface.Make(vali.Y, w, h, gpu) for w, h in SIZES]
    x = torch.zeros((len(SIZES), 3, NET[1], NET[0]), dtype=torch.float16, device=dev)
    torch.cuda.synchronize()
    pre = vali.PySurfacePreprocessor(gpu, div=255.0)
    tb = pre.PrepareTensorBatch(frames, x, None, [vali.letterbox_rect(w, h, *NET) for w, h in SIZES])
    assert pre.RunTensorBatch(tb, pad=(114, 114, 114))[0]
    logits = head(x)
    torch.cuda.synchronize()

    colours = [vali.pack_colour(*rgb) for rgb in ((230, 40, 40), (40, 200, 60), (30, 60, 240), (240, 220, 30), (200, 40, 220))]
    sp = vali.PySemanticPainter(gpu)
    sb = sp.Prepare(frames, logits, labels, net_size=NET)
    cc = pm.cc_ctx_of(vali, "601_JPEG")
    assert sp.Run(sb, tb.rects, colours, alpha=110, cc_ctx=cc) == (True, vali.TaskExecInfo.SUCCESS)

    rects = [tuple(int(v) for v in r) for r in tb.rects]
    assert rects[0][:4] == (0, 0, 96, 80) and rects[1][:4] == (0, 0, 70, 50)
    maps = sm.apply(hosts, "NV12", SIZES, logits.float().cpu().numpy(), rects, colours, 110, NET, pm.matrices()["601_JPEG"])
    for i, (f, l) in enumerate(zip(frames, labels)):
        assert len(np.unique(maps[i])) >= 3 and (maps[i] != 255).all(), i
        assert np.array_equal(download(vali, gpu, f), hosts[i]), i
        assert np.array_equal(download(vali, gpu, l), maps[i].reshape(-1)), i

    got = jpegs(vali, gpu, frames)
    again = [vali.Surface.Make(vali.NV12, w, h, gpu) for w, h in SIZES]
    for s, host in zip(again, hosts):
        assert vali.PyFrameUploader(gpu).Run(host, s)[0]
    want = jpegs(vali, gpu, again)
    assert got == want and all(len(b) > 200 and b[:2] == b"\xff\xd8" for b in got)
