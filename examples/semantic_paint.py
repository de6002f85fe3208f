#!/usr/bin/env python3
"""From a semantic segmentation network's RAW logits to a class map per frame and JPEG files with the classes tinted on,
with no F.interpolate, no argmax and no (N, C, H, W) tensor:

  NV12 frames  --PySurfacePreprocessor.RunTensorBatch (letterbox)-->  (N, 3, 512, 512) float16, and the records it was
                                                                      placed with
  the network  -->  class logits (N, C, 128, 128), a quarter of the input, as DeepLab, SegFormer or BiSeNet return them
  the logits   --PySemanticPainter.Run, one launch-->  labels: a Y surface per frame holding the class of every frame
                                                       pixel (255 outside the picture's rectangle), and the classes
                                                       blended in place onto the NV12 frames in the palette's colours
  frames       --PySurfaceConverter, PyNvJpegEncoder(backend="hip")-->  one JPEG file per frame

The class maps stay on the GPU as surfaces (Surface.PlanePtr / __dlpack__ for whatever comes next); here one is
downloaded for the printout.

    python examples/semantic_paint.py

Runs on synthetic frames and a made-up head."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import python_vali as vali  # noqa: E402

import torch  # noqa: E402

C = 19          # Cityscapes


def network(x):
    """a stand-in for a segmentation network: smooth logits (N, C, H / 4, W / 4), float16, made up on the device"""
    n, dev = x.shape[0], x.device
    hs, ws = x.shape[2] // 4, x.shape[3] // 4
    g = torch.Generator(device=dev).manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(hs, device=dev) / hs, torch.arange(ws, device=dev) / ws, indexing="ij")
    freq = torch.rand((n, C, 2), device=dev, generator=g) * 3 - 1.5
    phase = torch.rand((n, C), device=dev, generator=g) * 6.283
    return (4 * torch.sin(6.283 * (freq[..., 0, None, None] * xx + freq[..., 1, None, None] * yy) + phase[..., None, None])).half()


def main():
    gpu_id, batch, w, h = 0, 4, 1920, 1080
    device = f"cuda:{gpu_id}"
    rng = np.random.default_rng(0)
    up = vali.PyFrameUploader(gpu_id)
    frames = [vali.Surface.Make(vali.PixelFormat.NV12, w, h, gpu_id) for _ in range(batch)]
    for f in frames:
        assert up.Run(rng.integers(0, 256, w * h * 3 // 2, dtype=np.uint8), f)[0]
    cc = vali.ColorspaceConversionContext(vali.ColorSpace.BT_709, vali.ColorRange.MPEG)

    # frames -> network input, letterboxed; tb.rects are the records the frames were placed with
    pre = vali.PySurfacePreprocessor(gpu_id, div=255.0)
    x = torch.zeros((batch, 3, 512, 512), dtype=torch.float16, device=device)
    torch.cuda.synchronize()
    tb = pre.PrepareTensorBatch(frames, x, None, [vali.letterbox_rect(w, h, 512, 512)] * batch)
    ok, info = pre.RunTensorBatch(tb, pad=(114, 114, 114), cc_ctx=cc)
    assert ok, info

    logits = network(x)                                               # (N, C, 128, 128)
    torch.cuda.synchronize()

    # logits -> labels and tinted frames
    palette = [vali.pack_colour(*(int(v) for v in rng.integers(0, 256, 3))) for _ in range(C)]
    labels = [vali.Surface.Make(vali.PixelFormat.Y, w, h, gpu_id) for _ in range(batch)]
    sp = vali.PySemanticPainter(gpu_id)
    sb = sp.Prepare(frames, logits, labels, net_size=(512, 512))
    ok, info = sp.Run(sb, tb.rects, palette, alpha=110, cc_ctx=cc)                                          # one launch
    assert ok, info

    cvt = vali.PySurfaceConverter(gpu_id)
    enc = vali.PyNvJpegEncoder(gpu_id, backend="hip")
    jcc = vali.ColorspaceConversionContext(vali.ColorSpace.BT_601, vali.ColorRange.JPEG)
    planar = [vali.Surface.Make(vali.PixelFormat.YUV420, w, h, gpu_id) for _ in range(batch)]
    for src, dst in zip(frames, planar):
        ok, info = cvt.Run(src, dst, jcc)
        assert ok, info
    files, info = enc.Run(enc.Context(90, vali.PixelFormat.YUV420), planar)
    assert info == vali.TaskExecInfo.SUCCESS, info
    host = np.zeros(w * h, np.uint8)
    for i, f in enumerate(files):
        assert vali.PySurfaceDownloader(gpu_id).Run(labels[i], host)[0]
        share = np.bincount(host, minlength=C)[:C] / host.size
        top = ", ".join(f"class {c}: {share[c]:.0%}" for c in np.argsort(-share)[:3])
        print(f"frame {i}: {top}; {f.size} bytes of JPEG")


if __name__ == "__main__":
    main()
