#!/usr/bin/env python3
"""From a segmentation network's RAW outputs to JPEG files with the instance masks painted on, with no torch glue and no
box or mask on the host:

  NV12 frames  --PySurfacePreprocessor.RunTensorBatch (letterbox)-->  (N, 3, 640, 640) float16, and the records it was
                                                                      placed with
  the network  -->  a YOLOv8-seg head (N, 4 + C + M, K): cx, cy, w, h, C class scores and M mask coefficients per
                    candidate, and prototypes (N, M, 160, 160)
  the head     --PyDetectionSelector.Run, four launches-->  dets (N * D, 8) in FRAME pixels (their `k` is the candidate's
                                                            index in the head), counts, and marks (N * D, 8) outlines
  dets         --PyInstanceMasker.Run, two launches-->  the mask of every detection -- coeffs[k] . protos, upsampled to the
                                                        frame, > 0 -- blended in place onto the NV12 frames, inside its box
  marks        --PySurfaceAnnotator.RunBatch, two launches-->  the outlines on top
  frames       --PySurfaceConverter, PyNvJpegEncoder(backend="hip")-->  one JPEG file per frame

The head's three parts go in as transposed slices of the network's output, without a copy; nothing between the network
and the encoder reads a detection on the host (the counts are fetched at the end, for the printout).

    python examples/segment_and_paint.py

Runs on synthetic frames and a made-up head."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import python_vali as vali  # noqa: E402

import torch  # noqa: E402

C, M, K, D = 5, 32, 8400, 20


def network(x):
    """a stand-in for a segmentation network: a raw YOLOv8-seg head (N, 4 + C + M, K) and prototypes (N, M, 160, 160),
    float16, made up on the device -- clusters of candidates that NMS has to thin out, smooth prototypes"""
    n, dev = x.shape[0], x.device
    g = torch.Generator(device=dev).manual_seed(0)
    centre = torch.rand((n, 12, 2), device=dev, generator=g) * torch.tensor([520.0, 240.0], device=dev) + \
        torch.tensor([60.0, 200.0], device=dev)
    which = torch.randint(0, 12, (n, K), device=dev, generator=g)
    cxcy = centre.gather(1, which[..., None].expand(-1, -1, 2)) + torch.randn((n, K, 2), device=dev, generator=g) * 4
    wh = 80 + torch.rand((n, K, 2), device=dev, generator=g) * 60
    scores = torch.rand((n, K, C), device=dev, generator=g) * 0.2
    hot = torch.rand((n, K), device=dev, generator=g) < 0.03
    scores.scatter_add_(2, (which % C)[..., None], torch.where(hot, 0.35 + 0.45 * torch.rand((n, K), device=dev, generator=g),
                                                               torch.zeros((n, K), device=dev))[..., None])
    coeffs = torch.randn((n, K, M), device=dev, generator=g)
    yy, xx = torch.meshgrid(torch.arange(160, device=dev) / 160.0, torch.arange(160, device=dev) / 160.0, indexing="ij")
    freq = torch.rand((n, M, 2), device=dev, generator=g) * 10 - 5
    phase = torch.rand((n, M), device=dev, generator=g) * 6.283
    protos = torch.sin(6.283 * (freq[..., 0, None, None] * xx + freq[..., 1, None, None] * yy) + phase[..., None, None])
    return torch.cat([cxcy, wh, scores, coeffs], 2).transpose(1, 2).contiguous().half(), protos.half()


def main():
    gpu_id, batch, w, h = 0, 4, 1280, 720
    device = f"cuda:{gpu_id}"
    rng = np.random.default_rng(0)
    up = vali.PyFrameUploader(gpu_id)
    frames = [vali.Surface.Make(vali.PixelFormat.NV12, w, h, gpu_id) for _ in range(batch)]
    for f in frames:
        assert up.Run(rng.integers(0, 256, w * h * 3 // 2, dtype=np.uint8), f)[0]
    cc = vali.ColorspaceConversionContext(vali.ColorSpace.BT_709, vali.ColorRange.MPEG)

    # frames -> network input, letterboxed; tb.rects are the records the frames were placed with
    pre = vali.PySurfacePreprocessor(gpu_id, div=255.0)
    x = torch.zeros((batch, 3, 640, 640), dtype=torch.float16, device=device)
    torch.cuda.synchronize()
    tb = pre.PrepareTensorBatch(frames, x, None, [vali.letterbox_rect(w, h, 640, 640)] * batch)
    ok, info = pre.RunTensorBatch(tb, pad=(114, 114, 114), cc_ctx=cc)
    assert ok, info

    pred, protos = network(x)                                         # (N, 4 + C + M, K), (N, M, 160, 160)
    torch.cuda.synchronize()                                          # the producer has finished before another stream reads

    # head -> detections and outline rows, all on the GPU
    colours = [vali.pack_colour(40, 255, 80), vali.pack_colour(255, 200, 0), vali.pack_colour(80, 160, 255)]
    dets = torch.zeros((batch * D, 8), dtype=torch.int32, device=device)
    counts = torch.zeros((batch,), dtype=torch.int32, device=device)
    marks = torch.zeros((batch * D, 8), dtype=torch.int32, device=device)
    torch.cuda.synchronize()
    sel = vali.PyDetectionSelector(gpu_id)
    sb = sel.Prepare(pred[:, :4].transpose(1, 2), pred[:, 4:4 + C].transpose(1, 2), dets, counts, marks=marks,
                     box_format="cxcywh", max_candidates=1024, max_det=D)
    ok, info = sel.Run(sb, tb.rects, score_thr=0.25, iou_thr=0.45, style=vali.DetectionStyle(2, colours))   # four launches
    assert ok, info

    # dets -> masks on the frames: the coefficients are the head's last M channels, as they lie
    mk = vali.PyInstanceMasker(gpu_id)
    mb = mk.Prepare(frames, protos, pred[:, 4 + C:].transpose(1, 2), dets, max_det=D, net_size=(640, 640))
    ok, info = mk.Run(mb, tb.rects, colours, alpha=110, cc_ctx=cc)                                          # two launches
    assert ok, info

    ann = vali.PySurfaceAnnotator(gpu_id)
    ok, info = ann.RunBatch(ann.PrepareBatch(frames), marks, cc_ctx=cc)                                     # two launches
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
    found = counts.cpu().tolist()
    for i, f in enumerate(files):
        print(f"frame {i}: {found[i]} detections with their masks, {f.size} bytes of JPEG")


if __name__ == "__main__":
    main()
