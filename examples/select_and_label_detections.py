#!/usr/bin/env python3
"""From a network's RAW head to labelled JPEG files with no torch glue and no box on the host:

  NV12 frames  --PySurfacePreprocessor.RunTensorBatch (letterbox)-->  (N, 3, 640, 640) float16, and the records it was
                                                                      placed with
  the network  -->  a YOLOv8 head (N, 4 + C, K): cx, cy, w, h and C class scores per candidate, network coordinates
  the head     --PyDetectionSelector.Run, four launches-->  dets (N * D, 8) in FRAME pixels, counts, and marks (3 * N * D, 8):
                                                            threshold, class arg-max, exact top-T, NMS, the way back
                                                            through the letterbox, outline + label rows per detection
  marks        --PySurfaceAnnotator.RunBatch(..., atlas=)-->  drawn in place onto the NV12 frames, two launches
  frames       --PySurfaceConverter, PyNvJpegEncoder(backend="hip")-->  one JPEG file per frame

The head's two parts go in as transposed slices of the network's output, without a copy; nothing between the network
and the encoder reads a detection on the host (the counts are fetched at the end, for the printout).

    python examples/select_and_label_detections.py

Runs on synthetic frames and a made-up head; needs Pillow for the label text."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import python_vali as vali  # noqa: E402

import torch  # noqa: E402

CLASSES = ["person", "bicycle", "car", "dog", "traffic light"]
K, D = 8400, 20


def network(x):
    """a stand-in for a detector: a raw YOLOv8 head (N, 4 + C, K) float16 for the input batch `x`, made up on the device --
    a few hundred candidates per frame score above the threshold, in clusters that NMS has to thin out"""
    n, dev = x.shape[0], x.device
    g = torch.Generator(device=dev).manual_seed(0)
    centre = torch.rand((n, 12, 2), device=dev, generator=g) * torch.tensor([560.0, 280.0], device=dev) + \
        torch.tensor([40.0, 180.0], device=dev)
    which = torch.randint(0, 12, (n, K), device=dev, generator=g)
    cxcy = centre.gather(1, which[..., None].expand(-1, -1, 2)) + torch.randn((n, K, 2), device=dev, generator=g) * 4
    wh = 60 + torch.rand((n, K, 2), device=dev, generator=g) * 30
    scores = torch.rand((n, K, len(CLASSES)), device=dev, generator=g) * 0.2
    hot = torch.rand((n, K), device=dev, generator=g) < 0.03
    cls = which % len(CLASSES)
    scores.scatter_add_(2, cls[..., None], torch.where(hot, 0.35 + 0.45 * torch.rand((n, K), device=dev, generator=g),
                                                       torch.zeros((n, K), device=dev))[..., None])
    return torch.cat([cxcy, wh, scores], 2).transpose(1, 2).contiguous().half()


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

    pred = network(x)                                                 # (N, 4 + C, K)
    torch.cuda.synchronize()                                          # the producer has finished before another stream reads

    # head -> detections, counts and annotator rows, all on the GPU
    labels = vali.LabelAtlas(gpu_id, CLASSES, pad=2)                  # rendered and uploaded once
    style = vali.DetectionStyle(thickness=2, colours=[vali.pack_colour(40, 255, 80), vali.pack_colour(255, 200, 0),
                                                      vali.pack_colour(80, 160, 255)], label_rects=labels.rects)
    dets = torch.zeros((batch * D, 8), dtype=torch.int32, device=device)
    counts = torch.zeros((batch,), dtype=torch.int32, device=device)
    marks = torch.zeros((3 * batch * D, 8), dtype=torch.int32, device=device)
    torch.cuda.synchronize()
    sel = vali.PyDetectionSelector(gpu_id)
    sb = sel.Prepare(pred[:, :4].transpose(1, 2), pred[:, 4:].transpose(1, 2), dets, counts, marks=marks,
                     box_format="cxcywh", max_candidates=1024, max_det=D)
    ok, info = sel.Run(sb, tb.rects, score_thr=0.25, iou_thr=0.45, style=style)          # four launches
    assert ok, info

    ann = vali.PySurfaceAnnotator(gpu_id)
    ok, info = ann.RunBatch(ann.PrepareBatch(frames), marks, atlas=labels.surface)          # two launches
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
    first = dets[:found[0]].cpu().numpy()
    for i, f in enumerate(files):
        print(f"frame {i}: {found[i]} detections, {f.size} bytes of JPEG")
    for row in first[:3]:
        print(f"  frame 0: {CLASSES[row[5]]} {row[6:7].view(np.float32)[0]:.2f} at ({row[1]}, {row[2]}) {row[3]} x {row[4]}")


if __name__ == "__main__":
    main()
