#!/usr/bin/env python3
"""Writing WHAT a detector found: NV12 frames + a detections tensor on the GPU -> labelled JPEG files, no box and no class
id ever on the host.

  class names  --vali.LabelAtlas, once-->  a coverage atlas on the GPU, one strip per class, and rects (L, 4)
  detections (K, 6) on the GPU: frame, x, y, w, h, class
               --torch, on the device-->  marks (3K, 8) int32: per detection an outline (MARK_BOX), the label's
                                          background (MARK_FILL) and its text (MARK_STAMP from the atlas)
               --PySurfaceAnnotator.RunBatch(..., atlas=...)-->  drawn IN PLACE onto the NV12 frames, two launches
               --PySurfaceConverter NV12 -> YUV420, PyNvJpegEncoder(backend="hip").Run-->  one 4:2:0 JPEG file per frame
                 (the frames as they are would go to PyNvEncoder; the JPEG encoder takes planar 4:2:0)

The label of a detection is the strip rects[class] of the atlas: gathering it is an index operation on the device.

    python examples/label_detections.py

Runs on synthetic frames and made-up detections; needs Pillow for the text."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import python_vali as vali  # noqa: E402

import torch  # noqa: E402

CLASSES = ["person", "bicycle", "car", "dog", "traffic light"]


def detector(batch, w, h, per_frame, device):
    """a stand-in for a detector's output: (K, 6) int32 rows (frame, x, y, w, h, class), made up on the device"""
    g = torch.Generator(device=device).manual_seed(0)
    k = batch * per_frame
    frame = torch.arange(k, device=device, dtype=torch.int32) // per_frame
    bw = torch.randint(60, 300, (k,), device=device, generator=g, dtype=torch.int32)
    bh = torch.randint(60, 300, (k,), device=device, generator=g, dtype=torch.int32)
    x = torch.randint(0, w - 60, (k,), device=device, generator=g, dtype=torch.int32)
    y = torch.randint(0, h - 60, (k,), device=device, generator=g, dtype=torch.int32)
    cls = torch.randint(0, len(CLASSES), (k,), device=device, generator=g, dtype=torch.int32)
    return torch.stack([frame, x, y, bw, bh, cls], 1)


def marks_of(det, rects):
    """(K, 6) detections and the atlas's (L, 4) rects, both on the device -> (3K, 8) marks: all outlines, then all label
    backgrounds, then all texts (marks are applied in row order).  The label sits on top of its box's upper edge."""
    k = det.shape[0]
    dev = det.device

    def rows(x, y, w, h, kind, arg, colour):
        cols = [det[:, 0], x, y, w, h] + [v if torch.is_tensor(v) else torch.full((k,), v, dtype=torch.int32, device=dev)
                                          for v in (kind, arg, colour)]
        return torch.stack(cols, 1)

    r = rects[det[:, 5].long()]                                    # (u, v, w, h) of each detection's label
    lx, ly = det[:, 1], det[:, 2] - r[:, 3]                        # (a label above the frame's top edge is clipped)
    green = vali.pack_colour(40, 255, 80)
    outline = rows(det[:, 1], det[:, 2], det[:, 3], det[:, 4], vali.MARK_BOX, 2, green)
    background = rows(lx, ly, r[:, 2], r[:, 3], vali.MARK_FILL, 0, vali.pack_colour(40, 255, 80, 200))
    text = rows(lx, ly, r[:, 2], r[:, 3], vali.MARK_STAMP, r[:, 0] | r[:, 1] << 16, vali.pack_colour(0, 0, 0))
    return torch.cat([outline, background, text], 0).contiguous()


def main():
    gpu_id, batch, w, h = 0, 4, 1280, 720
    device = f"cuda:{gpu_id}"
    rng = np.random.default_rng(0)
    up = vali.PyFrameUploader(gpu_id)
    frames = [vali.Surface.Make(vali.PixelFormat.NV12, w, h, gpu_id) for _ in range(batch)]
    for f in frames:
        assert up.Run(rng.integers(0, 256, w * h * 3 // 2, dtype=np.uint8), f)[0]

    labels = vali.LabelAtlas(gpu_id, CLASSES, pad=2)               # rendered and uploaded once
    rects = torch.from_numpy(labels.rects).to(device)
    marks = marks_of(detector(batch, w, h, 6, device), rects)
    torch.cuda.synchronize()                          # the producer has finished before another stream reads the tensor

    ann = vali.PySurfaceAnnotator(gpu_id)
    enc = vali.PyNvJpegEncoder(gpu_id, backend="hip")
    ab = ann.PrepareBatch(frames)
    ok, info = ann.RunBatch(ab, marks, atlas=labels.surface)       # two launches
    assert ok, info
    cvt = vali.PySurfaceConverter(gpu_id)
    cc = vali.ColorspaceConversionContext(vali.ColorSpace.BT_601, vali.ColorRange.JPEG)
    planar = [vali.Surface.Make(vali.PixelFormat.YUV420, w, h, gpu_id) for _ in range(batch)]
    for src, dst in zip(frames, planar):
        ok, info = cvt.Run(src, dst, cc)
        assert ok, info
    files, info = enc.Run(enc.Context(90, vali.PixelFormat.YUV420), planar)
    assert info == vali.TaskExecInfo.SUCCESS, info
    for i, f in enumerate(files):
        print(f"frame {i}: {w}x{h} NV12, {marks.shape[0] // batch} marks, {f.size} bytes of JPEG")


if __name__ == "__main__":
    main()
