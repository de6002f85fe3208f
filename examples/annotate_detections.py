#!/usr/bin/env python3
"""Drawing what a detector found: frames + a boxes tensor on the GPU -> annotated JPEG files, no box ever on the host.

  RGB frames, boxes (K, 5) on the GPU  --torch, on the device-->  marks (2K, 8) int32 on the GPU
               --PySurfaceAnnotator.RunBatchAsync-->  every box outlined, every second one pixelated, IN PLACE
               --PyNvJpegEncoder(backend="hip").Run-->  one JPEG file per frame

The annotator and the encoder work on the same stream, so nothing synchronises between drawing and encoding, and the
boxes are never copied to the host: the marks tensor is built from them with torch on the device.  The torch chain this
replaces (slice assignments on DLPack views) needs the boxes on the host and four launches per box and plane.

    python examples/annotate_detections.py

Runs on synthetic frames and made-up boxes."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import python_vali as vali  # noqa: E402

import torch  # noqa: E402


def detector(batch, w, h, per_frame, device):
    """a stand-in for a detector's output: (K, 5) int32 rows (frame, x, y, w, h), made up on the device"""
    g = torch.Generator(device=device).manual_seed(0)
    k = batch * per_frame
    frame = torch.arange(k, device=device, dtype=torch.int32) // per_frame
    bw = torch.randint(40, 240, (k,), device=device, generator=g, dtype=torch.int32)
    bh = torch.randint(40, 240, (k,), device=device, generator=g, dtype=torch.int32)
    x = torch.randint(-20, w - 20, (k,), device=device, generator=g, dtype=torch.int32)      # some stick out: clipped
    y = torch.randint(-20, h - 20, (k,), device=device, generator=g, dtype=torch.int32)
    return torch.stack([frame, x, y, bw, bh], 1)


def marks_of(boxes):
    """(K, 5) boxes -> (2K, 8) marks, on the device: every second box pixelated (cells of 16), then every box outlined.
    Marks are applied in row order, so the outlines stay sharp on top of the pixelation."""
    k = boxes.shape[0]
    green = vali.pack_colour(40, 255, 80)
    outline = torch.cat([boxes, torch.tensor([[vali.MARK_BOX, 3, green]], dtype=torch.int32,
                                             device=boxes.device).expand(k, 3)], 1)
    pix = torch.cat([boxes, torch.tensor([[vali.MARK_PIXELATE, 16, 0]], dtype=torch.int32,
                                         device=boxes.device).expand(k, 3)], 1)
    pix[1::2, 5] = vali.MARK_NONE                     # a row of kind 0 is skipped by the kernel
    return torch.cat([pix, outline], 0).contiguous()


def main():
    gpu_id, batch, w, h = 0, 4, 1280, 720
    device = f"cuda:{gpu_id}"
    rng = np.random.default_rng(0)
    up = vali.PyFrameUploader(gpu_id)
    frames = [vali.Surface.Make(vali.PixelFormat.RGB, w, h, gpu_id) for _ in range(batch)]
    for f in frames:
        assert up.Run(rng.integers(0, 256, w * h * 3, dtype=np.uint8), f)[0]

    marks = marks_of(detector(batch, w, h, 6, device))
    torch.cuda.synchronize()                          # the producer has finished before another stream reads the tensor

    ann = vali.PySurfaceAnnotator(gpu_id)
    enc = vali.PyNvJpegEncoder(gpu_id, backend="hip")
    ab = ann.PrepareBatch(frames)                     # prepared once; re-run per batch of detections
    ok, info = ann.RunBatchAsync(ab, marks)           # two launches; the encoder's work queues behind them
    assert ok, info
    files, info = enc.Run(enc.Context(90, vali.PixelFormat.RGB), frames)
    assert info == vali.TaskExecInfo.SUCCESS, info
    for i, f in enumerate(files):
        print(f"frame {i}: {w}x{h} RGB, {marks.shape[0] // batch} marks, {f.size} bytes of JPEG")


if __name__ == "__main__":
    main()
