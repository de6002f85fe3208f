#!/usr/bin/env python3
"""Detection and second-stage classification inputs from NV12 frames, without leaving the library:

  1. letterbox: a batch of 1080p frames -> 640 x 640 with the aspect ratio kept (a 640 x 360 picture at y = 140,
     the bands filled with 114, 114, 114), normalised, in ONE launch;
  2. crops: 16 boxes held in a GPU tensor (where a detector leaves them) -> a 224 x 224 batch, ONE launch, no
     device-to-host synchronisation for the boxes.

    python examples/letterbox_for_detection.py

Runs on synthetic frames; the boxes stand in for a detector's output."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import python_vali as vali  # noqa: E402

import torch  # noqa: E402


def main():
    gpu_id, batch, w, h = 0, 8, 1920, 1080
    rng = np.random.default_rng(0)
    up = vali.PyFrameUploader(gpu_id)
    frames = [vali.Surface.Make(vali.PixelFormat.NV12, w, h, gpu_id) for _ in range(batch)]
    for f in frames:
        assert up.Run(rng.integers(16, 236, w * h * 3 // 2, dtype=np.uint8), f)[0]
    pre = vali.PySurfacePreprocessor(gpu_id, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), div=1.0)
    cc = vali.ColorspaceConversionContext(vali.ColorSpace.BT_709, vali.ColorRange.MPEG)

    # 1. letterbox the whole batch (the arrays are uploaded once; keep `lb` and re-run it per batch of frames)
    place = vali.letterbox_rect(w, h, 640, 640)                      # (0, 140, 640, 360)
    det_in = [vali.Surface.Make(vali.PixelFormat.RGB_32F_PLANAR, 640, 640, gpu_id) for _ in frames]
    lb = pre.PrepareRoiBatch(frames, det_in, None, [place] * batch)
    ok, info = pre.RunRoiBatch(lb, pad=(114, 114, 114), cc_ctx=cc)
    assert ok, info
    det = torch.stack([torch.from_dlpack(s).view(3, 640, 640) for s in det_in])
    print("detector input:", tuple(det.shape), "letterbox", place)

    # 2. 16 boxes of frame 0 as a device int32 tensor (x, y, w, h of the crop; x, y, w, h in the 224 x 224 slot).
    #    The kernel clamps every box to its frame, so raw detector boxes (rounded to integers) are safe to pass.
    n = 16
    xy = torch.randint(0, 1600, (n, 2), device="cuda", dtype=torch.int32)
    wh = torch.randint(32, 320, (n, 2), device="cuda", dtype=torch.int32)
    slot = torch.tensor([0, 0, 224, 224], device="cuda", dtype=torch.int32).expand(n, 4)
    boxes = torch.cat([xy, wh, slot], dim=1).contiguous()
    torch.cuda.synchronize()                                         # the boxes are ready before the task's stream reads them
    crops_out = [vali.Surface.Make(vali.PixelFormat.RGB_32F_PLANAR, 224, 224, gpu_id) for _ in range(n)]
    cb = pre.PrepareRoiBatch([frames[0]] * n, crops_out)             # prepared once; the rectangles come per call
    ok, info = pre.RunRoiBatch(cb, pad=(0, 0, 0), cc_ctx=cc, rects=boxes)
    assert ok, info
    crops = torch.stack([torch.from_dlpack(s).view(3, 224, 224) for s in crops_out])
    print("classifier input:", tuple(crops.shape), "mean %.4f" % crops.mean().item())


if __name__ == "__main__":
    main()
