#!/usr/bin/env python3
"""NV12 frames straight into the tensor a half-precision detector takes, in ONE launch:

  a batch of 1080p frames -> letterboxed 640 x 640 (a 640 x 360 picture at y = 140, the bands 114, 114, 114),
  normalised, float16, channels last, written into one (N, 3, 640, 640) torch tensor.

No destination surfaces, no torch.stack, no .half(): the kernel converts its 3 x 256 normalisation table once per
workgroup and stores finished 16-bit elements, 2 bytes per element instead of the 4 + (4 + 4) + (4 + 2) of the
surface -> stack -> cast route.

    python examples/fp16_batch_for_inference.py

Runs on synthetic frames."""
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

    # the network's input itself: allocated once, in the dtype and memory format the network runs in
    net_in = torch.empty((batch, 3, 640, 640), dtype=torch.float16, device=f"cuda:{gpu_id}")
    net_in = net_in.contiguous(memory_format=torch.channels_last)
    place = vali.letterbox_rect(w, h, 640, 640)                      # (0, 140, 640, 360)
    # prepared once (descriptors and rectangles are uploaded here); re-run per batch of decoded frames
    tb = pre.PrepareTensorBatch(frames, net_in, None, [place] * batch)
    ok, info = pre.RunTensorBatch(tb, pad=(114, 114, 114), cc_ctx=cc)
    assert ok, info
    print("network input:", tuple(net_in.shape), net_in.dtype,
          "channels last" if net_in.is_contiguous(memory_format=torch.channels_last) else "planar", "letterbox", place)
    band, picture = net_in[:, :, :140], net_in[:, :, 140:500]
    print("band value %.4f (114 / 255 = %.4f), picture mean %.4f" % (band.float().mean().item(), 114 / 255,
                                                                    picture.float().mean().item()))


if __name__ == "__main__":
    main()
