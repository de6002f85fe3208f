#!/usr/bin/env python3
"""Closing the loop for video: decoded NV12 frames -> network input -> network output -> NV12 frames, two launches.

  NV12 frames  --PySurfacePreprocessor.RunTensorBatch-->  (N, 3, H, W) float16 in 0..1
               --a stand-in network (a mild sharpen)--->  (N, 3, H, W) float16
               --PySurfacePostprocessor.RunTensorBatch-->  N NV12 surfaces, what PyNvEncoder takes

The way back replaces torch's quantise chain (seven elementwise launches), a permute + contiguous and, per frame,
Surface.from_dlpack + RGB -> YUV420 + YUV420 -> NV12 with ONE launch that reads every element once and writes every
byte of the frames once.  The frames go to PyNvEncoder when PyAV is importable and are downloaded otherwise.

    python examples/tensor_to_video_frames.py

Runs on synthetic frames."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import python_vali as vali  # noqa: E402

import torch  # noqa: E402


def network(x):
    """a stand-in for a restoration network: an unsharp mask, (N, 3, H, W) float16 in, the same out"""
    blur = torch.nn.functional.avg_pool2d(x, 3, stride=1, padding=1)
    return x + 0.5 * (x - blur)


def main():
    gpu_id, batch, w, h = 0, 4, 1280, 720
    rng = np.random.default_rng(0)
    up = vali.PyFrameUploader(gpu_id)
    frames = [vali.Surface.Make(vali.PixelFormat.NV12, w, h, gpu_id) for _ in range(batch)]
    for f in frames:
        assert up.Run(rng.integers(16, 236, w * h * 3 // 2, dtype=np.uint8), f)[0]
    cc = vali.ColorspaceConversionContext(vali.ColorSpace.BT_709, vali.ColorRange.MPEG)      # HD video

    # in: the network's input itself, float16 in 0..1 (div = 255 undoes the 0..255 range)
    pre = vali.PySurfacePreprocessor(gpu_id, div=1.0)
    net_in = torch.empty((batch, 3, h, w), dtype=torch.float16, device=f"cuda:{gpu_id}")
    tb = pre.PrepareTensorBatch(frames, net_in)
    ok, info = pre.RunTensorBatch(tb, cc_ctx=cc)
    assert ok, info

    net_out = network(net_in)
    torch.cuda.synchronize()                       # the producer has finished before another stream reads the tensor

    # out: straight into the frames the encoder takes; scale = 255 is the default for float tensors
    post = vali.PySurfacePostprocessor(gpu_id)
    outs = [vali.Surface.Make(vali.PixelFormat.NV12, w, h, gpu_id) for _ in range(batch)]
    fb = post.PrepareTensorBatch(net_out, outs)    # prepared once; re-run per batch
    ok, info = post.RunTensorBatch(fb, cc_ctx=cc)
    assert ok, info

    try:
        import av  # noqa: F401
        enc = vali.PyNvEncoder({"s": f"{w}x{h}", "codec": "h264", "fps": "30"}, gpu_id, vali.PixelFormat.NV12)
        packet, total = np.ndarray(shape=(0,), dtype=np.uint8), 0
        for s in outs:
            if enc.EncodeSingleSurface(s, packet):
                total += packet.size
        while enc.FlushSinglePacket(packet) and packet.size:
            total += packet.size
        print(f"{batch} frames of {w}x{h} encoded: {total} bytes of h264")
    except (ImportError, RuntimeError):
        dn = vali.PySurfaceDownloader(gpu_id)
        host = np.zeros(outs[0].HostSize, np.uint8)
        for i, s in enumerate(outs):
            assert dn.Run(s, host)[0]
            print(f"frame {i}: {w}x{h} NV12, luma mean {host[:w * h].mean():.1f}, chroma mean {host[w * h:].mean():.1f}")


if __name__ == "__main__":
    main()
