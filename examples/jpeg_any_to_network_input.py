#!/usr/bin/env python3
"""JPEG files of ANY sampling and size -> RGB surfaces on the GPU -> letterboxed, normalised network input:

  1. PyNvJpegDecoder decodes a mixed batch (4:4:4, 4:2:0 of odd size, grey, ...) to RGB surfaces -- Pillow's
     convert("RGB") bit for bit, whatever the file's sampling;
  2. PySurfacePreprocessor letterboxes all of them to 299 x 299 RGB_32F_PLANAR in ONE launch.  RGB sources need
     nothing to be even, and there is no colour matrix to choose.

    python examples/jpeg_any_to_network_input.py [file.jpg ...]

Without arguments it encodes a few synthetic pictures with Pillow first."""
import io
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import python_vali as vali  # noqa: E402

SIZE = 299


def synthetic():
    from PIL import Image

    yy, xx = np.mgrid[0:375, 0:501]
    rgb = np.stack([(xx + 40) % 256, (yy + xx // 3) % 256, (2 * yy + 9) % 256], -1).astype(np.uint8)
    files = []
    for img, kw in ((Image.fromarray(rgb), dict(subsampling=0)),                    # 4:4:4, 501 x 375
                    (Image.fromarray(rgb[:251, :333]), dict(subsampling=2)),        # 4:2:0, 333 x 251
                    (Image.fromarray(rgb[:157, :200, 1]), {})):                     # grey, 200 x 157
        out = io.BytesIO()
        img.save(out, "JPEG", quality=90, **kw)
        files.append(out.getvalue())
    return files


def letterbox(src_w, src_h, size):
    """centred, aspect-preserving placement; any integers (vali.letterbox_rect gives the even one NV12 needs)"""
    s = min(size / src_w, size / src_h)
    w, h = min(size, max(1, round(src_w * s))), min(size, max(1, round(src_h * s)))
    return (size - w) // 2, (size - h) // 2, w, h


def main():
    gpu_id = 0
    files = [Path(p).read_bytes() for p in sys.argv[1:]] or synthetic()
    dec = vali.PyNvJpegDecoder(gpu_id)
    frames, status = dec.Run(files, vali.RGB)
    assert status == vali.TaskExecInfo.SUCCESS, dec.last_status

    pre = vali.PySurfacePreprocessor(gpu_id, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), div=255.0)
    net_in = [vali.Surface.Make(vali.PixelFormat.RGB_32F_PLANAR, SIZE, SIZE, gpu_id) for _ in frames]
    places = [letterbox(f.Width, f.Height, SIZE) for f in frames]
    batch = pre.PrepareRoiBatch(frames, net_in, None, places)
    ok, info = pre.RunRoiBatch(batch, pad=(114, 114, 114))
    assert ok, info
    for f, data, p in zip(frames, files, places):
        print(f"{dec.Info(data).sampling:>4} {f.Width} x {f.Height} -> {SIZE} x {SIZE}, placement {p}")


if __name__ == "__main__":
    main()
