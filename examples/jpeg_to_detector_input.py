#!/usr/bin/env python3
"""JPEG files -> NV12 surfaces on the GPU -> letterboxed, normalised detector input, without a CPU decode:

  1. PyNvJpegDecoder decodes a batch of 4:2:0 JPEG files straight into NV12 surfaces (the decoded planes as they
     are: no resampling, no colour conversion);
  2. PySurfacePreprocessor letterboxes them to 640 x 640 RGB_32F_PLANAR in one launch.  JPEG's YCbCr is BT.601
     full range (JFIF), hence the colour context.

    python examples/jpeg_to_detector_input.py [file.jpg ...]

Without arguments it first encodes a few synthetic 1080p RGB surfaces on the GPU, 4:2:0
(PyNvJpegEncoder(backend="hip"), Context(..., subsampling="420")): the whole round trip then stays on the device."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import python_vali as vali  # noqa: E402


def synthetic(gpu_id, n=4, w=1920, h=1080):
    yy, xx = np.mgrid[0:h, 0:w]
    surfaces = []
    for i in range(n):
        rgb = np.stack([(xx + 40 * i) % 256, (yy + xx // 3) % 256, (2 * yy + 9 * i) % 256], -1).astype(np.uint8)
        s = vali.Surface.Make(vali.PixelFormat.RGB, w, h, gpu_id)
        ok, info = vali.PyFrameUploader(gpu_id).Run(rgb.reshape(-1), s)
        assert ok, info
        surfaces.append(s)
    enc = vali.PyNvJpegEncoder(gpu_id, backend="hip")
    # 4:2:0, as libjpeg and Pillow write RGB pixels by default: the files PyNvJpegDecoder returns as NV12
    files, status = enc.Run(enc.Context(90, vali.PixelFormat.RGB, subsampling="420"), surfaces)
    assert status == vali.TaskExecInfo.SUCCESS
    return [f.tobytes() for f in files]


def main():
    gpu_id = 0
    files = [Path(p).read_bytes() for p in sys.argv[1:]] or synthetic(gpu_id)
    dec = vali.PyNvJpegDecoder(gpu_id)
    for f in files:
        info = dec.Info(f)                                  # host only: size, sampling, restart interval
        assert info.sampling == "420" and info.width % 2 == 0 and info.height % 2 == 0, info
    frames, status = dec.Run(files, vali.PixelFormat.NV12)
    assert status == vali.TaskExecInfo.SUCCESS, dec.last_status

    pre = vali.PySurfacePreprocessor(gpu_id, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), div=1.0)
    cc = vali.ColorspaceConversionContext(vali.ColorSpace.BT_601, vali.ColorRange.JPEG)
    det_in = [vali.Surface.Make(vali.PixelFormat.RGB_32F_PLANAR, 640, 640, gpu_id) for _ in frames]
    places = [vali.letterbox_rect(f.Width, f.Height, 640, 640) for f in frames]
    batch = pre.PrepareRoiBatch(frames, det_in, None, places)
    ok, info = pre.RunRoiBatch(batch, pad=(114, 114, 114), cc_ctx=cc)
    assert ok, info
    print(f"{len(files)} JPEG files -> NV12 {frames[0].Width}x{frames[0].Height} -> 640 x 640 detector input, "
          f"letterbox {places[0]}")


if __name__ == "__main__":
    main()
