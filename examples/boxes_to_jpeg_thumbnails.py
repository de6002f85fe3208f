#!/usr/bin/env python3
"""The objects a detector found in a frame, stored as JPEG thumbnails, in ONE call:

  a JPEG frame -> decoded on the GPU into an RGB surface (PyNvJpegDecoder)
  -> N boxes of N different sizes (made up here; a detector's output in real use)
  -> N 4:2:0 JPEG files at quality 90 (PyNvJpegEncoder.RunRoi).

No crop is copied into a surface of its own and no box costs a launch set of its own: the encoder's kernels start at
the rectangle's origin and replicate at the rectangle's edge, and every file is byte for byte the file of a copy of
the crop.  The route it replaces, one `Run` per copied crop, is run next to it on the first boxes.

    python examples/boxes_to_jpeg_thumbnails.py [out_dir] [frame.jpg]
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import python_vali as vali  # noqa: E402


def main():
    gpu_id = 0
    path = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "tests" / "golden" / "frame_0.jpg"
    dec = vali.PyNvJpegDecoder(gpu_id)
    frames, info = dec.Run([path.read_bytes()], vali.RGB)
    assert info == vali.TaskExecInfo.SUCCESS, info
    frame = frames[0]
    W, H = frame.Width, frame.Height

    # stands in for the detector: 64 boxes between 24 pixels and a third of the frame, anywhere, odd origins included
    rng = np.random.default_rng(0)
    boxes = []
    for _ in range(64):
        w, h = int(rng.integers(24, W // 3)), int(rng.integers(24, H // 3))
        boxes.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))

    enc = vali.PyNvJpegEncoder(gpu_id, backend="hip")
    ctx = enc.Context(90, vali.RGB, subsampling="420")
    files, info = enc.RunRoi(ctx, [frame] * len(boxes), boxes)
    assert info == vali.TaskExecInfo.SUCCESS, info

    # the route it replaces, for the first boxes: download, crop, upload a surface per box, one Run each
    host = np.zeros(frame.HostSize, np.uint8)
    ok, info = vali.PySurfaceDownloader(gpu_id).Run(frame, host)
    assert ok, info
    host = host.reshape(H, W, 3)
    for i, (x, y, w, h) in enumerate(boxes[:4]):
        crop = vali.Surface.Make(vali.RGB, w, h, gpu_id)
        ok, info = vali.PyFrameUploader(gpu_id).Run(np.ascontiguousarray(host[y:y + h, x:x + w]).reshape(-1), crop)
        assert ok, info
        alone, info = enc.Run(ctx, [crop])
        assert info == vali.TaskExecInfo.SUCCESS, info
        same = alone[0].tobytes() == files[i].tobytes()
        print(f"box {i} {boxes[i]}: {files[i].size} bytes, {'the same file as' if same else 'DIFFERS from'} Run on a copy")

    print(f"{len(files)} thumbnails out of one {W} x {H} frame, {sum(f.size for f in files)} bytes in all")
    if len(sys.argv) > 1:
        out = Path(sys.argv[1])
        out.mkdir(parents=True, exist_ok=True)
        for i, f in enumerate(files):
            (out / f"box_{i:02d}.jpg").write_bytes(f.tobytes())
        print(f"written to {out}")


if __name__ == "__main__":
    main()
