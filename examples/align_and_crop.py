#!/usr/bin/env python3
"""From a face detector's RAW output to aligned network inputs, and from rotated boxes to upright crops, with no torch
glue per frame and no box, landmark or matrix on the host:

  NV12 frames  --PySurfacePreprocessor.RunTensorBatch (letterbox)-->  (N, 3, 640, 640) float16, and the records it was
                                                                      placed with
  the network  -->  a detector head with landmarks (N, 4 + 1 + 3 P, K): cx, cy, w, h, a face score and P = 5 landmarks
                    (x, y, confidence) per candidate
  the head     --PyDetectionSelector.Run, four launches-->  dets (N * D, 8) in FRAME pixels (their `k` is the candidate's
                                                            index in the head) and counts
  dets         --PySurfaceWarper.Run, two launches-->  (N * D, 3, 112, 112) float16: every detection's face under the
                                                       similarity that takes the five ArcFace points onto its landmarks,
                                                       sampled from the NV12 frames themselves and normalised for the
                                                       embedder; slots without a detection are pad; and the matrices
  rotated boxes (cx, cy, w, h, theta)  --a few torch operations, then PySurfaceWarper.Run, one launch-->  upright crops

    python examples/align_and_crop.py

Runs on synthetic frames and a made-up head."""
import math
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import python_vali as vali  # noqa: E402

import torch  # noqa: E402

P, K, D = 5, 8400, 8


def network(x):
    """a stand-in for a face detector: a raw head (N, 4 + 1 + 3 P, K), float16, made up on the device -- clusters of
    candidates that NMS has to thin out, each with the five ArcFace points turned and scaled into its box"""
    n, dev = x.shape[0], x.device
    g = torch.Generator(device=dev).manual_seed(0)
    centre = torch.rand((n, 6, 2), device=dev, generator=g) * torch.tensor([480.0, 200.0], device=dev) + \
        torch.tensor([80.0, 220.0], device=dev)
    which = torch.randint(0, 6, (n, K), device=dev, generator=g)
    cxcy = centre.gather(1, which[..., None].expand(-1, -1, 2)) + torch.randn((n, K, 2), device=dev, generator=g) * 2
    side = 50.0 + 5.0 * which[..., None].float()
    wh = torch.cat([side, side * 1.2], 2)
    hot = torch.rand((n, K), device=dev, generator=g) < 0.03
    score = torch.where(hot, 0.4 + 0.5 * torch.rand((n, K), device=dev, generator=g),
                        0.2 * torch.rand((n, K), device=dev, generator=g))[..., None]
    t = torch.tensor(vali.ARCFACE_112, device=dev) - 56.0                       # (5, 2) around the canvas centre
    th = (which.float() - 2.5) * 0.2                                              # every cluster has its own tilt
    s = (side / 112.0)[..., None]
    cos, sin = torch.cos(th)[..., None], torch.sin(th)[..., None]
    kx = cxcy[..., :1] + s[..., 0] * (cos * t[:, 0] - sin * t[:, 1])
    ky = cxcy[..., 1:] + s[..., 0] * (sin * t[:, 0] + cos * t[:, 1])
    kpts = torch.stack([kx, ky, torch.full_like(kx, 0.9)], 3).flatten(2)
    return torch.cat([cxcy, wh, score, kpts], 2).transpose(1, 2).contiguous().half()


def rotated_box_matrices(boxes, frame_of, out_w, out_h):
    """(M, 8) int32 rows for PrepareMatrices from rotated boxes (cx, cy, w, h, theta) in frame pixels, on the device: canvas
    position (u, v) samples the frame at centre + R(theta) ((u / out_w - 0.5) w, (v / out_h - 0.5) h)"""
    cx, cy, w, h, th = boxes.unbind(1)
    cos, sin = torch.cos(th), torch.sin(th)
    a, b = cos * w / out_w, -sin * h / out_h
    d, e = sin * w / out_w, cos * h / out_h
    c = cx - 0.5 * (cos * w - sin * h)
    f = cy - 0.5 * (sin * w + cos * h)
    co = torch.stack([a, b, c, d, e, f], 1).float().contiguous()
    rows = torch.zeros((len(boxes), 8), dtype=torch.int32, device=boxes.device)
    rows[:, 0] = frame_of
    rows[:, 1:7] = co.view(torch.int32)
    return rows


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

    pred = network(x)                                                 # (N, 4 + 1 + 3 P, K)

    # head -> detections, all on the GPU
    dets = torch.zeros((batch * D, 8), dtype=torch.int32, device=device)
    counts = torch.zeros((batch,), dtype=torch.int32, device=device)
    faces = torch.zeros((batch * D, 3, 112, 112), dtype=torch.float16, device=device)
    matrices = torch.zeros((batch * D, 8), dtype=torch.int32, device=device)
    torch.cuda.synchronize()                                          # the producer has finished before another stream reads
    sel = vali.PyDetectionSelector(gpu_id)
    sb = sel.Prepare(pred[:, :4].transpose(1, 2), pred[:, 4:5].transpose(1, 2), dets, counts, box_format="cxcywh",
                     max_candidates=1024, max_det=D)
    ok, info = sel.Run(sb, tb.rects, score_thr=0.25, iou_thr=0.45)                                   # four launches
    assert ok, info

    # dets + landmarks -> aligned faces, normalised as ArcFace embedders expect: (x / 255 - 0.5) / 0.5
    wp = vali.PySurfaceWarper(gpu_id, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5))
    wb = wp.PrepareKeypoints(frames, faces, pred[:, 5:].transpose(1, 2).unflatten(2, (P, 3)), dets, max_det=D,
                             template=vali.ARCFACE_112, matrices=matrices)
    ok, info = wp.Run(wb, tb.rects, kpt_thr=0.5, min_points=3, pad=(0, 0, 0), cc_ctx=cc)              # two launches
    assert ok, info

    # rotated boxes -> upright 96 x 32 crops (plates, text lines), the matrices built by a few torch operations
    g = torch.Generator(device=device).manual_seed(1)
    m = 12
    boxes = torch.stack([200 + 800 * torch.rand(m, device=device, generator=g), 150 + 400 * torch.rand(m, device=device, generator=g),
                         120 + 80 * torch.rand(m, device=device, generator=g), 40 + 20 * torch.rand(m, device=device, generator=g),
                         (torch.rand(m, device=device, generator=g) - 0.5) * math.pi / 2], 1)
    frame_of = torch.arange(m, device=device, dtype=torch.int32) % batch
    rows = rotated_box_matrices(boxes, frame_of, 96, 32)
    plates = torch.zeros((m, 3, 32, 96), dtype=torch.float16, device=device).contiguous(memory_format=torch.channels_last)
    torch.cuda.synchronize()
    plain = vali.PySurfaceWarper(gpu_id, div=255.0)
    ok, info = plain.Run(plain.PrepareMatrices(frames, plates, rows), pad=(0, 0, 0), cc_ctx=cc)       # one launch
    assert ok, info

    found = counts.cpu().tolist()
    rows_h = matrices.cpu().numpy()
    co = np.ascontiguousarray(rows_h[:, 1:7]).view(np.float32)
    for i in range(batch):
        mine = rows_h[i * D:(i + 1) * D]
        scales = [float(np.hypot(*co[i * D + r, [0, 3]])) for r in range(D) if mine[r, 0] >= 0]
        print(f"frame {i}: {found[i]} detections, {len(scales)} aligned faces, frame pixels per canvas pixel "
              f"{min(scales, default=0):.2f} .. {max(scales, default=0):.2f}")
    print(f"faces {tuple(faces.shape)} {faces.dtype}, mean {faces.float().mean().item():+.3f}; "
          f"plates {tuple(plates.shape)} channels last, mean {plates.float().mean().item():.3f}")


if __name__ == "__main__":
    main()
