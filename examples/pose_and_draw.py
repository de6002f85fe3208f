#!/usr/bin/env python3
"""From a pose network's RAW output to JPEG files with the skeletons drawn on, with no torch glue and no box or keypoint
on the host:

  NV12 frames  --PySurfacePreprocessor.RunTensorBatch (letterbox)-->  (N, 3, 640, 640) float16, and the records it was
                                                                      placed with
  the network  -->  a YOLOv8-pose head (N, 4 + 1 + 3 P, K): cx, cy, w, h, a person score and P keypoints (x, y,
                    confidence) per candidate, P = 17
  the head     --PyDetectionSelector.Run, four launches-->  dets (N * D, 8) in FRAME pixels (their `k` is the candidate's
                                                            index in the head), counts, and marks (N * D, 8) outlines
  dets         --PyPoseDrawer.Run, two launches-->  points (N * D, P, 4): every detection's keypoints in frame pixels with
                                                    their confidence and visibility, for whatever comes next (tracking,
                                                    action recognition); and the COCO skeleton of every detection drawn in
                                                    place onto the NV12 frames
  marks        --PySurfaceAnnotator.RunBatch, two launches-->  the outlines on top
  frames       --PySurfaceConverter, PyNvJpegEncoder(backend="hip")-->  one JPEG file per frame

The head's three parts go in as transposed slices of the network's output, without a copy; nothing between the network
and the encoder reads a detection on the host (the counts and the points are fetched at the end, for the printout).

    python examples/pose_and_draw.py

Runs on synthetic frames and a made-up head."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import python_vali as vali  # noqa: E402

import torch  # noqa: E402

P, K, D = 17, 8400, 20


def network(x):
    """a stand-in for a pose network: a raw YOLOv8-pose head (N, 4 + 1 + 3 P, K), float16, made up on the device --
    clusters of candidates that NMS has to thin out, keypoints scattered over each candidate's box"""
    n, dev = x.shape[0], x.device
    g = torch.Generator(device=dev).manual_seed(0)
    centre = torch.rand((n, 8, 2), device=dev, generator=g) * torch.tensor([480.0, 200.0], device=dev) + \
        torch.tensor([80.0, 220.0], device=dev)
    which = torch.randint(0, 8, (n, K), device=dev, generator=g)
    cxcy = centre.gather(1, which[..., None].expand(-1, -1, 2)) + torch.randn((n, K, 2), device=dev, generator=g) * 3
    wh = torch.tensor([70.0, 140.0], device=dev) + torch.rand((n, K, 2), device=dev, generator=g) * 30
    hot = torch.rand((n, K), device=dev, generator=g) < 0.03
    score = torch.where(hot, 0.4 + 0.5 * torch.rand((n, K), device=dev, generator=g),
                        0.2 * torch.rand((n, K), device=dev, generator=g))[..., None]
    kxy = cxcy[:, :, None, :] + (torch.rand((n, K, P, 2), device=dev, generator=g) - 0.5) * wh[:, :, None, :]
    conf = torch.rand((n, K, P, 1), device=dev, generator=g)
    kpts = torch.cat([kxy, conf], 3).flatten(2)
    return torch.cat([cxcy, wh, score, kpts], 2).transpose(1, 2).contiguous().half()


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
    torch.cuda.synchronize()                                          # the producer has finished before another stream reads

    # head -> detections and outline rows, all on the GPU
    dets = torch.zeros((batch * D, 8), dtype=torch.int32, device=device)
    counts = torch.zeros((batch,), dtype=torch.int32, device=device)
    marks = torch.zeros((batch * D, 8), dtype=torch.int32, device=device)
    points = torch.zeros((batch * D, P, 4), dtype=torch.int32, device=device)
    torch.cuda.synchronize()
    sel = vali.PyDetectionSelector(gpu_id)
    sb = sel.Prepare(pred[:, :4].transpose(1, 2), pred[:, 4:5].transpose(1, 2), dets, counts, marks=marks,
                     box_format="cxcywh", max_candidates=1024, max_det=D)
    style = vali.DetectionStyle(2, [vali.pack_colour(40, 255, 80)])
    ok, info = sel.Run(sb, tb.rects, score_thr=0.25, iou_thr=0.45, style=style)                               # four launches
    assert ok, info

    # dets -> keypoints in frame pixels and skeletons on the frames: the keypoints are the head's last 3 P channels, as
    # they lie
    limb_colours = [vali.pack_colour(255, 120, 0), vali.pack_colour(0, 180, 255), vali.pack_colour(255, 60, 200)]
    joint_colours = [vali.pack_colour(255, 255, 255, 220)]
    pd = vali.PyPoseDrawer(gpu_id)
    pb = pd.Prepare(frames, pred[:, 5:].transpose(1, 2).unflatten(2, (P, 3)), dets, max_det=D, limbs=vali.COCO_SKELETON,
                    points=points)
    ok, info = pd.Run(pb, tb.rects, limb_colours, joint_colours, kpt_thr=0.5, thickness=3, diameter=7, cc_ctx=cc)  # two launches
    assert ok, info

    ann = vali.PySurfaceAnnotator(gpu_id)
    ok, info = ann.RunBatch(ann.PrepareBatch(frames), marks, cc_ctx=cc)                                     # two launches
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
    visible = (points.cpu().numpy()[:, :, 3] != 0).reshape(batch, D, P).sum((1, 2)).tolist()
    for i, f in enumerate(files):
        print(f"frame {i}: {found[i]} detections, {visible[i]} visible keypoints drawn, {f.size} bytes of JPEG")


if __name__ == "__main__":
    main()
