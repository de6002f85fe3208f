#!/usr/bin/env python3
"""Top-down pose, from a detector's RAW output to JPEG files with the skeletons drawn on, with no torch glue between the
stages and no box, crop, heatmap or keypoint on the host:

  NV12 frames  --PySurfacePreprocessor.RunTensorBatch (letterbox)-->  (N, 3, 640, 640) float16, and the records it was
                                                                      placed with
  the detector -->  a raw head (N, 4 + 1, K): cx, cy, w, h and a person score per candidate
  the head     --PyDetectionSelector.Run, four launches-->  dets (N * D, 8) in FRAME pixels, counts, and rois (N * D, 8):
                                                            each detection's box as the source of a 192 x 256 crop
  rois         --PySurfacePreprocessor.RunTensorBatch(rects=rois), one launch-->  (N * D, 3, 256, 192) float16 crops
  the pose net -->  heatmaps (N * D, 17, 64, 48) float16 (HRNet, ViTPose, ...): here Gaussians planted at known positions
  heatmaps     --PyKeypointDecoder.Run, one launch-->  points (N * D, 17, 4) in FRAME pixels through the same rois, with
                                                       their confidence and visibility, and kpts (N * D, 17, 3) as floats
  points       --PyPoseDrawer.RunPoints, two launches-->  the COCO skeleton of every detection on the NV12 frames
  frames       --PySurfaceConverter, PyNvJpegEncoder(backend="hip")-->  one JPEG file per frame

    python examples/topdown_pose.py

Runs on synthetic frames, a made-up detector head and a made-up pose network."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import python_vali as vali  # noqa: E402

import torch  # noqa: E402

P, K, D = 17, 8400, 8
CW, CH, WH, HH = 192, 256, 48, 64


def detector(x):
    """a stand-in for a person detector: a raw head (N, 4 + 1, K), float16, made up on the device -- clusters of
    candidates that NMS has to thin out"""
    n, dev = x.shape[0], x.device
    g = torch.Generator(device=dev).manual_seed(0)
    centre = torch.rand((n, 6, 2), device=dev, generator=g) * torch.tensor([480.0, 200.0], device=dev) + \
        torch.tensor([80.0, 220.0], device=dev)
    which = torch.randint(0, 6, (n, K), device=dev, generator=g)
    cxcy = centre.gather(1, which[..., None].expand(-1, -1, 2)) + torch.randn((n, K, 2), device=dev, generator=g) * 3
    wh = torch.tensor([70.0, 140.0], device=dev) + torch.rand((n, K, 2), device=dev, generator=g) * 30
    hot = torch.rand((n, K), device=dev, generator=g) < 0.03
    score = torch.where(hot, 0.4 + 0.5 * torch.rand((n, K), device=dev, generator=g),
                        0.2 * torch.rand((n, K), device=dev, generator=g))[..., None]
    return torch.cat([cxcy, wh, score], 2).transpose(1, 2).contiguous().half()


def pose_network(crops):
    """a stand-in for a top-down pose network: one Gaussian of sigma 2 cells per keypoint at a made-up position of the
    crop, its height the keypoint's confidence; returns the heatmaps and the positions in heat cells"""
    m, dev = crops.shape[0], crops.device
    g = torch.Generator(device=dev).manual_seed(1)
    centre = torch.rand((m, P, 2), device=dev, generator=g) * torch.tensor([WH - 8.0, HH - 8.0], device=dev) + 4.0
    conf = 0.2 + 0.8 * torch.rand((m, P), device=dev, generator=g)
    x = torch.arange(WH, device=dev) + 0.5
    y = torch.arange(HH, device=dev) + 0.5
    d2 = (x[None, None, None, :] - centre[..., 0, None, None]) ** 2 + (y[None, None, :, None] - centre[..., 1, None, None]) ** 2
    return (conf[..., None, None] * torch.exp(-d2 / 8.0)).half(), centre


def main():
    gpu_id, batch, w, h = 0, 4, 1280, 720
    device = f"cuda:{gpu_id}"
    rng = np.random.default_rng(0)
    up = vali.PyFrameUploader(gpu_id)
    frames = [vali.Surface.Make(vali.PixelFormat.NV12, w, h, gpu_id) for _ in range(batch)]
    for f in frames:
        assert up.Run(rng.integers(0, 256, w * h * 3 // 2, dtype=np.uint8), f)[0]
    cc = vali.ColorspaceConversionContext(vali.ColorSpace.BT_709, vali.ColorRange.MPEG)

    # frames -> detector input, letterboxed; tb.rects are the records the frames were placed with
    pre = vali.PySurfacePreprocessor(gpu_id, div=255.0)
    x = torch.zeros((batch, 3, 640, 640), dtype=torch.float16, device=device)
    torch.cuda.synchronize()
    tb = pre.PrepareTensorBatch(frames, x, None, [vali.letterbox_rect(w, h, 640, 640)] * batch)
    ok, info = pre.RunTensorBatch(tb, pad=(114, 114, 114), cc_ctx=cc)
    assert ok, info

    pred = detector(x)                                                # (N, 4 + 1, K)

    # head -> detections and the rois of their crops, all on the GPU
    dets = torch.zeros((batch * D, 8), dtype=torch.int32, device=device)
    counts = torch.zeros((batch,), dtype=torch.int32, device=device)
    rois = torch.zeros((batch * D, 8), dtype=torch.int32, device=device)
    crops = torch.zeros((batch * D, 3, CH, CW), dtype=torch.float16, device=device)
    points = torch.zeros((batch * D, P, 4), dtype=torch.int32, device=device)
    kpts = torch.zeros((batch * D, P, 3), dtype=torch.float32, device=device)
    torch.cuda.synchronize()                                          # the producer has finished before another stream reads
    sel = vali.PyDetectionSelector(gpu_id)
    sb = sel.Prepare(pred[:, :4].transpose(1, 2), pred[:, 4:5].transpose(1, 2), dets, counts, rois, box_format="cxcywh",
                     max_candidates=1024, max_det=D)
    ok, info = sel.Run(sb, tb.rects, score_thr=0.25, iou_thr=0.45, crop_placement=(0, 0, CW, CH))     # four launches
    assert ok, info

    # rois -> the second stage's input: crop i * D + r comes from frame i
    crop = vali.PySurfacePreprocessor(gpu_id, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), div=255.0)
    cb = crop.PrepareTensorBatch([frames[i] for i in range(batch) for _ in range(D)], crops)
    ok, info = crop.RunTensorBatch(cb, pad=(0, 0, 0), cc_ctx=cc, rects=rois)                          # one launch
    assert ok, info

    heat, centre = pose_network(crops)                                # (N * D, P, 64, 48)
    torch.cuda.synchronize()

    # heatmaps -> points in frame pixels, through the rois the crops were cut with
    dec = vali.PyKeypointDecoder(gpu_id)
    kb = dec.PrepareHeatmaps(frames, heat, points, canvas=(CW, CH), rois=rois, max_det=D, kpts=kpts)
    ok, info = dec.Run(kb, kpt_thr=0.3, refine="quarter", align="centre")                             # one launch
    assert ok, info

    # points -> skeletons on the frames
    limb_colours = [vali.pack_colour(255, 120, 0), vali.pack_colour(0, 180, 255), vali.pack_colour(255, 60, 200)]
    joint_colours = [vali.pack_colour(255, 255, 255, 220)]
    pd = vali.PyPoseDrawer(gpu_id)
    pb = pd.PreparePoints(frames, points, max_det=D, limbs=vali.COCO_SKELETON)
    ok, info = pd.RunPoints(pb, limb_colours, joint_colours, thickness=3, diameter=7, cc_ctx=cc)      # two launches
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

    # for the printout: how far the decoded keypoints are from where the Gaussians were planted, in frame pixels
    found = counts.cpu().tolist()
    r = rois.cpu().numpy().astype(np.float64)
    c = centre.cpu().numpy().astype(np.float64)
    truth = np.stack([r[:, None, 0] + c[..., 0] / WH * r[:, None, 2], r[:, None, 1] + c[..., 1] / HH * r[:, None, 3]], 2)
    got, flags = kpts.cpu().numpy(), points.cpu().numpy()[:, :, 3]
    for i, f in enumerate(files):
        rows = slice(i * D, i * D + found[i])
        err = np.abs(got[rows, :, :2] - truth[rows]).max() if found[i] else 0.0
        print(f"frame {i}: {found[i]} detections, {int((flags[rows] != 0).sum())} visible keypoints drawn, worst distance "
              f"from the planted position {err:.2f} px, {f.size} bytes of JPEG")


if __name__ == "__main__":
    main()
