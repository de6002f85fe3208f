"""The top-down chain with no host step between its links: frames -> PyDetectionSelector (`rois`) ->
PySurfacePreprocessor.RunTensorBatch(rects=rois) -> a heatmap "network" that plants Gaussians at known frame positions ->
PyKeypointDecoder (the same `rois`) -> PyPoseDrawer.RunPoints.  The decoded points equal tests/kpt_decode_model.py on the
model's rois and land where the Gaussians were planted; the frames equal pose_model's drawing of those points."""
import numpy as np
import pytest

import detect_model as dm
import kpt_decode_model as kd
import postproc_model as pm
from test_detect_host import random_head
from test_gpu_annotate import download, make_frames

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

W, H = 64, 48
N, K, C, D, P = 3, 65, 4, 4, 5
RECT = (0, 0, W, H, 2, 4, 32, 24)             # the frames went into a 36 x 32 network input at (2, 4), halved
CW, CH, WH, HH = 24, 32, 12, 16               # the crops' canvas and the second stage's heatmaps
LIMBS = ((0, 1), (1, 2), (2, 3), (3, 4))
ROWS_601 = "601_JPEG"


def test_rois_cut_the_crops_and_bring_the_keypoints_back(vali, gpu):
    dev = f"cuda:{gpu}"
    boxes, scores, _ = random_head(5, N, K, C, "xyxy", RECT)
    rects = [RECT, RECT, (0, 0, W, H, 2, 4, 0, 24)]                 # the last frame has no detections
    b, s = torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev)
    dets = torch.zeros((N * D, 8), dtype=torch.int32, device=dev)
    counts = torch.zeros((N,), dtype=torch.int32, device=dev)
    rois = torch.zeros_like(dets)
    torch.cuda.synchronize()
    sel = vali.PyDetectionSelector(gpu)
    sb = sel.Prepare(b, s, dets, counts, rois, max_candidates=64, max_det=D)
    assert sel.Run(sb, rects, 0.5, 0.3, crop_placement=(0, 0, CW, CH)) == (True, vali.TaskExecInfo.SUCCESS)
    want_d, want_c = dm.select(boxes, scores, np.asarray(rects, np.int32), 0.5, 0.3, False, "xyxy", 64, D)
    want_r = dm.rois_of(want_d, (0, 0, CW, CH))
    assert np.array_equal(rois.cpu().numpy(), want_r) and want_c[0] >= 2 and want_c[1] >= 2 and want_c[2] == 0

    # rois -> the crops, item i * D + r from frame i
    frames, hosts = make_frames(vali, gpu, "NV12", [(W, H)] * N, seed=3)
    crops = torch.zeros((N * D, 3, CH, CW), dtype=torch.float16, device=dev)
    torch.cuda.synchronize()
    pre = vali.PySurfacePreprocessor(gpu, div=255.0)
    tb = pre.PrepareTensorBatch([frames[i] for i in range(N) for _ in range(D)], crops)
    assert pre.RunTensorBatch(tb, pad=(0, 0, 0), rects=rois) == (True, vali.TaskExecInfo.SUCCESS)
    used = np.flatnonzero(want_d[:, 0] >= 0)
    assert len({crops[k].cpu().numpy().tobytes() for k in used}) >= 3

    # the "network": Gaussians at known positions of each detection's source rectangle, as heat cells
    rng = np.random.default_rng(4)
    heat = np.zeros((N * D, P, HH, WH), np.float32)
    truth = np.zeros((N * D, P, 2))
    x, y = np.arange(WH) + 0.5, np.arange(HH) + 0.5
    for k in used:
        sx, sy, sw, sh = (int(v) for v in want_r[k, :4])
        for j in range(P):
            hx, hy = rng.uniform(1.6, WH - 1.6), rng.uniform(1.6, HH - 1.6)            # the peak cell off the border
            heat[k, j] = np.exp(-((x[None] - hx) ** 2 + (y[:, None] - hy) ** 2) / 8) * rng.uniform(0.2, 1.0)
            truth[k, j] = sx + hx / WH * sw, sy + hy / HH * sh
    heat = torch.from_numpy(heat).to(torch.float16)
    points = torch.zeros((N * D, P, 4), dtype=torch.int32, device=dev)
    kpts = torch.zeros((N * D, P, 3), dtype=torch.float32, device=dev)
    dec = vali.PyKeypointDecoder(gpu)
    kb = dec.PrepareHeatmaps(frames, heat.to(dev), points, canvas=(CW, CH), rois=rois, max_det=D, kpts=kpts)
    assert dec.Run(kb, kpt_thr=0.3) == (True, vali.TaskExecInfo.SUCCESS)
    want_p, want_k = kd.decode([(W, H)] * N, want_r, D, (CW, CH), heat=heat.float().numpy(), thr=0.3)
    got_p, got_k = points.cpu().numpy(), kpts.cpu().numpy()
    assert np.array_equal(got_p, want_p) and kd.same_floats(got_k, want_k)
    unused = np.setdiff1d(np.arange(N * D), used)
    assert not got_p[unused].any() and (got_p[used][..., 3] != 0).sum() > len(used) * P // 2
    # a quarter of a heat cell, in frame pixels, and float32's rounding at these sizes
    tol = 0.25 * want_r[used, 2:4][:, None, :] / np.asarray([WH, HH]) + 2.0 ** -6
    assert (abs(got_k[used][..., :2] - truth[used]) <= tol).all()

    # the points -> skeletons on the frames
    lcol, jcol = [vali.pack_colour(230, 40, 40, 200), vali.pack_colour(40, 200, 60)], [vali.pack_colour(255, 255, 255, 230)]
    pd = vali.PyPoseDrawer(gpu)
    pb = pd.PreparePoints(frames, points, max_det=D, limbs=LIMBS)
    assert pd.RunPoints(pb, lcol, jcol, thickness=2, diameter=5, cc_ctx=pm.cc_ctx_of(vali, ROWS_601)) == \
        (True, vali.TaskExecInfo.SUCCESS)
    before = [h.copy() for h in hosts]
    assert kd.paint_points(hosts, "NV12", [(W, H)] * N, want_p, D, LIMBS, lcol, jcol, 2, 5, None, pm.matrices()[ROWS_601]) > 10
    for i in range(N):
        assert np.array_equal(download(vali, gpu, frames[i]), hosts[i]), i
        assert np.array_equal(hosts[i], before[i]) == (i == 2), i
