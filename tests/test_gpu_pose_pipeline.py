"""Selector -> pose drawer on one small batch, with no host read of `dets` in between: a raw YOLOv8-pose-shaped head
(N, 4 + 1 + 3 P, K) is sliced without a copy into boxes, scores and keypoints, the selector's dets tensor goes straight
into PyPoseDrawer.Prepare.  The final frames and the points equal the two models chained (tests/detect_model.py,
tests/pose_model.py)."""
import numpy as np
import pytest

import detect_model as dm
import pose_model as po
import postproc_model as pm
from test_detect_host import random_head
from test_gpu_annotate import download, make_frames

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SIZES = [(96, 80), (96, 80), (70, 50)]
N, K, D, P = 3, 65, 4, 5
RECT = (0, 0, 96, 80, 0, 5, 64, 53)            # the letterbox of a 96 x 80 frame in the 64 x 64 network input
LIMBS = ((0, 1), (1, 2), (2, 3), (3, 4), (0, 2))


@pytest.mark.parametrize("fmt", ["NV12", "RGB"])
def test_selector_pose_drawer(vali, gpu, fmt):
    dev = f"cuda:{gpu}"
    boxes, scores, _ = random_head(7, N, K, 1, "xyxy", RECT)
    rects = [RECT, RECT, (0, 0, 70, 50, 0, 9, 0, 46)]              # the last frame has no detections
    rng = np.random.default_rng(6)
    kpts = np.zeros((N, K, P, 3), np.float32)
    kpts[..., 0] = rng.uniform(2, 62, (N, K, P))                    # inside the letterboxed picture
    kpts[..., 1] = rng.uniform(7, 56, (N, K, P))
    kpts[..., 2] = rng.uniform(0.3, 1.0, (N, K, P))
    head = np.concatenate([boxes.transpose(0, 2, 1), scores.transpose(0, 2, 1),
                           kpts.reshape(N, K, 3 * P).transpose(0, 2, 1)], 1)
    pred = torch.from_numpy(np.ascontiguousarray(head)).to(dev)      # (N, 4 + 1 + 3 P, K)
    b, s = pred[:, :4].transpose(1, 2), pred[:, 4:5].transpose(1, 2)
    kt = pred[:, 5:].transpose(1, 2).unflatten(2, (P, 3))
    assert not kt.is_contiguous()
    limb_colours = [vali.pack_colour(40, 255, 80, 220), vali.pack_colour(250, 20, 20, 150)]
    joint_colours = [vali.pack_colour(255, 255, 255)]
    dets = torch.zeros((N * D, 8), dtype=torch.int32, device=dev)
    points = torch.zeros((N * D, P, 4), dtype=torch.int32, device=dev)
    rects_t = torch.tensor(np.asarray(rects, np.int32), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    frames, hosts = make_frames(vali, gpu, fmt, SIZES, seed=22)
    untouched = hosts[2].copy()

    sel, pd = vali.PyDetectionSelector(gpu), vali.PyPoseDrawer(gpu)
    sb = sel.Prepare(b, s, dets, max_candidates=64, max_det=D)
    pb = pd.Prepare(frames, kt, dets, max_det=D, limbs=LIMBS, points=points)
    assert sel.RunAsync(sb, rects_t, 0.5, 0.3) == (True, vali.TaskExecInfo.SUCCESS)
    assert pd.RunAsync(pb, rects_t, limb_colours, joint_colours, kpt_thr=0.5, thickness=2, diameter=5) == \
        (True, vali.TaskExecInfo.SUCCESS)

    want_d, want_c = dm.select(boxes, scores, np.asarray(rects, np.int32), 0.5, 0.3, False, "xyxy", 64, D)
    assert want_c.tolist()[2] == 0 and want_c[0] >= 2 and want_c[1] >= 2
    want_p, drawn = po.apply(hosts, fmt, SIZES, want_d, D, kpts, rects, LIMBS, limb_colours, joint_colours, 0.5, 2, 5, None,
                             pm.matrices()["601_JPEG"])
    assert {d[0] for d in drawn} == {i * D + r for i in range(N) for r in range(int(want_c[i]))}
    assert sum(d[1] < len(LIMBS) and d[3].any() for d in drawn) >= 4          # limbs are drawn, not joints alone
    for i, f in enumerate(frames):
        assert np.array_equal(download(vali, gpu, f), hosts[i]), (fmt, i)
    assert np.array_equal(hosts[2], untouched)
    assert np.array_equal(points.cpu().numpy(), want_p)
    assert np.array_equal(dets.cpu().numpy(), want_d)                      # read only now, after everything ran
