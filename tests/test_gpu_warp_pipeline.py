"""Selector -> warper on one small batch, with no host read of `dets` in between: a raw face-detector-shaped head
(N, 4 + 1 + 3 P, K) is sliced without a copy into boxes, scores and five landmarks, the selector's dets tensor goes
straight into PySurfaceWarper.PrepareKeypoints, and (N * D, 3, 112, 112) aligned crops come out.  The crops equal the
model (tests/warp_model.py) run on the selector's downloaded dets, and the matrices take the ArcFace template onto the
planted landmarks."""
import numpy as np
import pytest

import detect_model as dm
import warp_model as wm
from test_detect_host import random_head
from test_gpu_annotate import make_frames

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SIZES = [(96, 80), (96, 80), (70, 50)]
N, K, D, P = 3, 65, 4, 5
RECT = (0, 0, 96, 80, 0, 5, 64, 53)            # the letterbox of a 96 x 80 frame in the 64 x 64 network input
NORM = (1.0, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))  # the ArcFace normalisation


def planted(rng):
    """(frame landmarks (N, K, P, 2) float64, the same in network coordinates): the ArcFace template under a random
    similarity into the 96 x 80 frame, taken back through the letterbox"""
    t = np.asarray(wm.ARCFACE_112)
    s, th = rng.uniform(0.15, 0.5, (N, K, 1)), rng.uniform(-0.6, 0.6, (N, K, 1))
    al, be = s * np.cos(th), s * np.sin(th)
    cx, cy = rng.uniform(25, 70, (N, K, 1)), rng.uniform(25, 55, (N, K, 1))
    fx = al * (t[:, 0] - 56) - be * (t[:, 1] - 56) + cx
    fy = be * (t[:, 0] - 56) + al * (t[:, 1] - 56) + cy
    sx, sy, sw, sh, dx, dy, dw, dh = RECT
    net = np.stack([(fx - sx) * dw / sw + dx, (fy - sy) * dh / sh + dy], -1)
    return np.stack([fx, fy], -1), net


@pytest.mark.parametrize("fmt", ["NV12", "RGB"])
def test_selector_warper(vali, gpu, fmt):
    dev = f"cuda:{gpu}"
    boxes, scores, _ = random_head(7, N, K, 1, "xyxy", RECT)
    rects = [RECT, RECT, (0, 0, 70, 50, 0, 9, 0, 46)]              # the last frame has no detections
    frame_pts, net = planted(np.random.default_rng(8))
    kpts = np.zeros((N, K, P, 3), np.float32)
    kpts[..., :2], kpts[..., 2] = net, 0.9
    head = np.concatenate([boxes.transpose(0, 2, 1), scores.transpose(0, 2, 1),
                           kpts.reshape(N, K, 3 * P).transpose(0, 2, 1)], 1)
    pred = torch.from_numpy(np.ascontiguousarray(head)).to(dev)      # (N, 4 + 1 + 3 P, K)
    b, s = pred[:, :4].transpose(1, 2), pred[:, 4:5].transpose(1, 2)
    kt = pred[:, 5:].transpose(1, 2).unflatten(2, (P, 3))
    assert not kt.is_contiguous()
    dets = torch.zeros((N * D, 8), dtype=torch.int32, device=dev)
    mats = torch.zeros((N * D, 8), dtype=torch.int32, device=dev)
    out = torch.full((N * D, 3, 112, 112), -7.0, dtype=torch.float16, device=dev)
    rects_t = torch.tensor(np.asarray(rects, np.int32), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    frames, hosts = make_frames(vali, gpu, fmt, SIZES, seed=23)

    sel, wp = vali.PyDetectionSelector(gpu), vali.PySurfaceWarper(gpu, mean=NORM[1], std=NORM[2], div=NORM[0])
    sb = sel.Prepare(b, s, dets, max_candidates=64, max_det=D)
    wb = wp.PrepareKeypoints(frames, out, kt, dets, max_det=D, template=vali.ARCFACE_112, matrices=mats)
    assert sel.RunAsync(sb, rects_t, 0.5, 0.3) == (True, vali.TaskExecInfo.SUCCESS)
    assert wp.Run(wb, rects_t, kpt_thr=0.5, min_points=5, pad=(0, 0, 0)) == (True, vali.TaskExecInfo.SUCCESS)

    want_d, want_c = dm.select(boxes, scores, np.asarray(rects, np.int32), 0.5, 0.3, False, "xyxy", 64, D)
    assert want_c.tolist()[2] == 0 and want_c[0] >= 2 and want_c[1] >= 2
    torch.cuda.synchronize()
    assert np.array_equal(dets.cpu().numpy(), want_d)
    rows = wm.fit(SIZES, want_d, D, kpts, rects, wm.ARCFACE_112, 0.5, 5)
    used = {i * D + r for i in range(N) for r in range(int(want_c[i]))}
    assert {m for m in range(N * D) if rows[m, 0] >= 0} == used
    assert np.array_equal(mats.cpu().numpy(), rows)
    from vali_amd import tasks

    want, inside = wm.warp(hosts, fmt, SIZES, rows, (112, 112), NORM, (0, 0, 0), tasks.CSC_NPP_709HDTV, "float16")
    got = out.float().cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), np.argwhere(got != want)[:6].tolist()
    assert inside[sorted(used)].mean() > 0.5 and not inside[sorted(set(range(N * D)) - used)].any()
    # the matrices take the template onto the planted landmarks: the bound of tests/test_warp_host.py
    t = np.asarray(wm.ARCFACE_112, np.float32).astype(np.float64)
    co = wm.coeffs_of(rows).astype(np.float64)
    for m in sorted(used):
        a, bb, c, d, e, f = co[m]
        mapped = np.stack([a * t[:, 0] + bb * t[:, 1] + c, d * t[:, 0] + e * t[:, 1] + f], 1)
        assert np.abs(mapped - frame_pts[m // D, int(want_d[m, 7])]).max() <= 2.0 ** -8, m
