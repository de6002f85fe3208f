"""Speed of PyPoseDrawer.RunAsync on a YOLOv8-pose-sized batch: 16 x 1080p NV12 frames behind a 640 x 640 letterbox,
keypoints (16, 8400, 17, 3) float16, COCO_SKELETON, max_det = 100 with 30 detections per frame whose boxes are 40 to 400
pixels a side and whose keypoints lie inside their box; thickness 3, diameter 7.

The yardstick is PyInstanceMasker.RunAsync on the same frames, dets and rects (the batch of tests/test_gpu_perf_masks.py),
on the same stream in the same process, each run between two events, the median of the runs after warm-up, the two
alternating.  The drawer reads no prototypes and covers fewer pixels, so it may take at most 1.25 times the masker's time:
the margin this project's ratio guards give for drift between processes on one box.
Measured on an MI355X: RunAsync 235.1 us against 234.1 us for the masker, ratio 1.004 (profiles/pose.md)."""
import numpy as np
import pytest

import mask_cases as mc
from test_gpu_perf_masks import ALPHA, D, HP, K, LETTERBOX, M, N, NET, USED, W, WP, H, _medians, detections

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

P = 17


def keypoints(rows, seed=2):
    """(N, K, P, 3) float32 in network coordinates: the P keypoints of each used row's candidate at random pixels of its
    box, confidences 0.3 .. 1 (about a quarter below the threshold of 0.5); other candidates far outside"""
    rng = np.random.default_rng(seed)
    kpts = np.full((N, K, P, 3), -1e4, np.float32)
    sx, sy, sw, sh, dx, dy, dw, dh = LETTERBOX
    for i in range(N):
        for r in range(USED):
            _, x, y, w, h, _, _, k = (int(v) for v in rows[i * D + r])
            px, py = rng.uniform(x, x + w, P), rng.uniform(y, y + h, P)
            kpts[i, k, :, 0] = (px - sx) * dw / sw + dx
            kpts[i, k, :, 1] = (py - sy) * dh / sh + dy
            kpts[i, k, :, 2] = rng.uniform(0.3, 1.0, P)
    return kpts


def test_run_takes_at_most_1_25_times_the_maskers(vali, gpu):
    torch.cuda.set_device(gpu)
    dev = f"cuda:{gpu}"
    stream = torch.cuda.current_stream(gpu).cuda_stream
    rng = np.random.default_rng(1)
    rows = detections()
    dets = torch.from_numpy(rows).to(dev)
    rects = torch.tensor([LETTERBOX] * N, dtype=torch.int32, device=dev)
    palette = [vali.pack_colour(*(int(v) for v in rng.integers(0, 256, 3))) for _ in range(20)]
    colours = torch.tensor(palette, dtype=torch.int32, device=dev)
    protos = torch.from_numpy(mc.protos(M, WP, HP, "float16", n=N, seed=3)).to(dev).to(torch.float16)
    coeffs = torch.from_numpy(rng.standard_normal((N, K, M)).astype(np.float32)).to(dev).to(torch.float16)
    kpts = torch.from_numpy(keypoints(rows)).to(dev).to(torch.float16)
    points = torch.zeros((N * D, P, 4), dtype=torch.int32, device=dev)
    frames = [vali.Surface.Make(vali.NV12, W, H, gpu) for _ in range(N)]
    up = vali.PyFrameUploader(gpu)
    noise = rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8)
    for f in frames:
        assert up.Run(noise, f)[0]
    torch.cuda.synchronize()

    mk, pd = vali.PyInstanceMasker(gpu, stream), vali.PyPoseDrawer(gpu, stream)
    mb = mk.Prepare(frames, protos, coeffs, dets, max_det=D, net_size=NET)
    pb = pd.Prepare(frames, kpts, dets, max_det=D, limbs=vali.COCO_SKELETON, points=points)

    def mask():
        assert mk.RunAsync(mb, rects, colours, alpha=ALPHA)[0]

    def pose():
        assert pd.RunAsync(pb, rects, colours, colours, kpt_thr=0.5, thickness=3, diameter=7, alpha=ALPHA)[0]

    before = np.zeros(frames[0].HostSize, np.uint8)
    assert vali.PySurfaceDownloader(gpu).Run(frames[0], before)[0]
    pose()
    torch.cuda.synchronize()
    after = np.zeros(frames[0].HostSize, np.uint8)
    assert vali.PySurfaceDownloader(gpu).Run(frames[0], after)[0]
    pts = points.cpu().numpy()
    visible = int((pts[:D * 1, :, 3] != 0).sum())
    assert 0.5 * USED * P < visible < USED * P, visible                  # about three quarters of frame 0's keypoints
    changed = int((before != after).sum())
    assert changed > 7 * 7 // 2 * visible // 2, (changed, visible)       # the skeletons are there
    t_pose, t_mask = _medians([pose, mask])
    print(f"\npose skeletons {N} x {W}x{H} NV12, keypoints ({N}, {K}, {P}, 3) float16, {USED} detections a frame of "
          f"max_det = {D}, 19 limbs: RunAsync {t_pose * 1e3:.1f} us (2 launches), PyInstanceMasker.RunAsync "
          f"{t_mask * 1e3:.1f} us, ratio {t_pose / t_mask:.3f}; {changed} bytes of frame 0 changed")
    assert t_pose <= 1.25 * t_mask, f"RunAsync {t_pose * 1e3:.1f} us vs the masker's {t_mask * 1e3:.1f} us"
