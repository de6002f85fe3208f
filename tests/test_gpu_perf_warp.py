"""Speed of PySurfaceWarper.RunAsync, form (b), on a face-recognition-sized batch: 16 x 1080p NV12 frames behind a 640 x 640
letterbox, max_det = 32 with 20 detections per frame whose boxes are 60 to 300 pixels a side, five landmarks planted inside
each box, the ArcFace template, out float16 (512, 3, 112, 112) planar.

The yardstick is what a user writes today, on the same stream in the same process, each run between two events, the median
of the runs after warm-up, the two alternating: one PySurfacePreprocessor.RunTensorBatch of the 16 frames to a same-size
float16 tensor (timed: the warper reads NV12 directly), then per frame F.affine_grid + F.grid_sample over
rgb[i:i+1].expand(m_i, -1, -1, -1), with the thetas precomputed on the GPU outside the timing.  RunAsync may take at most
1.0 times that chain, with no further margin: the task has to be no slower than the torch road it replaces.
Measured on an MI355X: RunAsync 82.5 us against 1150.8 us for the road, ratio 0.072 (profiles/aligned_crops.md)."""
import numpy as np
import pytest

import warp_model as wm
from test_gpu_perf_masks import _medians

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

N, D, USED, K, P = 16, 32, 20, 1024, 5
W, H = 1920, 1080
LETTERBOX = (0, 0, W, H, 0, 140, 640, 360)
CANVAS = (112, 112)
NORM = (1.0, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))


def faces(seed=0):
    """(dets (N * D, 8) int32, kpts (N, K, P, 3) float32): USED rows per frame with boxes of 60 .. 300 pixels a side inside
    the frame, the rest unused; candidate k of a row holds the ArcFace template under a similarity that fills 80 % of the
    box, turned by up to +-0.5 rad, taken back through the letterbox"""
    rng = np.random.default_rng(seed)
    t = np.asarray(wm.ARCFACE_112)
    rows = np.zeros((N * D, 8), np.int32)
    rows[:, 0] = -1
    kpts = np.zeros((N, K, P, 3), np.float32)
    kpts[..., 2] = 0.9
    sx, sy, sw, sh, dx, dy, dw, dh = LETTERBOX
    for i in range(N):
        ks = rng.permutation(K)[:USED]
        for r in range(USED):
            side = int(rng.integers(60, 301))
            x, y = int(rng.integers(0, W - side + 1)), int(rng.integers(0, H - side + 1))
            rows[i * D + r] = (i, x, y, side, side, 0, 0x3F000000, int(ks[r]))
            s, th = 0.8 * side / 112.0, rng.uniform(-0.5, 0.5)
            al, be = s * np.cos(th), s * np.sin(th)
            fx = al * (t[:, 0] - 56) - be * (t[:, 1] - 56) + x + side / 2
            fy = be * (t[:, 0] - 56) + al * (t[:, 1] - 56) + y + side / 2
            kpts[i, ks[r], :, 0] = (fx - sx) * dw / sw + dx
            kpts[i, ks[r], :, 1] = (fy - sy) * dh / sh + dy
    return rows, kpts


def test_run_is_no_slower_than_the_torch_road(vali, gpu):
    import torch.nn.functional as F
    from vali_amd import tasks

    torch.cuda.set_device(gpu)
    dev = f"cuda:{gpu}"
    stream = torch.cuda.current_stream(gpu).cuda_stream          # torch's work and ours on one stream
    rng = np.random.default_rng(1)
    rows, kp = faces()
    dets = torch.from_numpy(rows).to(dev)
    kt = torch.from_numpy(kp).to(dev)
    rects = torch.tensor([LETTERBOX] * N, dtype=torch.int32, device=dev)
    frames = [vali.Surface.Make(vali.NV12, W, H, gpu) for _ in range(N)]
    up = vali.PyFrameUploader(gpu)
    noise = rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8)
    for f in frames:
        assert up.Run(noise, f)[0]
    out = torch.full((N * D, 3, CANVAS[1], CANVAS[0]), -7.0, dtype=torch.float16, device=dev)
    mats = torch.zeros((N * D, 8), dtype=torch.int32, device=dev)
    rgb = torch.zeros((N, 3, H, W), dtype=torch.float16, device=dev)
    torch.cuda.synchronize()

    wp = vali.PySurfaceWarper(gpu, stream, mean=NORM[1], std=NORM[2], div=NORM[0])
    pp = vali.PySurfacePreprocessor(gpu, stream, mean=NORM[1], std=NORM[2], div=NORM[0])
    wb = wp.PrepareKeypoints(frames, out, kt, dets, max_det=D, template=vali.ARCFACE_112, matrices=mats)
    wm_only = wp.PrepareMatrices(frames, out, mats)
    tb = pp.PrepareTensorBatch(frames, rgb)

    def run():
        assert wp.RunAsync(wb, rects, kpt_thr=0.5, min_points=5, pad=(0, 0, 0))[0]

    def sample_only():
        assert wp.RunAsync(wm_only, pad=(0, 0, 0))[0]

    # before timing: the crops are the model's for one slot, and the used slots are not all pad
    run()
    torch.cuda.synchronize()
    got_rows = mats.cpu().numpy()
    want_rows = wm.fit([(W, H)] * N, rows, D, kp, [LETTERBOX] * N, wm.ARCFACE_112, 0.5, 5)
    assert np.array_equal(got_rows, want_rows) and (want_rows[:, 0] >= 0).sum() == N * USED
    slot = 3 * D + 7
    want, inside = wm.warp([noise] * N, "NV12", [(W, H)] * N, want_rows[slot:slot + 1], CANVAS, NORM, (0, 0, 0),
                           tasks.CSC_NPP_709HDTV, "float16")
    got = out[slot:slot + 1].float().cpu().numpy()
    assert inside.all() and np.array_equal(got.view(np.int32), want.view(np.int32))
    padv = out[D - 1, :, 0, 0].float().cpu().numpy()                 # an unused slot: all pad
    used = torch.tensor(np.flatnonzero(want_rows[:, 0] >= 0), device=dev)
    assert all(bool((out[used, c] != float(padv[c])).any(dim=2).any(dim=1).all()) for c in range(3))

    # the thetas of affine_grid from the warper's own matrices, on the GPU: with u = (xn + 1) w / 2 and gx = 2 sx / W - 1
    co = mats[:, 1:7].view(torch.float32)
    w, h = CANVAS
    theta = torch.stack([co[:, 0] * w / W, co[:, 1] * h / W, (co[:, 0] * w + co[:, 1] * h + 2 * co[:, 2]) / W - 1,
                         co[:, 3] * w / H, co[:, 4] * h / H, (co[:, 3] * w + co[:, 4] * h + 2 * co[:, 5]) / H - 1],
                        1).view(-1, 2, 3).to(torch.float16)
    thetas = [theta[i * D:i * D + USED].contiguous() for i in range(N)]
    crops = [None] * N
    torch.cuda.synchronize()

    def chain():
        assert pp.RunTensorBatchAsync(tb)[0]
        for i in range(N):
            grid = F.affine_grid(thetas[i], (USED, 3, h, w), align_corners=False)
            crops[i] = F.grid_sample(rgb[i:i + 1].expand(USED, -1, -1, -1), grid, mode="bilinear", padding_mode="zeros",
                                     align_corners=False)

    t_run, t_chain, t_sample = _medians([run, chain, sample_only])
    nbytes = N * D * 3 * h * w * 2
    print(f"\naligned crops {N} x {W}x{H} NV12, {USED} of max_det = {D} detections a frame, ({N * D}, 3, {h}, {w}) float16: "
          f"RunAsync {t_run * 1e3:.1f} us (2 launches), of which the sampler alone {t_sample * 1e3:.1f} us = "
          f"{nbytes / (t_sample * 1e-3) / 8e12 * 100:.1f} % of 8 TB/s over the {nbytes / 1e6:.1f} MB written; "
          f"torch road {t_chain * 1e3:.1f} us, ratio {t_run / t_chain:.4f}")
    assert t_run <= 1.0 * t_chain, f"RunAsync {t_run * 1e3:.1f} us vs the torch road {t_chain * 1e3:.1f} us"
