"""Speed of PyInstanceMasker.RunAsync on a YOLOv8-seg-sized batch: 16 x 1080p NV12 frames behind a 640 x 640 letterbox,
prototypes (16, 32, 160, 160) float16, max_det = 100 with 30 detections per frame whose boxes are 40 to 400 pixels a side.

The yardstick is the device part of the torch chain a user writes today, on the same stream in the same process, each run
between two events, the median of the runs after warm-up, the two alternating.  Per frame, with the boxes already on the
host: coeffs[k] @ protos.view(M, -1), the crop of the logits to the letterboxed picture and F.interpolate(...,
mode="bilinear", align_corners=False) to the frame, and per detection the crop to its box, > 0 and the blend on the Y and
UV planes (the chroma mask taken as every second sample: cheaper than the mean the masker forms).  The chain needs some
ten launches per detection and a full-resolution float32 plane for each; RunAsync issues two launches.  So RunAsync may
take at most 1.0 times the chain, with no further margin.
Measured on an MI355X: RunAsync 281.5 us against 57233 us for the chain, ratio 0.005 (profiles/instance_masks.md)."""
import numpy as np
import pytest

import mask_cases as mc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

N, M, HP, WP, K, D, USED = 16, 32, 160, 160, 8400, 100, 30
W, H = 1920, 1080
NET = (640, 640)
LETTERBOX = (0, 0, W, H, 0, 140, 640, 360)
ALPHA = 128


def detections(seed=0):
    """(N * D, 8) rows: USED per frame with even boxes of 40 .. 400 pixels a side inside the frame, the rest unused"""
    rng = np.random.default_rng(seed)
    rows = np.zeros((N * D, 8), np.int32)
    rows[:, 0] = -1
    for i in range(N):
        for r in range(USED):
            w, h = (int(v) & ~1 for v in rng.integers(40, 401, 2))
            x, y = int(rng.integers(0, W - w + 1)) & ~1, int(rng.integers(0, H - h + 1)) & ~1
            rows[i * D + r] = (i, x, y, w, h, int(rng.integers(0, 80)), 0x3F000000, int(rng.integers(0, K)))
    return rows


def _medians(fns, runs=15, warm=3):
    """per-run device time between two events on the current stream, the functions alternating: medians in ms"""
    times = [[] for _ in fns]
    for r in range(warm + runs):
        for j, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warm:
                times[j].append(e0.elapsed_time(e1))
    return [float(np.median(t)) for t in times]


def test_run_is_no_slower_than_the_torch_chain(vali, gpu):
    import torch.nn.functional as F

    torch.cuda.set_device(gpu)
    dev = f"cuda:{gpu}"
    stream = torch.cuda.current_stream(gpu).cuda_stream          # torch's work and ours on one stream
    rng = np.random.default_rng(1)
    protos = torch.from_numpy(mc.protos(M, WP, HP, "float16", n=N, seed=3)).to(dev).to(torch.float16)
    coeffs = torch.from_numpy(rng.standard_normal((N, K, M)).astype(np.float32)).to(dev).to(torch.float16)
    rows = detections()
    dets = torch.from_numpy(rows).to(dev)
    rects = torch.tensor([LETTERBOX] * N, dtype=torch.int32, device=dev)
    palette = [vali.pack_colour(*(int(v) for v in rng.integers(0, 256, 3))) for _ in range(20)]
    colours = torch.tensor(palette, dtype=torch.int32, device=dev)
    frames = [vali.Surface.Make(vali.NV12, W, H, gpu) for _ in range(N)]
    up = vali.PyFrameUploader(gpu)
    noise = rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8)
    for f in frames:
        assert up.Run(noise, f)[0]
    ys = [torch.from_numpy(noise[:W * H].reshape(H, W)).to(dev) for _ in range(N)]
    uvs = [torch.from_numpy(noise[W * H:].reshape(H // 2, W // 2, 2)).to(dev) for _ in range(N)]
    yuv = torch.tensor([[int(v) for v in rng.integers(0, 256, 3)] for _ in palette], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    mk = vali.PyInstanceMasker(gpu, stream)
    mb = mk.Prepare(frames, protos, coeffs, dets, max_det=D, net_size=NET)

    def run():
        assert mk.RunAsync(mb, rects, colours, alpha=ALPHA)[0]

    # the boxes are on the host already: the chain pays for no device-to-host copy
    boxes = [[tuple(int(v) for v in rows[i * D + r]) for r in range(USED)] for i in range(N)]
    ks = [torch.tensor([b[7] for b in boxes[i]], device=dev) for i in range(N)]
    py0, py1 = LETTERBOX[5] * HP // NET[1], (LETTERBOX[5] + LETTERBOX[7]) * HP // NET[1]

    def blend(plane, sel, c):
        v = plane.to(torch.int32)
        return torch.where(sel, (v * (255 - ALPHA) + c * ALPHA + 127) // 255, v).to(torch.uint8)

    def chain():
        for i in range(N):
            L = (coeffs[i, ks[i]].float() @ protos[i].float().view(M, -1)).view(1, USED, HP, WP)
            up_ = F.interpolate(L[:, :, py0:py1], size=(H, W), mode="bilinear", align_corners=False)[0]
            for r, (_, x, y, w, h, cls, _, _) in enumerate(boxes[i]):
                inside = up_[r, y:y + h, x:x + w] > 0
                c = yuv[cls % len(palette)]
                ys[i][y:y + h, x:x + w] = blend(ys[i][y:y + h, x:x + w], inside, c[0])
                uv = uvs[i][y // 2:(y + h) // 2, x // 2:(x + w) // 2]
                uvs[i][y // 2:(y + h) // 2, x // 2:(x + w) // 2] = blend(uv, inside[0::2, 0::2, None], c[1:])

    before = np.zeros(frames[0].HostSize, np.uint8)
    assert vali.PySurfaceDownloader(gpu).Run(frames[0], before)[0]
    run()
    torch.cuda.synchronize()
    after = np.zeros(frames[0].HostSize, np.uint8)
    assert vali.PySurfaceDownloader(gpu).Run(frames[0], after)[0]
    changed = int((before != after).sum())
    area = sum(b[3] * b[4] for b in boxes[0])
    assert 0.05 * area < changed, (changed, area)                # the masks are there
    t_run, t_chain = _medians([run, chain])
    print(f"\ninstance masks {N} x {W}x{H} NV12, prototypes ({N}, {M}, {HP}, {WP}) float16, {USED} detections a frame of "
          f"max_det = {D}: RunAsync {t_run * 1e3:.1f} us (2 launches), torch chain {t_chain * 1e3:.1f} us, "
          f"ratio {t_run / t_chain:.4f}; workspace {mb.ws_bytes / 1e6:.0f} MB")
    assert t_run <= 1.0 * t_chain, f"RunAsync {t_run * 1e3:.1f} us vs the torch chain {t_chain * 1e3:.1f} us"
