"""Speed of PySemanticPainter.RunAsync on a segmentation-sized batch: 16 x 1080p NV12 frames behind a 512 x 512 letterbox,
logits (16, 19, 128, 128) float16, a 19-colour palette at alpha 128, label surfaces on.

The yardstick is the device part of the torch chain a user writes today, on the same stream in the same process, each run
between two events, the median of 15 runs after 3 warm-ups, the two alternating.  Per frame: the crop of the logits to the
letterboxed rows, F.interpolate(..., mode="bilinear", align_corners=False) to the frame, argmax over the classes, the
palette gather, and the blend on the Y plane and, with every second label (cheaper than the mean the painter forms), on
the UV plane.  The chain moves more than ten times the bytes through about ten launches a frame; RunAsync issues one
launch.  So RunAsync may take at most 1.0 times the chain, with no further margin.
Measured on an MI355X: RunAsync 373.0 us against 2603.9 us for the chain, ratio 0.143 (profiles/semantic.md)."""
import numpy as np
import pytest

import semantic_cases as sc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

N, C, HS, WS = 16, 19, 128, 128
W, H = 1920, 1080
NET = (512, 512)
LETTERBOX = (0, 0, W, H, 0, 112, 512, 288)
ALPHA = 128


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
    logits = torch.from_numpy(sc.logits(C, WS, HS, "float16", n=N, seed=4)).to(dev).to(torch.float16)
    rects = torch.tensor([LETTERBOX] * N, dtype=torch.int32, device=dev)
    palette = [vali.pack_colour(*(int(v) for v in rng.integers(0, 256, 3))) for _ in range(C)]
    colours = torch.tensor(palette, dtype=torch.int32, device=dev)
    frames = [vali.Surface.Make(vali.NV12, W, H, gpu) for _ in range(N)]
    labels = [vali.Surface.Make(vali.Y, W, H, gpu) for _ in range(N)]
    up = vali.PyFrameUploader(gpu)
    noise = rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8)
    for f in frames:
        assert up.Run(noise, f)[0]
    ys = [torch.from_numpy(noise[:W * H].reshape(H, W)).to(dev) for _ in range(N)]
    uvs = [torch.from_numpy(noise[W * H:].reshape(H // 2, W // 2, 2)).to(dev) for _ in range(N)]
    yuv = torch.tensor([[int(v) for v in rng.integers(0, 256, 3)] for _ in palette], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    sp = vali.PySemanticPainter(gpu, stream)
    sb = sp.Prepare(frames, logits, labels, net_size=NET)

    def run():
        assert sp.RunAsync(sb, rects, colours, alpha=ALPHA)[0]

    py0, py1 = LETTERBOX[5] * HS // NET[1], (LETTERBOX[5] + LETTERBOX[7]) * HS // NET[1]

    def blend(plane, c):
        return ((plane.to(torch.int32) * (255 - ALPHA) + c * ALPHA + 127) // 255).to(torch.uint8)

    def chain():
        for i in range(N):
            up_ = F.interpolate(logits[i:i + 1, :, py0:py1], size=(H, W), mode="bilinear", align_corners=False)[0]
            lab = up_.argmax(0)
            col = yuv[lab]
            ys[i].copy_(blend(ys[i], col[:, :, 0]))
            uvs[i].copy_(blend(uvs[i], col[0::2, 0::2, 1:]))

    before = np.zeros(frames[0].HostSize, np.uint8)
    assert vali.PySurfaceDownloader(gpu).Run(frames[0], before)[0]
    run()
    torch.cuda.synchronize()
    after = np.zeros(frames[0].HostSize, np.uint8)
    assert vali.PySurfaceDownloader(gpu).Run(frames[0], after)[0]
    lab0 = np.zeros(W * H, np.uint8)
    assert vali.PySurfaceDownloader(gpu).Run(labels[0], lab0)[0]
    changed = (before != after).mean()
    assert changed > 0.5, changed                                 # the whole frame is the region and is tinted
    assert lab0.max() < C and len(np.unique(lab0)) >= 5           # ... with several classes
    t_run, t_chain = _medians([run, chain])
    moved = N * (2 * W * H * 3 // 2 + W * H) + logits.numel() * 2          # frames read and written, labels written, logits
    print(f"\nsemantic maps {N} x {W}x{H} NV12, logits ({N}, {C}, {HS}, {WS}) float16, labels on: RunAsync "
          f"{t_run * 1e3:.1f} us (1 launch), torch chain {t_chain * 1e3:.1f} us, ratio {t_run / t_chain:.4f}; "
          f"{moved / 1e6:.1f} MB moved = {moved / 8e12 * 1e6:.1f} us at 8 TB/s")
    assert t_run <= 1.0 * t_chain, f"RunAsync {t_run * 1e3:.1f} us vs the torch chain {t_chain * 1e3:.1f} us"
