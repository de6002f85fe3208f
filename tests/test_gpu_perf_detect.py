"""Speed of PyDetectionSelector.Run on a YOLOv8-sized head: 16 x 8400 x 80 float16 in the head's own layout (N, 4 + C, K),
passed as two transposed slices, T = 1024, D = 100, seeded so that about 300 candidates per frame pass.

The yardstick is the device part of the torch chain a user writes today, on the same stream in the same process, each run
between two events, the median of 25 runs after warm-up, the two alternating: scores.float().max(-1), the mask, topk(T),
the gather of the boxes, and the (N, T, T) IoU matrix with its threshold and class mask.  That chain stops BEFORE the
sequential suppression -- it has no detections yet -- and needs some twenty launches; Run issues four and ends with
dets, counts, rois and marks written.  So Run may take at most 1.0 times the chain, with no further margin.
Measured on an MI355X: Run 48.9 us against 545.5 us for the chain, ratio 0.09 (profiles/detect_select.md)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

N, K, C, T, D = 16, 8400, 80, 1024, 100
PASSING = 300
LETTERBOX = (0, 0, 1920, 1080, 0, 140, 640, 360)
THR, IOU = 0.25, 0.45
PEAK = 8e12


def yolo_head(gpu, seed=0):
    """(N, 4 + C, K) float16: xyxy boxes inside the letterboxed picture, scores below the threshold except for PASSING
    candidates per frame"""
    rng = np.random.default_rng(seed)
    scores = (rng.random((N, K, C)) * 0.2).astype(np.float32)
    for i in range(N):
        k = rng.permutation(K)[:PASSING]
        scores[i, k, rng.integers(0, C, PASSING)] = 0.3 + 0.65 * rng.random(PASSING)
    x, y = rng.random((N, K)) * 560, 140 + rng.random((N, K)) * 300
    w, h = 20 + rng.random((N, K)) * 60, 20 + rng.random((N, K)) * 60
    boxes = np.stack([x, y, x + w, y + h], 2).astype(np.float32)
    pred = torch.from_numpy(np.concatenate([boxes, scores], 2)).to(f"cuda:{gpu}").to(torch.float16)
    return pred.transpose(1, 2).contiguous()


def _medians(fns, runs=25, warm=5):
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


def test_run_is_no_slower_than_the_torch_chain_before_its_suppression(vali, gpu):
    torch.cuda.set_device(gpu)
    stream = torch.cuda.current_stream(gpu).cuda_stream          # torch's work and ours on one stream
    pred = yolo_head(gpu)
    boxes, scores = pred[:, :4].transpose(1, 2), pred[:, 4:].transpose(1, 2)
    assert scores.stride() == ((4 + C) * K, 1, K)
    dev = pred.device
    dets = torch.zeros((N * D, 8), dtype=torch.int32, device=dev)
    counts = torch.zeros((N,), dtype=torch.int32, device=dev)
    rois, marks = torch.zeros_like(dets), torch.zeros_like(dets)
    rects = torch.tensor([LETTERBOX] * N, dtype=torch.int32, device=dev)
    style = vali.DetectionStyle(colours=torch.tensor([vali.pack_colour(40, 255, 80)], dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    sel = vali.PyDetectionSelector(gpu, stream)
    sb = sel.Prepare(boxes, scores, dets, counts, rois, marks, max_candidates=T, max_det=D)

    def run():
        assert sel.RunAsync(sb, rects, THR, IOU, crop_placement=(0, 0, 224, 224), style=style)[0]

    def chain():
        s, cls = scores.float().max(-1)
        s = torch.where(s > THR, s, torch.full_like(s, -float("inf")))
        top, idx = s.topk(T, dim=1)
        b = boxes.gather(1, idx[..., None].expand(-1, -1, 4)).float()
        c = cls.gather(1, idx)
        x1, y1, x2, y2 = b.unbind(-1)
        iw = (torch.minimum(x2[:, :, None], x2[:, None, :]) - torch.maximum(x1[:, :, None], x1[:, None, :])).clamp_(min=0)
        ih = (torch.minimum(y2[:, :, None], y2[:, None, :]) - torch.maximum(y1[:, :, None], y1[:, None, :])).clamp_(min=0)
        inter = iw * ih
        a = (x2 - x1) * (y2 - y1)
        uni = (a[:, :, None] + a[:, None, :]) - inter
        return (inter > IOU * uni) & (c[:, :, None] == c[:, None, :]) & (top > THR)[:, :, None]

    run()
    torch.cuda.synchronize()
    got = counts.cpu().numpy()
    passing = (scores.float().max(-1)[0] > THR).sum(1).cpu().numpy()
    assert (np.abs(passing - PASSING) <= 30).all() and (got > 20).all() and (got <= D).all(), (passing, got)
    t_run, t_chain = _medians([run, chain])
    score_bytes = N * K * C * 2 + N * K * 4 * 2
    print(f"\ndetect select {N} x {K} x {C} float16, T = {T}, D = {D}, ~{PASSING} passing: Run {t_run * 1e3:.1f} us (4 launches), "
          f"torch chain without its suppression {t_chain * 1e3:.1f} us, ratio {t_run / t_chain:.4f}; the head is "
          f"{score_bytes / 1e6:.1f} MB, {score_bytes / PEAK * 1e6:.2f} us at 8 TB/s")
    assert t_run <= 1.0 * t_chain, f"Run {t_run * 1e3:.1f} us vs the torch chain {t_chain * 1e3:.1f} us"
