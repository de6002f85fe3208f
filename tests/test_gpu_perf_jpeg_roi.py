"""What RunRoi costs, on the test's own machine, in one process, warm, as the median of 15 interleaved calls each (as
tests/test_gpu_perf_jpeg_optimize.py times its calls).

1. Uniform: 8 x 1080p RGB surfaces, 4:2:0, quality 90, whole-surface rectangles, `RunRoi` against `Run` on the same
   surfaces.  The guard is the ratio measured on one MI355X when the feature was written (profiles/jpeg_roi.md) times
   1.25, rounded up to one decimal: the margin is the 27 % process-to-process spread this project has recorded for one
   binary on one box.
2. Thumbnails: 64 rectangles of distinct sizes between 32 and 256 pixels out of one 1080p frame, one `RunRoi` against
   today's route, 64 `Run` calls on ready-made copies of the crops (making the copies is not timed).  The assertion is
   what the design promises, not a tuned number: the one call takes no longer than the 64."""
import statistics
import time
from pathlib import Path

import numpy as np
import pytest

PIL = pytest.importorskip("PIL.Image")
torch = pytest.importorskip("torch")

GOLDEN = Path(__file__).resolve().parent / "golden"
N, H, W = 8, 1080, 1920
CALLS = 15
MEASURED_RATIO = 1.03     # RunRoi / Run, profiles/jpeg_roi.md
GUARD = 1.3                # ceil(MEASURED_RATIO * 1.25, one decimal)


def _pictures(n):
    """the reference's frame tiled to 1920 x 1080, every item shifted"""
    frame = np.asarray(PIL.open(GOLDEN / "frame_0.jpg").convert("RGB"))
    fh, fw = frame.shape[:2]
    tiled = np.tile(frame, (-(-(H + 64) // fh), -(-(W + 64) // fw), 1))
    return [np.ascontiguousarray(tiled[8 * i:8 * i + H, 8 * i:8 * i + W]) for i in range(n)]


def _upload(vali, gpu, rgb):
    h, w = rgb.shape[:2]
    s = vali.Surface.Make(vali.RGB, w, h, gpu)
    ok, info = vali.PyFrameUploader(gpu).Run(np.ascontiguousarray(rgb).reshape(-1), s)
    assert ok, info
    return s


def _median_ms(calls):
    """medians of CALLS interleaved runs of each callable, after two warm calls each"""
    for c in calls:
        c()
        c()
    times = [[] for _ in calls]
    for _ in range(CALLS):
        for k, c in enumerate(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return [statistics.median(t) for t in times]


@pytest.mark.gpu
def test_whole_surfaces_cost_what_run_costs(vali, gpu):
    surfs = [_upload(vali, gpu, p) for p in _pictures(N)]
    enc = vali.PyNvJpegEncoder(gpu, backend="hip")
    ctx = enc.Context(90, vali.RGB, subsampling="420")
    files = [None, None]

    def run():
        files[0], info = enc.Run(ctx, surfs)
        assert info == vali.TaskExecInfo.SUCCESS

    def roi():
        files[1], info = enc.RunRoi(ctx, surfs)
        assert info == vali.TaskExecInfo.SUCCESS

    plain, rois = _median_ms([run, roi])
    assert all(np.array_equal(a, b) for a, b in zip(*files))
    print(f"\njpeg_roi uniform ({N}, {H}, {W}) RGB 4:2:0 q90: Run {plain:.3f} ms, RunRoi {rois:.3f} ms, "
          f"ratio {rois / plain:.3f} (guard {GUARD})")
    assert rois <= GUARD * plain, (rois, plain)


@pytest.mark.gpu
def test_64_thumbnails_in_one_call_take_no_longer_than_64_calls(vali, gpu):
    frame = _pictures(1)[0]
    surf = _upload(vali, gpu, frame)
    rng = np.random.default_rng(64)
    sizes = set()
    while len(sizes) < 64:
        sizes.add(tuple(int(v) for v in rng.integers(32, 257, 2)))
    rects = [(int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h) for w, h in sorted(sizes)]
    crops = [_upload(vali, gpu, frame[y:y + h, x:x + w]) for x, y, w, h in rects]
    enc = vali.PyNvJpegEncoder(gpu, backend="hip")
    ctx = enc.Context(90, vali.RGB, subsampling="420")
    files = [None, None]

    def runs():
        out = []
        for c in crops:
            f, info = enc.Run(ctx, [c])
            assert info == vali.TaskExecInfo.SUCCESS
            out.append(f[0])
        files[0] = out

    def roi():
        files[1], info = enc.RunRoi(ctx, [surf] * len(rects), rects)
        assert info == vali.TaskExecInfo.SUCCESS

    many, one = _median_ms([runs, roi])
    assert all(np.array_equal(a, b) for a, b in zip(*files))
    print(f"\njpeg_roi thumbnails: 64 rectangles of 32..256 pixels out of one {W} x {H} RGB frame, 4:2:0 q90: "
          f"64 Run calls {many:.3f} ms, one RunRoi {one:.3f} ms, ratio {one / many:.3f}")
    assert one <= many, (one, many)
