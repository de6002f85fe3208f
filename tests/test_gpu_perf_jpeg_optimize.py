"""What per-image Huffman tables cost: whole `Run` calls of 8 x 1080p at quality 90 and 4:2:0 with and without
`optimize`, on the test's own machine, in one process, warm, as the median of 15 interleaved calls each (as
tests/test_gpu_perf_jpeg_tensor.py times its calls).

The guard is the ratio measured on one MI355X when the feature was written (profiles/jpeg_optimize.md) times 1.25,
rounded up to one decimal: the margin is the 27 % process-to-process spread this project has recorded for one binary on
one box.  The optimised files must also be smaller, by what the model of a smaller picture of the
same content promises (tests/test_gpu_jpeg_optimize.py pins the bytes)."""
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
MEASURED_RATIO = 1.18     # optimised / plain, profiles/jpeg_optimize.md
GUARD = 1.5                # ceil(MEASURED_RATIO * 1.25, one decimal)


def _pictures():
    """the reference's frame tiled to 1920 x 1080, every item shifted"""
    frame = np.asarray(PIL.open(GOLDEN / "frame_0.jpg").convert("RGB"))
    fh, fw = frame.shape[:2]
    tiled = np.tile(frame, (-(-(H + 64) // fh), -(-(W + 64) // fw), 1))
    return [np.ascontiguousarray(tiled[8 * i:8 * i + H, 8 * i:8 * i + W]) for i in range(N)]


@pytest.mark.gpu
def test_optimised_run_costs_no_more_than_the_guard(vali, gpu):
    surfs = []
    for p in _pictures():
        s = vali.Surface.Make(vali.RGB, W, H, gpu)
        ok, info = vali.PyFrameUploader(gpu).Run(p.reshape(-1), s)
        assert ok, info
        surfs.append(s)
    enc = vali.PyNvJpegEncoder(gpu, backend="hip")
    ctxs = [enc.Context(90, vali.RGB, subsampling="420"), enc.Context(90, vali.RGB, subsampling="420", optimize=True)]
    sizes = [0, 0]

    def call(k):
        files, info = enc.Run(ctxs[k], surfs)
        assert info == vali.TaskExecInfo.SUCCESS
        sizes[k] = sum(f.size for f in files)

    for k in (0, 1):
        call(k)
        call(k)
    times = [[], []]
    for _ in range(CALLS):
        for k in (0, 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(k)
            times[k].append((time.perf_counter() - t0) * 1e3)
    plain, opt = (statistics.median(t) for t in times)
    print(f"\njpeg_optimize ({N}, {H}, {W}) RGB 4:2:0 q90: Run {plain:.3f} ms, Run with optimize {opt:.3f} ms, "
          f"ratio {opt / plain:.3f} (guard {GUARD}); bytes {sizes[0]} -> {sizes[1]}, ratio {sizes[1] / sizes[0]:.3f}")
    assert sizes[1] < sizes[0]
    assert opt <= GUARD * plain, (opt, plain)
