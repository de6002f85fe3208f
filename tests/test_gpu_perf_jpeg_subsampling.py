"""Guard of the subsampled GPU JPEG path: 16 frames of 1080p RGB at q = 90 encode with subsampling="420" in at most
1.25 times the wall time of the 4:4:4 `Run` of the same surfaces in the same process (whole Run calls: launches, the
sizes, the D2H copies and the headers included).  The 4:4:4 path is the yardstick; the margin is the process-to-process
spread of one binary on one box, not an expectation that 4:2:0 is slower: it codes half the blocks.
profiles/jpeg_subsampling.md has the measured figures."""
import time

import numpy as np
import pytest

import jpeg_model as jm
import jpeg_subsample_model as sm

pytest.importorskip("PIL.Image")
pytestmark = pytest.mark.gpu


def _best(fn, reps):
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def test_420_run_takes_at_most_1_25x_the_444_run(vali, gpu):
    w, h, n = 1920, 1080, 16
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:h, 0:w]
    surfs = []
    for i in range(n):       # the surfaces of tests/test_gpu_perf_jpeg.py: a smooth picture + mild noise
        rgb = np.stack([(xx + 7 * i) % 256, (yy + xx // 3) % 256, (2 * yy + 11 * i) % 256], -1).astype(np.int16)
        rgb = np.clip(rgb + rng.integers(-6, 7, rgb.shape), 0, 255).astype(np.uint8)
        s = vali.Surface.Make(vali.RGB, w, h, gpu)
        assert vali.PyFrameUploader(gpu).Run(rgb.reshape(-1), s)[0]
        surfs.append(s)
    host3 = np.zeros(surfs[3].HostSize, np.uint8)
    assert vali.PySurfaceDownloader(gpu).Run(surfs[3], host3)[0]
    enc = vali.PyNvJpegEncoder(gpu, backend="hip")
    c444, c420 = enc.Context(90, vali.RGB), enc.Context(90, vali.RGB, subsampling="420")
    for ctx, samp in ((c444, "444"), (c420, "420")):         # warm-up: buffers, headers, code objects
        out, info = enc.Run(ctx, surfs)
        assert info == vali.TaskExecInfo.SUCCESS and len(out) == n
        assert bytes(out[3].tobytes()) == sm.encode(jm.RGB, host3, w, h, 90, samp)
    t444 = _best(lambda: enc.Run(c444, surfs), 5)
    t420 = _best(lambda: enc.Run(c420, surfs), 5)
    print(f"16 x 1080p RGB q90: 4:4:4 {t444 * 1e3:.2f} ms, 4:2:0 {t420 * 1e3:.2f} ms, ratio {t420 / t444:.2f}")
    assert t420 <= 1.25 * t444, (t444, t420)
