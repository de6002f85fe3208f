"""Loose guard of the GPU JPEG path: 16 frames of 1080p RGB at q = 90 encode at least 5x faster (wall time, whole
Run call: launches, the sizes, the D2H copies and the headers included) with backend="hip" than with the Pillow
backend on the same box.  profiles/jpeg.md has the measured figures."""
import time

import numpy as np
import pytest

import jpeg_model as jm

pytest.importorskip("PIL.Image")
pytestmark = pytest.mark.gpu


def _best(fn, reps):
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def test_hip_backend_is_at_least_5x_faster_than_pillow(vali, gpu):
    w, h, n = 1920, 1080, 16
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:h, 0:w]
    surfs = []
    for i in range(n):       # smooth picture + mild noise: a realistic bit rate, not the worst case
        rgb = np.stack([(xx + 7 * i) % 256, (yy + xx // 3) % 256, (2 * yy + 11 * i) % 256], -1).astype(np.int16)
        rgb = np.clip(rgb + rng.integers(-6, 7, rgb.shape), 0, 255).astype(np.uint8)
        s = vali.Surface.Make(vali.RGB, w, h, gpu)
        assert vali.PyFrameUploader(gpu).Run(rgb.reshape(-1), s)[0]
        surfs.append(s)
    hip = vali.PyNvJpegEncoder(gpu, backend="hip")
    cpu = vali.PyNvJpegEncoder(gpu, backend="cpu")
    ctx = hip.Context(90, vali.RGB)
    out, info = hip.Run(ctx, surfs)                          # warm-up: buffers, headers, code objects
    assert info == vali.TaskExecInfo.SUCCESS and len(out) == n
    assert bytes(out[3].tobytes()) == jm.encode(jm.RGB, _host(vali, gpu, surfs[3]), w, h, 90)
    t_hip = _best(lambda: hip.Run(ctx, surfs), 5)
    t_cpu = _best(lambda: cpu.Run(ctx, surfs), 2)
    print(f"16 x 1080p RGB q90: hip {t_hip * 1e3:.1f} ms, cpu {t_cpu * 1e3:.1f} ms, {t_cpu / t_hip:.1f}x")
    assert t_cpu >= 5 * t_hip, (t_hip, t_cpu)


def _host(vali, gpu, s):
    host = np.zeros(s.HostSize, np.uint8)
    assert vali.PySurfaceDownloader(gpu).Run(s, host)[0]
    return host
