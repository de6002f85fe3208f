"""Loose guard of the GPU JPEG decoder: 16 files of 1080p 4:2:0 q90 without restart markers (Pillow's default) decode
at least 5x faster with PyNvJpegDecoder (whole Run calls: parsing, the staging and H2D copy, the launches and the
status read back included) than with Pillow on one thread.  profiles/jpeg_decode.md has the measured figures."""
import io
import time

import numpy as np
import pytest

PIL = pytest.importorskip("PIL.Image")
pytestmark = pytest.mark.gpu


def _best(fn, reps):
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def test_hip_decoder_is_at_least_5x_faster_than_pillow(vali, gpu):
    w, h, n = 1920, 1080, 16
    yy, xx = np.mgrid[0:h, 0:w]
    files = []
    for i in range(n):      # smooth picture + mild noise: a realistic bit rate, not the worst case
        rng = np.random.default_rng(i)
        rgb = np.stack([(xx + 7 * i) % 256, (yy + xx // 3) % 256, (2 * yy + 11 * i) % 256], -1).astype(np.int16)
        rgb = np.clip(rgb + rng.integers(-6, 7, rgb.shape), 0, 255).astype(np.uint8)
        out = io.BytesIO()
        PIL.fromarray(rgb).save(out, "JPEG", quality=90, subsampling=2)
        files.append(out.getvalue())
    dec = vali.PyNvJpegDecoder(gpu)
    surfaces, info = dec.Run(files, vali.RGB)                 # warm-up: buffers, header cache, code objects
    assert info == vali.TaskExecInfo.SUCCESS and len(surfaces) == n
    host = np.zeros(surfaces[5].HostSize, np.uint8)
    assert vali.PySurfaceDownloader(gpu).Run(surfaces[5], host)[0]
    assert np.array_equal(host.reshape(h, w, 3), np.asarray(PIL.open(io.BytesIO(files[5])).convert("RGB")))

    def hip():
        s, i = dec.Run(files, vali.RGB)
        assert i == vali.TaskExecInfo.SUCCESS

    def pillow():
        for f in files:
            PIL.open(io.BytesIO(f)).convert("RGB").load()

    t_hip, t_cpu = _best(hip, 8), _best(pillow, 3)
    print(f"16 x 1080p 4:2:0 q90: hip {1e3 * t_hip:.2f} ms, Pillow one thread {1e3 * t_cpu:.2f} ms, "
          f"{t_cpu / t_hip:.1f}x")
    assert t_cpu / t_hip >= 5.0, (t_hip, t_cpu)
