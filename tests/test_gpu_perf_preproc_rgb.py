"""Cliff guard of the RGB-source region path (conditions, not measurements): in one process, alternating three times
and keeping the minimum of each side, batch 64,
  - RGB 1080p -> 640 x 640 RGB_32F_PLANAR letterbox in one RunRoiBatchAsync takes less time than the chain it replaces:
    batched resizer + two batched converter steps + a pad fill of the canvases (ONE memset of the canvases' bytes;
    the torch part left out -- both in the chain's favour).  The chain moves over twice the bytes in four launches.
  - RGB 1080p -> RGB_32F_PLANAR at equal size takes no longer than RGB -> RGB_32F + RGB_32F -> RGB_32F_PLANAR batched.
Measured ratios: profiles/preproc_rgb.md."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
N = 64


def _timed(gpu, stream, fn, reps=8):
    from vali_amd._native import shim

    for _ in range(2):
        fn()
    e0, e1 = shim.event_create(gpu), shim.event_create(gpu)
    shim.event_record(gpu, e0, stream)
    for _ in range(reps):
        fn()
    shim.event_record(gpu, e1, stream)
    shim.event_sync(gpu, e1)
    ms = shim.event_elapsed_ms(e0, e1) / reps
    shim.event_destroy(gpu, e0)
    shim.event_destroy(gpu, e1)
    return ms


def _alternate(gpu, stream, a, b):
    ta = tb = 1e9
    for _ in range(3):
        ta = min(ta, _timed(gpu, stream, a))
        tb = min(tb, _timed(gpu, stream, b))
    return ta, tb


def _sources(vali, gpu, w, h, n):
    host = np.random.default_rng(1).integers(0, 256, w * h * 3, dtype=np.uint8)
    up = vali.PyFrameUploader(gpu)
    out = [vali.Surface.Make(vali.RGB, w, h, gpu) for _ in range(n)]
    for s in out:
        assert up.Run(host, s)[0]
    return out


def _make(vali, gpu, fmt, w, h):
    return [vali.Surface.Make(fmt, w, h, gpu) for _ in range(N)]


def test_letterbox_beats_the_chain_it_replaces(vali, gpu):
    from vali_amd._native import shim

    srcs = _sources(vali, gpu, 1920, 1080, N)
    place = vali.letterbox_rect(1920, 1080, 640, 640)
    pp = vali.PySurfacePreprocessor(gpu, mean=MEAN, std=STD, div=255.0)
    stream = pp.Stream
    fused = pp.PrepareRoiBatch(srcs, _make(vali, gpu, vali.RGB_32F_PLANAR, 640, 640), None, [place] * N)
    # the chain: resize to the placement's size, RGB -> RGB_32F -> RGB_32F_PLANAR, and the canvases' pad fill
    rs = vali.PySurfaceResizer(vali.RGB, gpu, stream, interpolation=vali.Interpolation.LINEAR)
    cvt = vali.PySurfaceConverter(gpu, stream)
    small = _make(vali, gpu, vali.RGB, place[2], place[3])
    f32 = _make(vali, gpu, vali.RGB_32F, place[2], place[3])
    pl = _make(vali, gpu, vali.RGB_32F_PLANAR, place[2], place[3])
    b_rs, b_f, b_p = rs.PrepareBatch(srcs, small), cvt.PrepareBatch(small, f32), cvt.PrepareBatch(f32, pl)
    canvas_bytes = N * 3 * 640 * 640 * 4
    canvases = shim.mem_alloc(gpu, canvas_bytes)

    def chain():
        shim.memset2d_async(gpu, canvases, 1 << 20, 0, 1 << 20, canvas_bytes >> 20, stream)
        assert rs.RunBatchAsync(b_rs)[0] and cvt.RunBatchAsync(b_f)[0] and cvt.RunBatchAsync(b_p)[0]

    try:
        t_chain, t_fused = _alternate(gpu, stream, chain, lambda: pp.RunRoiBatchAsync(fused, (114, 114, 114)))
    finally:
        shim.stream_sync(gpu, stream)
        shim.mem_free(gpu, canvases)
    print(f"letterbox 1080p -> 640 x 640, batch {N}: fused {t_fused * 1e3 / N:.2f} us, chain {t_chain * 1e3 / N:.2f} us "
          f"per frame, ratio {t_fused / t_chain:.3f}")
    assert t_fused < t_chain, f"fused {t_fused * 1e3:.1f} us vs chain {t_chain * 1e3:.1f} us"


def test_equal_size_keeps_up_with_the_two_converters(vali, gpu):
    srcs = _sources(vali, gpu, 1920, 1080, N)
    pp = vali.PySurfacePreprocessor(gpu, mean=MEAN, std=STD, div=255.0)
    stream = pp.Stream
    fused = pp.PrepareBatch(srcs, _make(vali, gpu, vali.RGB_32F_PLANAR, 1920, 1080))
    cvt = vali.PySurfaceConverter(gpu, stream)
    f32 = _make(vali, gpu, vali.RGB_32F, 1920, 1080)
    pl = _make(vali, gpu, vali.RGB_32F_PLANAR, 1920, 1080)
    b_f, b_p = cvt.PrepareBatch(srcs, f32), cvt.PrepareBatch(f32, pl)

    def chain():
        assert cvt.RunBatchAsync(b_f)[0] and cvt.RunBatchAsync(b_p)[0]

    t_chain, t_fused = _alternate(gpu, stream, chain, lambda: pp.RunBatchAsync(fused))
    print(f"1080p -> 1080p, batch {N}: fused {t_fused * 1e3 / N:.2f} us, chain {t_chain * 1e3 / N:.2f} us per frame, "
          f"ratio {t_fused / t_chain:.3f}")
    assert t_fused <= t_chain, f"fused {t_fused * 1e3:.1f} us vs chain {t_chain * 1e3:.1f} us"
