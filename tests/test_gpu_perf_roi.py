"""Cliff guard of the region path (not a tight floor): in one process, alternating three times and keeping the minimum
of each side,
  - whole-canvas rectangles (crop = source, placement = destination, no padding) against RunBatchAsync at the three
    preprocessor geometries of the secondary benchmark, batch 64: at most 1.25 x its time;
  - 256 mixed crops of 32-512 px from one 1080p frame -> 224 x 224 float planar: at most 2 x the time per frame of
    whole-frame 1080p -> 224 x 224."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


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
    host = np.random.default_rng(1).integers(16, 236, w * h * 3 // 2, dtype=np.uint8)
    up = vali.PyFrameUploader(gpu)
    out = [vali.Surface.Make(vali.NV12, w, h, gpu) for _ in range(n)]
    for s in out:
        assert up.Run(host, s)[0]
    return out


@pytest.mark.parametrize("geom", [(1920, 1080, 1920, 1080), (3840, 2160, 640, 640), (1920, 1080, 640, 384)])
def test_whole_canvas_rects_keep_up_with_the_batch(vali, gpu, geom):
    sw, sh, dw, dh = geom
    n = 64
    srcs = _sources(vali, gpu, sw, sh, n)
    dsts = [vali.Surface.Make(vali.RGB_32F_PLANAR, dw, dh, gpu) for _ in range(n)]
    cc = vali.ColorspaceConversionContext(vali.ColorSpace.BT_709, vali.ColorRange.MPEG)
    pp = vali.PySurfacePreprocessor(gpu, mean=MEAN, std=STD, div=255.0)
    plain = pp.PrepareBatch(srcs, dsts)
    roi = pp.PrepareRoiBatch(srcs, dsts)
    t_plain, t_roi = _alternate(gpu, pp.Stream, lambda: pp.RunBatchAsync(plain, None, cc),
                                lambda: pp.RunRoiBatchAsync(roi, None, cc))
    assert t_roi <= 1.25 * t_plain, f"regions {t_roi * 1e3:.1f} us vs batch {t_plain * 1e3:.1f} us"


def test_mixed_crops_per_crop_cost(vali, gpu):
    n = 256
    frame = _sources(vali, gpu, 1920, 1080, 1)[0]
    rng = np.random.default_rng(7)
    crops = []
    for _ in range(n):
        w, h = (int(v) & ~1 for v in rng.integers(32, 513, 2))
        x, y = int(rng.integers(0, 1920 - w + 1)) & ~1, int(rng.integers(0, 1080 - h + 1)) & ~1
        crops.append((x, y, w, h))
    dsts = [vali.Surface.Make(vali.RGB_32F_PLANAR, 224, 224, gpu) for _ in range(n)]
    pp = vali.PySurfacePreprocessor(gpu, mean=MEAN, std=STD, div=255.0)
    boxes = pp.PrepareRoiBatch([frame] * n, dsts, crops)
    frames = _sources(vali, gpu, 1920, 1080, 64)
    whole = pp.PrepareBatch(frames, dsts[:64])
    t_whole, t_boxes = _alternate(gpu, pp.Stream, lambda: pp.RunBatchAsync(whole),
                                  lambda: pp.RunRoiBatchAsync(boxes, (114, 114, 114)))
    per_frame, per_crop = t_whole / 64, t_boxes / n
    assert per_crop <= 2 * per_frame, f"{per_crop * 1e3:.2f} us per crop vs {per_frame * 1e3:.2f} us per frame"
