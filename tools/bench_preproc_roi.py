#!/usr/bin/env python3
"""Regions of the fused preprocessor (PySurfacePreprocessor.RunRoiBatchAsync, kernel k_nv12_preproc_roi).

  full_canvas  crop = source, placement = destination, no padding, batch 64, at the three geometries of
               bench_configs.preproc; the same frames through RunBatchAsync (k_nv12_preproc) alongside
  letterbox    1920x1080 -> 640x640 RGB_32F_PLANAR, pad 114, batch 64
  mixed_crops  256 crops of 32-512 px of one 1080p frame -> 224x224 RGB_32F_PLANAR, pad 114
Bytes: the source rows the bilinear grid touches (luma and chroma, over the crop's width) plus 12 B per WRITTEN
destination pixel (pixels a no-padding item leaves alone do not count).  Kernel time = HIP events on the task's
stream, best of 5 windows of 20 launches.  Prints one JSON object per line; --out also writes them to a file.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import vali_amd as vali  # noqa: E402
from vali_amd._native import shim  # noqa: E402

DEV = 0
PEAK_GBS = 8000.0
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def touched_rows(src_rows, dst_rows):
    """distinct source rows the bilinear grid of make_lerp reads (float32 scale, as the kernel)"""
    if src_rows == dst_rows:
        return src_rows
    scale = np.float32(src_rows) / np.float32(dst_rows)
    f = np.arange(dst_rows, dtype=np.float32) * scale
    i0 = np.minimum(np.floor(f).astype(np.int64), src_rows - 1)
    return len(np.union1d(i0, np.minimum(i0 + 1, src_rows - 1)))


def item_bytes(crop, place, canvas, pad):
    _, _, sw, sh = crop
    _, _, dw, dh = place
    read = sw * touched_rows(sh, dh) + sw * touched_rows(sh // 2, dh // 2)
    written = canvas[0] * canvas[1] if pad else dw * dh
    return read + 12 * written


def timed(stream, fn, reps=20, windows=5):
    for _ in range(3):
        fn()
    best = 1e9
    for _ in range(windows):
        e0, e1 = shim.event_create(DEV), shim.event_create(DEV)
        shim.event_record(DEV, e0, stream)
        for _ in range(reps):
            ok, info = fn()
            assert ok, info
        shim.event_record(DEV, e1, stream)
        shim.event_sync(DEV, e1)
        best = min(best, shim.event_elapsed_ms(e0, e1) / reps)
        shim.event_destroy(DEV, e0)
        shim.event_destroy(DEV, e1)
    return best


def sources(w, h, n):
    host = np.random.default_rng(w + h).integers(16, 236, w * h * 3 // 2, dtype=np.uint8)
    up = vali.PyFrameUploader(DEV)
    out = [vali.Surface.Make(vali.NV12, w, h, DEV) for _ in range(n)]
    for s in out:
        assert up.Run(host, s)[0]
    return out


def line(name, ms, nbytes, extra):
    gbs = nbytes / (ms * 1e-3) / 1e9
    r = {"config": name, "us": round(ms * 1e3, 2), "bytes": int(nbytes), "GB_s": round(gbs, 1),
         "frac_8TBs": round(gbs / PEAK_GBS, 3)}
    r.update(extra)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert vali.GetNumGpus() > 0, "needs a HIP device"
    n = args.n
    pp = vali.PySurfacePreprocessor(DEV, mean=MEAN, std=STD, div=255.0)
    cc = vali.ColorspaceConversionContext(vali.ColorSpace.BT_709, vali.ColorRange.MPEG)
    out = []
    for (sw, sh, dw, dh) in ((1920, 1080, 1920, 1080), (3840, 2160, 640, 640), (1920, 1080, 640, 384)):
        srcs = sources(sw, sh, n)
        dsts = [vali.Surface.Make(vali.RGB_32F_PLANAR, dw, dh, DEV) for _ in range(n)]
        plain, roi = pp.PrepareBatch(srcs, dsts), pp.PrepareRoiBatch(srcs, dsts)
        t_plain = t_roi = 1e9
        for _ in range(3):        # alternate: the two forms see the same box state
            t_plain = min(t_plain, timed(pp.Stream, lambda: pp.RunBatchAsync(plain, None, cc)))
            t_roi = min(t_roi, timed(pp.Stream, lambda: pp.RunRoiBatchAsync(roi, None, cc)))
        b = n * item_bytes((0, 0, sw, sh), (0, 0, dw, dh), (dw, dh), False)
        out.append(line(f"full_canvas {sw}x{sh}->{dw}x{dh} b{n}", t_roi, b,
                        {"us_per_frame": round(t_roi * 1e3 / n, 3), "batch_us": round(t_plain * 1e3, 2),
                         "roi_over_batch": round(t_roi / t_plain, 3)}))
        del srcs, dsts, plain, roi

    srcs = sources(1920, 1080, n)
    dsts = [vali.Surface.Make(vali.RGB_32F_PLANAR, 640, 640, DEV) for _ in range(n)]
    place = vali.letterbox_rect(1920, 1080, 640, 640)
    lb = pp.PrepareRoiBatch(srcs, dsts, None, [place] * n)
    t = timed(pp.Stream, lambda: pp.RunRoiBatchAsync(lb, (114, 114, 114), cc))
    out.append(line(f"letterbox 1920x1080->640x640 b{n}", t, n * item_bytes((0, 0, 1920, 1080), place, (640, 640), True),
                    {"us_per_frame": round(t * 1e3 / n, 3)}))
    del dsts, lb

    m = 256
    rng = np.random.default_rng(7)
    crops = []
    for _ in range(m):
        w, h = (int(v) & ~1 for v in rng.integers(32, 513, 2))
        crops.append((int(rng.integers(0, 1920 - w + 1)) & ~1, int(rng.integers(0, 1080 - h + 1)) & ~1, w, h))
    dsts = [vali.Surface.Make(vali.RGB_32F_PLANAR, 224, 224, DEV) for _ in range(m)]
    mc = pp.PrepareRoiBatch([srcs[0]] * m, dsts, crops)
    t = timed(pp.Stream, lambda: pp.RunRoiBatchAsync(mc, (114, 114, 114), cc))
    b = sum(item_bytes(c, (0, 0, 224, 224), (224, 224), True) for c in crops)
    whole = pp.PrepareBatch(srcs, dsts[:n])
    t_whole = timed(pp.Stream, lambda: pp.RunBatchAsync(whole, None, cc))
    out.append(line(f"mixed_crops 256 x 32-512px of 1080p->224x224", t, b,
                    {"us_per_crop": round(t * 1e3 / m, 3), "whole_1080p_224_us_per_frame": round(t_whole * 1e3 / n, 3)}))
    for r in out:
        print(json.dumps(r), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("".join(json.dumps(r) + "\n" for r in out))


if __name__ == "__main__":
    main()
