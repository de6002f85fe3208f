#!/usr/bin/env python3
"""Regions of the fused preprocessor from RGB-family sources (kernel k_rgb_preproc_roi), each next to the NV12 figure
of the same geometry from the same run:

  letterbox    1920x1080 -> 640x640 RGB_32F_PLANAR, pad 114, batch 64
  same_size    1920x1080 -> 1920x1080 RGB_32F_PLANAR, whole surfaces, batch 64
  mixed_crops  256 crops of 32-512 px of one 1080p frame -> 224x224 RGB_32F_PLANAR, pad 114
Bytes: the source rows the bilinear grid touches over the crop's width (3 B per pixel for RGB sources, luma + chroma
for NV12) plus 12 B per written destination pixel.  Kernel time = HIP events on the task's stream, best of 5 windows
of 20 launches (tools/bench_preproc_roi.py's timer).  One JSON object per line; --out also writes them to a file.

    python tools/bench_preproc_rgb.py [--src-format RGB|BGR|RGB_PLANAR] [--n 64] [--out FILE]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from bench_preproc_roi import DEV, MEAN, STD, item_bytes, line, sources, timed, touched_rows, vali  # noqa: E402


def rgb_item_bytes(crop, place, canvas, pad):
    _, _, sw, sh = crop
    _, _, dw, dh = place
    return 3 * sw * touched_rows(sh, dh) + 12 * (canvas[0] * canvas[1] if pad else dw * dh)


def rgb_sources(fmt, w, h, n):
    host = np.random.default_rng(w + h).integers(0, 256, w * h * 3, dtype=np.uint8)
    up = vali.PyFrameUploader(DEV)
    out = [vali.Surface.Make(fmt, w, h, DEV) for _ in range(n)]
    for s in out:
        assert up.Run(host, s)[0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src-format", default="RGB", choices=["RGB", "BGR", "RGB_PLANAR"])
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert vali.GetNumGpus() > 0, "needs a HIP device"
    n, fmt = args.n, getattr(vali.PixelFormat, args.src_format)
    pp = vali.PySurfacePreprocessor(DEV, mean=MEAN, std=STD, div=255.0)
    cc = vali.ColorspaceConversionContext(vali.ColorSpace.BT_709, vali.ColorRange.MPEG)
    rgb, nv = rgb_sources(fmt, 1920, 1080, n), sources(1920, 1080, n)
    out = []

    def both(name, make_batch, nbytes_rgb, nbytes_nv, pad, per, count):
        b_rgb, b_nv = make_batch(rgb), make_batch(nv)
        t_rgb = t_nv = 1e9
        for _ in range(3):        # alternate: the two sources see the same box state
            t_rgb = min(t_rgb, timed(pp.Stream, lambda: pp.RunRoiBatchAsync(b_rgb, pad)))
            t_nv = min(t_nv, timed(pp.Stream, lambda: pp.RunRoiBatchAsync(b_nv, pad, cc)))
        r_nv = line(name + " NV12", t_nv, nbytes_nv, {})
        out.append(line(f"{name} {args.src_format}", t_rgb, nbytes_rgb,
                        {per: round(t_rgb * 1e3 / count, 3), "nv12_" + per: round(t_nv * 1e3 / count, 3),
                         "nv12_frac_8TBs": r_nv["frac_8TBs"]}))

    whole = (0, 0, 1920, 1080)
    place = vali.letterbox_rect(1920, 1080, 640, 640)
    dsts = [vali.Surface.Make(vali.RGB_32F_PLANAR, 640, 640, DEV) for _ in range(n)]
    both(f"letterbox 1920x1080->640x640 b{n}", lambda s: pp.PrepareRoiBatch(s, dsts, None, [place] * n),
         n * rgb_item_bytes(whole, place, (640, 640), True), n * item_bytes(whole, place, (640, 640), True),
         (114, 114, 114), "us_per_frame", n)
    dsts = [vali.Surface.Make(vali.RGB_32F_PLANAR, 1920, 1080, DEV) for _ in range(n)]
    both(f"same_size 1920x1080 b{n}", lambda s: pp.PrepareRoiBatch(s, dsts),
         n * rgb_item_bytes(whole, whole, (1920, 1080), False), n * item_bytes(whole, whole, (1920, 1080), False),
         None, "us_per_frame", n)
    m = 256
    rng = np.random.default_rng(7)
    crops = []
    for _ in range(m):
        w, h = (int(v) & ~1 for v in rng.integers(32, 513, 2))
        crops.append((int(rng.integers(0, 1920 - w + 1)) & ~1, int(rng.integers(0, 1080 - h + 1)) & ~1, w, h))
    dsts = [vali.Surface.Make(vali.RGB_32F_PLANAR, 224, 224, DEV) for _ in range(m)]
    box = (0, 0, 224, 224)
    both("mixed_crops 256 x 32-512px of 1080p->224x224", lambda s: pp.PrepareRoiBatch([s[0]] * m, dsts, crops),
         sum(rgb_item_bytes(c, box, (224, 224), True) for c in crops),
         sum(item_bytes(c, box, (224, 224), True) for c in crops), (114, 114, 114), "us_per_crop", m)
    for r in out:
        print(json.dumps(r), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("".join(json.dumps(r) + "\n" for r in out))


if __name__ == "__main__":
    main()
