"""Images per second and MB/s of compressed input of PyNvJpegDecoder (vali_jpeg_decode_batch) against Pillow on one
thread, whole Run calls: parsing (header cache), the staging copy, the one H2D copy, the launches and the status read
back included.  Cases: 16 x 1080p 4:2:0 q90 without restarts (Pillow's default), the same files with restart
markers, 16 x 2160p, a mixed-size batch.  Prints one JSON line per case and a markdown table (profiles/jpeg_decode.md).

  python tools/bench_jpeg_decode.py [--gpu 0] [--quick] [--reps 10]   (--quick: the 1080p case, GPU only: profiling)
"""
import argparse
import io
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import vali_amd as vali  # noqa: E402


def picture(w, h, i):
    """smooth picture + mild noise: a realistic bit rate (about 2.5 bits per pixel at q90 4:2:0)"""
    rng = np.random.default_rng(i)
    yy, xx = np.mgrid[0:h, 0:w]
    rgb = np.stack([(xx + 7 * i) % 256, (yy + xx // 3) % 256, (2 * yy + 11 * i) % 256], -1).astype(np.int16)
    return np.clip(rgb + rng.integers(-6, 7, rgb.shape), 0, 255).astype(np.uint8)


def jpeg(rgb, q=90, restart_blocks=0):
    from PIL import Image

    out = io.BytesIO()
    kw = {"restart_marker_blocks": restart_blocks} if restart_blocks else {}
    Image.fromarray(rgb).save(out, "JPEG", quality=q, subsampling=2, **kw)
    return out.getvalue()


def gpu_rate(dec, files, reps):
    surfaces, info = dec.Run(files, vali.RGB)                 # warm-up: buffers grow, headers cached
    assert info == vali.TaskExecInfo.SUCCESS, dec.last_status
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        ok, info = dec.RunInto(files, surfaces)
        best = min(best, time.perf_counter() - t0)
        assert ok, info
    return best


def pillow_rate(files, reps):
    from PIL import Image

    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        for f in files:
            Image.open(io.BytesIO(f)).convert("RGB").load()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    hd = [picture(1920, 1080, i) for i in range(16)]
    cases = [("16 x 1080p 4:2:0 q90, no restarts", [jpeg(p) for p in hd])]
    if not a.quick:
        cases.append(("16 x 1080p 4:2:0 q90, restart every 2 MCU rows", [jpeg(p, restart_blocks=2 * 120 * 6) for p in hd]))
        cases.append(("16 x 2160p 4:2:0 q90, no restarts", [jpeg(picture(3840, 2160, i)) for i in range(16)]))
        sizes = [(1920, 1080), (1280, 720), (640, 480), (3840, 2160), (320, 240), (1024, 768), (800, 600), (1920, 1080)]
        cases.append(("mixed batch of 8 sizes", [jpeg(picture(w, h, i)) for i, (w, h) in enumerate(sizes)]))
    dec = vali.PyNvJpegDecoder(a.gpu)
    rows = []
    for name, files in cases:
        mb = sum(len(f) for f in files) / 1e6
        t_gpu = gpu_rate(dec, files, a.reps)
        t_cpu = None if a.quick else pillow_rate(files, max(2, a.reps // 4))
        r = {"case": name, "images": len(files), "input_MB": round(mb, 2),
             "hip_ms": round(1e3 * t_gpu, 3), "hip_images_per_s": round(len(files) / t_gpu, 1),
             "hip_MB_per_s": round(mb / t_gpu, 1)}
        if t_cpu is not None:
            r.update({"pillow_ms": round(1e3 * t_cpu, 3), "pillow_images_per_s": round(len(files) / t_cpu, 1),
                      "speedup": round(t_cpu / t_gpu, 2)})
        print(json.dumps(r), flush=True)
        rows.append(r)
    print("\n| case | input MB | hip ms | hip img/s | hip MB/s | Pillow 1 thread ms | speed-up |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['case']} | {r['input_MB']} | {r['hip_ms']} | {r['hip_images_per_s']} | {r['hip_MB_per_s']} | "
              f"{r.get('pillow_ms', '-')} | {r.get('speedup', '-')} |")


if __name__ == "__main__":
    main()
