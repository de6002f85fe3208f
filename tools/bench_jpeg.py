"""Images per second of PyNvJpegEncoder, backend "hip" (vali_jpeg_encode_batch) against "cpu" (Pillow), whole Run
calls: launches, sizes, the exact D2H copies and the headers included.  1080p and 2160p, RGB and YUV420, q = 90,
batch 1 / 16 / 64.  Prints one JSON line per configuration and a markdown table (profiles/jpeg.md).

  python tools/bench_jpeg.py [--gpu 0] [--quick]     (--quick: 1080p RGB batch 16, hip only: the profiling run)
  python tools/bench_jpeg.py --sampled [--size 3840x2160]
      RGB batch 16 coded 4:4:4, 4:2:2 and 4:2:0 (Context(..., subsampling=...)), hip only, the three alternating in
      one process, best of 5 Run calls each (profiles/jpeg_subsampling.md); with --quick --subsampling 420 one of them
      alone, for a profiling run
  --optimize: every context with optimize=True (per-image Huffman tables, profiles/jpeg_optimize.md); with --sampled
      each sampling is timed with and without it
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import vali_amd as vali  # noqa: E402


def frames(fmt, w, h, k, gpu):
    """k distinct smooth-plus-noise pictures (a realistic bit rate), uploaded"""
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for i in range(k):
        rgb = np.stack([(xx + 7 * i) % 256, (yy + xx // 3) % 256, (2 * yy + 11 * i) % 256], -1).astype(np.int16)
        rgb = np.clip(rgb + rng.integers(-6, 7, rgb.shape), 0, 255).astype(np.uint8)
        s = vali.Surface.Make(vali.RGB, w, h, gpu)
        assert vali.PyFrameUploader(gpu).Run(rgb.reshape(-1), s)[0]
        if fmt != vali.RGB:
            d = vali.Surface.Make(fmt, w, h, gpu)
            assert vali.PySurfaceConverter(gpu).Run(s, d)[0]
            s = d
        out.append(s)
    return out


def run(enc, ctx, surfs, reps):
    enc.Run(ctx, surfs)                                       # warm-up (buffers grow, headers cached)
    best = float("inf")
    nbytes = 0
    for _ in range(reps):
        t0 = time.perf_counter()
        out, info = enc.Run(ctx, surfs)
        best = min(best, time.perf_counter() - t0)
        assert info == vali.TaskExecInfo.SUCCESS
        nbytes = sum(b.size for b in out)
    return best, nbytes


def sampled(a):
    w, h = (int(v) for v in a.size.split("x")) if a.size else (1920, 1080)
    pool = frames(vali.RGB, w, h, 4, a.gpu)
    surfs = [pool[i % len(pool)] for i in range(16)]
    enc = vali.PyNvJpegEncoder(a.gpu, backend="hip")
    ctxs = {s: enc.Context(90, vali.RGB, s) for s in ("444", "422", "420")}
    if a.optimize:
        ctxs.update({s + " optimize": enc.Context(90, vali.RGB, s, optimize=True) for s in ("444", "422", "420")})
    best, nbytes = {s: float("inf") for s in ctxs}, {}
    for s, ctx in ctxs.items():
        enc.Run(ctx, surfs)                                   # warm-up
    for _ in range(5):
        for s, ctx in ctxs.items():
            t0 = time.perf_counter()
            out, info = enc.Run(ctx, surfs)
            best[s] = min(best[s], time.perf_counter() - t0)
            assert info == vali.TaskExecInfo.SUCCESS
            nbytes[s] = sum(b.size for b in out)
    for s in ctxs:
        print(json.dumps({"size": f"{w}x{h}", "format": "RGB", "subsampling": s, "batch": 16,
                          "ms_per_call": round(best[s] * 1e3, 3), "images_per_s": round(16 / best[s], 1),
                          "mean_file_kib": round(nbytes[s] / 16 / 1024, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--sampled", action="store_true")
    ap.add_argument("--subsampling", choices=["444", "422", "420"], default=None, help="of RGB surfaces")
    ap.add_argument("--size", default=None, help="WxH instead of the default sizes")
    ap.add_argument("--optimize", action="store_true", help="per-image Huffman tables")
    a = ap.parse_args()
    if a.sampled:
        return sampled(a)
    sizes = [(1920, 1080)] if a.quick else [(1920, 1080), (3840, 2160)]
    if a.size:
        sizes = [tuple(int(v) for v in a.size.split("x"))]
    fmts = [vali.RGB] if a.quick else [vali.RGB, vali.YUV420]
    batches = [16] if a.quick else [1, 16, 64]
    backends = ["hip"] if a.quick else ["hip", "cpu"]
    rows = []
    for w, h in sizes:
        for fmt in fmts:
            pool = frames(fmt, w, h, 4, a.gpu)
            for n in batches:
                surfs = [pool[i % len(pool)] for i in range(n)]
                for backend in backends:
                    enc = vali.PyNvJpegEncoder(a.gpu, backend=backend)
                    ctx = enc.Context(90, fmt, a.subsampling if fmt == vali.RGB else None, optimize=a.optimize)
                    reps = 10 if backend == "hip" else (3 if n == 1 else 1)
                    t, nbytes = run(enc, ctx, surfs, reps)
                    r = {"size": f"{w}x{h}", "format": fmt.name, "batch": n, "backend": backend, "optimize": a.optimize,
                         "ms_per_call": round(t * 1e3, 3), "images_per_s": round(n / t, 1),
                         "mean_file_kib": round(nbytes / n / 1024, 1)}
                    rows.append(r)
                    print(json.dumps(r), flush=True)
    print("\n| size | format | batch | hip img/s | cpu img/s | hip / cpu | file KiB |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        if r["backend"] != "hip":
            continue
        c = next((x for x in rows if x["backend"] == "cpu" and all(x[k] == r[k] for k in ("size", "format", "batch"))),
                 None)
        cpu = c["images_per_s"] if c else float("nan")
        print(f"| {r['size']} | {r['format']} | {r['batch']} | {r['images_per_s']} | {cpu} | "
              f"{r['images_per_s'] / cpu:.0f}x | {r['mean_file_kib']} |")


if __name__ == "__main__":
    main()
