#!/usr/bin/env python3
"""The fused preprocessor into ONE batch tensor (PySurfacePreprocessor.RunTensorBatchAsync) next to the surface path
(RunRoiBatchAsync into RGB_32F_PLANAR surfaces) on the same frames, for float32 / float16 / bfloat16 x planar /
channels last:

  letterbox    1920x1080 -> 640x640, pad 114: the detector input (resized gather + bands of pure writes)
  same_size    1920x1080 -> 1920x1080, whole canvas: the streaming branch, bound by the bytes it writes
  classifier   1920x1080 -> 224x224, whole canvas: the TALL tiles

Bytes: tools/bench_preproc_roi.py's (the source rows the bilinear grid touches plus the written elements at their
size).  Kernel time = HIP events on the task's stream, best of 5 windows of 20 launches, each tensor form alternated with
the surface form three times.  Prints one JSON object per line; --out also writes them to a file."""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import vali_amd as vali  # noqa: E402
from bench_preproc_roi import DEV, MEAN, STD, PEAK_GBS, sources, timed, touched_rows  # noqa: E402

import torch  # noqa: E402

FORMS = [(torch.float32, 4), (torch.float16, 2), (torch.bfloat16, 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert vali.GetNumGpus() > 0, "needs a HIP device"
    n = args.n
    pp = vali.PySurfacePreprocessor(DEV, mean=MEAN, std=STD, div=255.0)
    cc = vali.ColorspaceConversionContext(vali.ColorSpace.BT_709, vali.ColorRange.MPEG)
    sw, sh = 1920, 1080
    srcs = sources(sw, sh, n)
    out = []
    for name, (dw, dh), place, pad in (("letterbox", (640, 640), vali.letterbox_rect(sw, sh, 640, 640), (114, 114, 114)),
                                       ("same_size", (1920, 1080), (0, 0, 1920, 1080), None),
                                       ("classifier", (224, 224), (0, 0, 224, 224), None)):
        read = n * (sw * touched_rows(sh, place[3]) + sw * touched_rows(sh // 2, place[3] // 2))
        elems = n * 3 * dw * dh
        dsts = [vali.Surface.Make(vali.RGB_32F_PLANAR, dw, dh, DEV) for _ in range(n)]
        roi = pp.PrepareRoiBatch(srcs, dsts, None, [place] * n)
        for dtype, esize in FORMS:
            for layout in ("planar", "packed"):
                t = torch.empty((n, 3, dh, dw), dtype=dtype, device=f"cuda:{DEV}")
                if layout == "packed":
                    t = t.contiguous(memory_format=torch.channels_last)
                torch.cuda.synchronize()
                tb = pp.PrepareTensorBatch(srcs, t, None, [place] * n)
                t_surf = t_tens = 1e9
                for _ in range(3):
                    t_surf = min(t_surf, timed(pp.Stream, lambda: pp.RunRoiBatchAsync(roi, pad, cc)))
                    t_tens = min(t_tens, timed(pp.Stream, lambda: pp.RunTensorBatchAsync(tb, pad, cc)))
                gbs = (read + elems * esize) / (t_tens * 1e-3) / 1e9
                out.append({"config": f"{name} {sw}x{sh}->{dw}x{dh} b{n}", "dtype": str(dtype)[6:], "layout": layout,
                            "us": round(t_tens * 1e3, 2), "surfaces_f32_us": round(t_surf * 1e3, 2),
                            "speedup": round(t_surf / t_tens, 3), "GB_s": round(gbs, 1),
                            "frac_8TBs": round(gbs / PEAK_GBS, 3),
                            "surfaces_frac_8TBs": round((read + elems * 4) / (t_surf * 1e-3) / 1e9 / PEAK_GBS, 3)})
                print(json.dumps(out[-1]), flush=True)
                del tb, t
        del dsts, roi
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("".join(json.dumps(r) + "\n" for r in out))


if __name__ == "__main__":
    main()
