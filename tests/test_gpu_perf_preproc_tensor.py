"""Cliff guard of the tensor path (not a tight floor): 16 NV12 1080p frames letterboxed to 640 x 640 (the case of
profiles/preproc_roi.md), in one process, alternating three times and keeping the minimum of each side.  The float16
planar tensor writes half the bytes of the RGB_32F_PLANAR surfaces of RunRoiBatch and must not be slower: at most 1.25 x
its time, the margin tests/test_gpu_perf_roi.py gives two forms that should keep up with each other.  The other dtypes
and layouts are timed and printed (run with -s), not bounded."""
import numpy as np
import pytest

from test_gpu_perf_roi import _alternate, _sources, _timed

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
N, SW, SH, DW, DH = 16, 1920, 1080, 640, 640
HBM = 8e12      # bytes per second


def test_float16_tensor_keeps_up_with_float32_surfaces(vali, gpu):
    import torch

    srcs = _sources(vali, gpu, SW, SH, N)
    place = [vali.letterbox_rect(SW, SH, DW, DH)] * N
    dsts = [vali.Surface.Make(vali.RGB_32F_PLANAR, DW, DH, gpu) for _ in range(N)]
    cc = vali.ColorspaceConversionContext(vali.ColorSpace.BT_709, vali.ColorRange.MPEG)
    pp = vali.PySurfacePreprocessor(gpu, mean=MEAN, std=STD, div=255.0)
    pad = (114, 114, 114)
    roi = pp.PrepareRoiBatch(srcs, dsts, None, place)

    def surfaces():
        pp.RunRoiBatchAsync(roi, pad, cc)

    def tensor_run(dtype, layout):
        out = torch.empty((N, 3, DH, DW), dtype=dtype, device=f"cuda:{gpu}")
        if layout == "packed":
            out = out.contiguous(memory_format=torch.channels_last)
        torch.cuda.synchronize()
        tb = pp.PrepareTensorBatch(srcs, out, None, place)
        return lambda: pp.RunTensorBatchAsync(tb, pad, cc)

    f16 = tensor_run(torch.float16, "planar")
    assert f16() == (True, vali.TaskExecInfo.SUCCESS)
    t_f32, t_f16 = _alternate(gpu, pp.Stream, surfaces, f16)
    read = N * SW * SH * 3 // 2
    px = N * 3 * DW * DH

    def line(name, ms, esize):
        print(f"  {name:28s} {ms * 1e3:8.1f} us  {t_f32 / ms:5.2f} x the f32 surfaces  "
              f"{(read + px * esize) / (ms * 1e-3) / HBM:5.3f} of 8 TB/s")

    print()
    line("RGB_32F_PLANAR surfaces", t_f32, 4)
    line("float16 planar tensor", t_f16, 2)
    for dtype, esize in ((torch.float32, 4), (torch.float16, 2), (torch.bfloat16, 2)):
        for layout in ("planar", "packed"):
            if (dtype, layout) == (torch.float16, "planar"):
                continue
            fn = tensor_run(dtype, layout)
            ms = min(_timed(gpu, pp.Stream, fn) for _ in range(3))
            line(f"{str(dtype)[6:]} {layout} tensor", ms, esize)
    assert t_f16 <= 1.25 * t_f32, f"float16 tensor {t_f16 * 1e3:.1f} us vs float32 surfaces {t_f32 * 1e3:.1f} us"
