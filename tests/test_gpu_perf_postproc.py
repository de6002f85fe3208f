"""Speed of PySurfacePostprocessor on 16 x 1080p float16 planar -> NV12, against two things that are not the code under
test (in one process, alternating three times, the minimum of each side; tests/test_gpu_perf_roi.py's harness):

1. the chain it replaces, on the same data: torch quantise (seven elementwise launches), permute + contiguous, then per
   item Surface.from_dlpack, PySurfaceConverter RGB -> YUV420 and YUV420 -> NV12.  At most 0.5 of its time.  The bound is
   derived, not measured: the chain moves more than 50 bytes per tensor element against 2.5 (a factor of 20) in 2N + 8
   launches against one; the remaining factor of 10 is left to launch overheads at this batch size.
2. the mirror: PySurfacePreprocessor.RunTensorBatchAsync of 16 NV12 1080p frames onto a whole-canvas (16, 3, 1080, 1920)
   float16 tensor moves the same bytes the other way and does more arithmetic.  At most 1.25 times its time, the margin
   the sibling tests give two forms that should keep up with each other.
3. print only (-s): the time and the fraction of 8 TB/s for every dtype x layout x destination."""
import numpy as np
import pytest

from test_gpu_perf_roi import _alternate, _timed

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

N, W, H = 16, 1920, 1080
PEAK = 8e12                                     # bytes per second


def _tensor(gpu, dtype=torch.float16, channels_last=False):
    g = torch.Generator(device=f"cuda:{gpu}").manual_seed(5)
    if dtype == torch.uint8:
        t = torch.randint(0, 256, (N, 3, H, W), dtype=torch.uint8, device=f"cuda:{gpu}", generator=g)
    else:
        t = (torch.rand((N, 3, H, W), device=f"cuda:{gpu}", generator=g) * 1.4 - 0.2).to(dtype)
    if channels_last:
        t = t.contiguous(memory_format=torch.channels_last)
    torch.cuda.synchronize()
    return t


def test_faster_than_the_chain_it_replaces(vali, gpu):
    stream = torch.cuda.current_stream(gpu).cuda_stream         # torch's work and ours on one stream
    t = _tensor(gpu)
    post = vali.PySurfacePostprocessor(gpu, stream)
    cvt = vali.PySurfaceConverter(gpu, stream)
    outs = [vali.Surface.Make(vali.NV12, W, H, gpu) for _ in range(N)]
    mids = [vali.Surface.Make(vali.YUV420, W, H, gpu) for _ in range(N)]
    nvs = [vali.Surface.Make(vali.NV12, W, H, gpu) for _ in range(N)]
    fb = post.PrepareTensorBatch(t, outs)

    def chain():
        p = torch.nan_to_num(t.float() * 255.0 + 0.0, nan=0.0).round().clamp(0, 255).to(torch.uint8)
        p = p.permute(0, 2, 3, 1).contiguous()
        for i in range(N):
            rgb = vali.Surface.from_dlpack(p[i].view(H, 3 * W), vali.RGB)
            assert cvt.RunAsync(rgb, mids[i])[0]
            assert cvt.RunAsync(mids[i], nvs[i])[0]

    t_fused, t_chain = _alternate(gpu, stream, lambda: post.RunTensorBatchAsync(fb), chain)
    torch.cuda.synchronize()
    # the two wrote the same frames
    dn = vali.PySurfaceDownloader(gpu)
    a, b = np.zeros(outs[0].HostSize, np.uint8), np.zeros(nvs[0].HostSize, np.uint8)
    assert dn.Run(outs[N - 1], a)[0] and dn.Run(nvs[N - 1], b)[0]
    assert np.array_equal(a, b)
    print(f"\npostproc 16 x 1080p float16 -> NV12: fused {t_fused * 1e3:.1f} us, chain {t_chain * 1e3:.1f} us, "
          f"ratio {t_fused / t_chain:.3f}")
    assert t_fused <= 0.5 * t_chain, f"fused {t_fused * 1e3:.1f} us vs chain {t_chain * 1e3:.1f} us"


def test_keeps_up_with_the_mirror(vali, gpu):
    t = _tensor(gpu)
    post = vali.PySurfacePostprocessor(gpu)
    stream = post.Stream
    pre = vali.PySurfacePreprocessor(gpu, stream)
    outs = [vali.Surface.Make(vali.NV12, W, H, gpu) for _ in range(N)]
    fb = post.PrepareTensorBatch(t, outs)
    host = np.random.default_rng(1).integers(16, 236, W * H * 3 // 2, dtype=np.uint8)
    srcs = [vali.Surface.Make(vali.NV12, W, H, gpu) for _ in range(N)]
    for s in srcs:
        assert vali.PyFrameUploader(gpu).Run(host, s)[0]
    canvas = torch.empty((N, 3, H, W), dtype=torch.float16, device=f"cuda:{gpu}")
    torch.cuda.synchronize()
    tb = pre.PrepareTensorBatch(srcs, canvas)
    t_post, t_pre = _alternate(gpu, stream, lambda: post.RunTensorBatchAsync(fb), lambda: pre.RunTensorBatchAsync(tb))
    moved = N * W * H * (3 * 2 + 1.5)
    print(f"\npostproc 16 x 1080p float16 -> NV12: {t_post * 1e3:.1f} us ({moved / (t_post * 1e-3) / PEAK:.2f} of 8 TB/s); "
          f"preproc NV12 -> float16: {t_pre * 1e3:.1f} us ({moved / (t_pre * 1e-3) / PEAK:.2f}); ratio {t_post / t_pre:.3f}")
    assert t_post <= 1.25 * t_pre, f"postprocessor {t_post * 1e3:.1f} us vs preprocessor {t_pre * 1e3:.1f} us"


def test_print_every_form(vali, gpu):
    """no assertion on speed: the table of profiles/postproc_tensor.md (run with -s)"""
    post = vali.PySurfacePostprocessor(gpu)
    out_bytes = {"NV12": 1.5, "YUV420": 1.5, "YUV444": 3.0, "RGB": 3.0, "RGB_PLANAR": 3.0}
    print()
    for dtype, es in ((torch.float16, 2), (torch.bfloat16, 2), (torch.float32, 4), (torch.uint8, 1)):
        for cl in (False, True):
            t = _tensor(gpu, dtype, cl)
            for dst, ob in out_bytes.items():
                outs = [vali.Surface.Make(getattr(vali, dst), W, H, gpu) for _ in range(N)]
                fb = post.PrepareTensorBatch(t, outs)
                ms = _timed(gpu, post.Stream, lambda: post.RunTensorBatchAsync(fb))
                moved = N * W * H * (3 * es + ob)
                print(f"{str(dtype).split('.')[1]:9s} {'channels_last' if cl else 'planar':13s} {dst:10s} "
                      f"{ms * 1e3:8.1f} us  {moved / (ms * 1e-3) / PEAK:.2f} of 8 TB/s")
                assert ms > 0
                del fb, outs
            del t
