"""What RunTensor is for: a batch held as a tensor becomes JPEG files without the elementwise chain in front of `Run`.

Measured on the test's own machine, in one process, warm, as the median of 15 whole calls each:
  (a) RunTensor on the tensor;
  (b) the torch chain (scale, round, clamp, to uint8, to channels last), Surface.from_dlpack per item, Run;
  (c) Run on ready-made RGB_PLANAR surfaces of the same pixels -- not a contender, the ratio (a) / (c) is what reading
      2- or 4-byte elements costs the kernel.
(a) <= (b) is asserted for the float16 contiguous batch: (a) does strictly less work on the GPU and on the host.  No
margin beyond that.  The float32 channels-last figures are printed only.  profiles/jpeg_tensor.md keeps the figures."""
import statistics
import time
from pathlib import Path

import numpy as np
import pytest

PIL = pytest.importorskip("PIL.Image")
torch = pytest.importorskip("torch")

GOLDEN = Path(__file__).resolve().parent / "golden"
N, H, W = 8, 1080, 1920
CALLS = 15


def _picture():
    """the reference's frame tiled to 1920 x 1080, every item shifted: (N, H, W, 3) uint8"""
    frame = np.asarray(PIL.open(GOLDEN / "frame_0.jpg").convert("RGB"))
    fh, fw = frame.shape[:2]
    tiled = np.tile(frame, (-(-(H + 64) // fh), -(-(W + 64) // fw), 1))
    return np.stack([tiled[8 * i:8 * i + H, 8 * i:8 * i + W] for i in range(N)])


def _medians_ms(*fns):
    """the median time of a whole call of each function, the calls interleaved so that a drift of the machine meets all
    alike; two warm-up calls each"""
    for fn in fns:
        fn()
        fn()
    times = [[] for _ in fns]
    for _ in range(CALLS):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return tuple(statistics.median(t) for t in times)


def _measure(vali, gpu, dtype, channels_last):
    from torch.utils.dlpack import to_dlpack

    enc = vali.PyNvJpegEncoder(gpu, backend="hip")
    ctx = enc.Context(90, vali.RGB, subsampling="420")
    planar_ctx = enc.Context(90, vali.RGB_PLANAR, subsampling="420")
    u8 = torch.from_numpy(_picture()).to(f"cuda:{gpu}")                          # (N, H, W, 3)
    x = (u8.permute(0, 3, 1, 2).float() / 255).to(dtype)
    x = x.contiguous(memory_format=torch.channels_last) if channels_last else x.contiguous()
    torch.cuda.synchronize()

    def tensor_path():
        files, info = enc.RunTensor(ctx, x)
        assert info == vali.TaskExecInfo.SUCCESS
        return files

    def chain_path():
        q = (x.float() * 255).round().clamp(0, 255).to(torch.uint8)
        q = q.permute(0, 2, 3, 1).contiguous()
        torch.cuda.synchronize()                                                # the encoder works on its own stream
        surfs = [vali.Surface.from_dlpack(to_dlpack(q[i].view(H, 3 * W)), vali.RGB) for i in range(N)]
        files, info = enc.Run(ctx, surfs)
        assert info == vali.TaskExecInfo.SUCCESS
        return files

    p = (x.float() * 255).round().clamp(0, 255).to(torch.uint8).cpu().numpy()   # (N, 3, H, W)
    planar = []
    for i in range(N):
        s = vali.Surface.Make(vali.RGB_PLANAR, W, H, gpu)
        ok, info = vali.PyFrameUploader(gpu).Run(np.ascontiguousarray(p[i]).reshape(-1), s)
        assert ok, info
        planar.append(s)

    def surface_path():
        files, info = enc.Run(planar_ctx, planar)
        assert info == vali.TaskExecInfo.SUCCESS
        return files

    # the three paths write the same files
    a, b, c = tensor_path(), chain_path(), surface_path()
    for i in range(N):
        assert a[i].tobytes() == b[i].tobytes() == c[i].tobytes(), i
    return _medians_ms(tensor_path, chain_path, surface_path)


@pytest.mark.gpu
def test_run_tensor_is_no_slower_than_the_chain_it_replaces(vali, gpu):
    a, b, c = _measure(vali, gpu, torch.float16, channels_last=False)
    print(f"\njpeg_tensor float16 contiguous ({N}, 3, {H}, {W}) 4:2:0 q90: RunTensor {a:.2f} ms, torch chain + Run "
          f"{b:.2f} ms, Run on RGB_PLANAR surfaces {c:.2f} ms, (a)/(c) = {a / c:.3f}")
    assert a <= b, (a, b)


@pytest.mark.gpu
def test_float32_channels_last_figures(vali, gpu):
    a, b, c = _measure(vali, gpu, torch.float32, channels_last=True)
    print(f"\njpeg_tensor float32 channels last ({N}, 3, {H}, {W}) 4:2:0 q90: RunTensor {a:.2f} ms, torch chain + Run "
          f"{b:.2f} ms, Run on RGB_PLANAR surfaces {c:.2f} ms, (a)/(c) = {a / c:.3f}")
    assert a > 0 and b > 0 and c > 0
