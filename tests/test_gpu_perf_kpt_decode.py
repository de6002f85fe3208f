"""Speed of PyKeypointDecoder.RunAsync on a top-down pose batch: M = 512 crops (16 frames x max_det 32), P = 17 heatmaps
of 64 x 48 float16 each (53.5 MB), the matrices mapping, quarter refinement.

The yardstick is the torch chain a user writes today for the same rows, on the same stream in the same process: the
flattened max, % and //, the four neighbour gathers and their signs, the affine map, floor, the visibility flags and the
stack into an int32 (M, P, 4) tensor.  Each run lies between two events, the median of the runs after warm-up, the two
alternating (_medians of tests/test_gpu_perf_masks.py).  RunAsync may take at most 1.0 times the chain.
The test prints both times and the fraction of 8 TB/s the one read of the maps comes to.
Measured on an MI355X: RunAsync 28.2 us against 487.8 us for the chain, ratio 0.058; 1.90 TB/s, 23.7 % of 8 TB/s
(profiles/kpt_decode.md)."""
import numpy as np
import pytest

import kpt_decode_model as kd
from test_gpu_perf_masks import _medians

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

N, D, P, HH, WH = 16, 32, 17, 64, 48
M = N * D
CANVAS = (192, 256)
W, H = 1920, 1080
THR = 0.3


def torch_chain(heat, rows, sizes):
    """what a user of torch writes for vali_kpt_decode's steps 2 to 6 (align "centre"); sizes: (M, 2) float32 W, H"""
    m, p, hh, wh = heat.shape
    conf, idx = heat.flatten(2).max(2)
    xp, yp = idx % wh, idx // wh
    flat = heat.flatten(2)
    xl, xr = (xp - 1).clamp(0, wh - 1), (xp + 1).clamp(0, wh - 1)
    yu, yd = (yp - 1).clamp(0, hh - 1), (yp + 1).clamp(0, hh - 1)
    dx = flat.gather(2, (yp * wh + xr)[..., None])[..., 0].float() - flat.gather(2, (yp * wh + xl)[..., None])[..., 0].float()
    dy = flat.gather(2, (yd * wh + xp)[..., None])[..., 0].float() - flat.gather(2, (yu * wh + xp)[..., None])[..., 0].float()
    ox = torch.where((xp > 0) & (xp < wh - 1), torch.sign(dx) * 0.25, torch.zeros_like(dx))
    oy = torch.where((yp > 0) & (yp < hh - 1), torch.sign(dy) * 0.25, torch.zeros_like(dy))
    cu = (xp.float() + 0.5 + ox) * (CANVAS[0] / wh)
    cv = (yp.float() + 0.5 + oy) * (CANVAS[1] / hh)
    co = rows[:, 1:7].view(torch.float32)[:, None, :]
    fx = co[..., 0] * cu + co[..., 1] * cv + co[..., 2]
    fy = co[..., 3] * cu + co[..., 4] * cv + co[..., 5]
    conf = conf.float()
    vis = (conf > THR) & (fx >= -65536) & (fx < 131072) & (fy >= -65536) & (fy < 131072)
    X, Y = torch.floor(fx).int() * vis, torch.floor(fy).int() * vis
    inside = vis & (X >= 0) & (X < sizes[:, None, 0]) & (Y >= 0) & (Y < sizes[:, None, 1])
    flag = vis.int() + 2 * inside.int()
    return torch.stack([X, Y, conf.view(torch.int32), flag], 2)


def test_run_is_no_slower_than_the_torch_chain(vali, gpu):
    torch.cuda.set_device(gpu)
    dev = f"cuda:{gpu}"
    stream = torch.cuda.current_stream(gpu).cuda_stream          # torch's work and ours on one stream
    rng = np.random.default_rng(1)
    # a Gaussian in noise per map: unique maxima, so that the chain's max and the decoder's tie rule agree
    cx, cy = rng.uniform(2, WH - 2, (M, P)).astype(np.float32), rng.uniform(2, HH - 2, (M, P)).astype(np.float32)
    x, y = np.arange(WH, dtype=np.float32) + 0.5, np.arange(HH, dtype=np.float32) + 0.5
    host = np.exp(-((x[None, None, None, :] - cx[..., None, None]) ** 2 + (y[None, None, :, None] - cy[..., None, None]) ** 2) / 8)
    host = (host * rng.uniform(0.1, 1.0, (M, P, 1, 1)).astype(np.float32)
            + rng.random(host.shape, dtype=np.float32) * np.float32(0.02)).astype(np.float16)
    heat = torch.from_numpy(host).to(dev)
    s, th = rng.uniform(0.5, 3.0, M), rng.uniform(0, 2 * np.pi, M)
    mats = np.stack([s * np.cos(th), -s * np.sin(th), rng.uniform(0, W, M), s * np.sin(th), s * np.cos(th),
                     rng.uniform(0, H, M)], 1)
    hrows = kd.matrix_rows(np.arange(M) // D, mats)
    rows = torch.from_numpy(hrows).to(dev)
    sizes = torch.tensor([[W, H]] * M, dtype=torch.float32, device=dev)
    points = torch.zeros((M, P, 4), dtype=torch.int32, device=dev)
    frames = [vali.Surface.Make(vali.NV12, W, H, gpu) for _ in range(N)]
    torch.cuda.synchronize()
    dec = vali.PyKeypointDecoder(gpu, stream)
    kb = dec.PrepareHeatmaps(frames, heat, points, canvas=CANVAS, matrices=rows)

    def ours():
        assert dec.RunAsync(kb, kpt_thr=THR, refine="quarter", align="centre")[0]

    out = []

    def chain():
        out[:] = [torch_chain(heat, rows, sizes)]

    ours()
    chain()
    torch.cuda.synchronize()
    got, ref = points.cpu().numpy(), out[0].cpu().numpy()
    want, _ = kd.decode([(W, H)] * N, hrows[:D], 0, CANVAS, heat=host[:D].astype(np.float32), thr=THR)
    assert np.array_equal(got[:D], want)
    # the chain does the same work: the same confidences, and the same rows but where float16 ties its max broke otherwise
    # or its fused arithmetic fell on the other side of a floor
    assert np.array_equal(got[..., 2], ref[..., 2]) and (got == ref).all(2).mean() > 0.98
    assert (got[..., 3] == 3).mean() > 0.3

    t_ours, t_chain = _medians([ours, chain])
    nbytes = heat.numel() * heat.element_size()
    print(f"\nkeypoint decode M = {M} ({N} x {D}), P = {P}, {HH} x {WH} float16, matrices, quarter: RunAsync "
          f"{t_ours * 1e3:.1f} us (1 launch), the torch chain {t_chain * 1e3:.1f} us, ratio {t_ours / t_chain:.3f}; "
          f"{nbytes / 1e6:.1f} MB read once: {nbytes / (t_ours * 1e-3) / 1e12:.2f} TB/s, "
          f"{nbytes / (t_ours * 1e-3) / 8e12:.1%} of 8 TB/s")
    assert t_ours <= 1.0 * t_chain, f"RunAsync {t_ours * 1e3:.1f} us vs the torch chain's {t_chain * 1e3:.1f} us"
