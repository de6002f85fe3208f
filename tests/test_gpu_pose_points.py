"""PyPoseDrawer.RunPoints (vali_pose_paint_points) on the GPU: the points an earlier Run wrote, drawn again on an untouched
copy of the frames, give the same bytes; caller-made points of every flag and every int32 value draw what
tests/kpt_decode_model.py (paint_points: pose_model's shapes, coverage and blend) draws; nothing else is written."""
import numpy as np
import pytest

import annotate_model as am
import kpt_decode_model as kd
import pose_cases as pc
import postproc_model as pm
from test_gpu_annotate import download, make_frames

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ROWS_601 = "601_JPEG"
SIZES = [(66, 34), (130, 70)]          # more than one tile, partial tiles, a ragged right edge
D, K, P = 4, 12, 5
RECTS = [(0, 0, w, h, 0, 0, w, h) for w, h in SIZES]         # network coordinates are frame pixels
DETS = [(i, 0, 0, w, h, 0, 0, (3 * r + 5 * i) % K) for i, (w, h) in enumerate(SIZES) for r in range(D)]


@pytest.fixture(scope="module")
def pd(vali, gpu):
    return vali.PyPoseDrawer(gpu)


def dev_i32(a, gpu):
    t = torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(f"cuda:{gpu}")
    torch.cuda.synchronize()
    return t


def same(vali, gpu, surfs, hosts, what):
    for i, s in enumerate(surfs):
        got = download(vali, gpu, s)
        if not np.array_equal(got, hosts[i]):
            bad = np.flatnonzero(got != hosts[i])
            raise AssertionError(f"{what} frame {i}: {bad.size} bytes differ, first at {bad[:6]}")


def offset_views(vali, gpu, fmt, hosts, x0=3, extra=9):
    """the frames as views of canary-filled buffers, at odd addresses and pitches; returns (surfaces, buffers)"""
    bufs, views = [], []
    for i, (w, h) in enumerate(SIZES):
        (prows, cols), = am.plane_shapes(fmt, w, h)
        pitch = (cols + x0 + extra) | 1
        buf = torch.full((prows + 4, pitch), 0xA5, dtype=torch.uint8, device=f"cuda:{gpu}")
        buf[2:2 + prows, x0:x0 + cols] = torch.from_numpy(hosts[i].reshape(prows, cols)).to(buf.device)
        bufs.append(buf)
        views.append(buf[2:2 + prows, x0:x0 + cols])
    torch.cuda.synchronize()
    return [vali.Surface.from_dlpack(v, getattr(vali, fmt)) for v in views], bufs


# ---- (a) the points of Run, drawn again -------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", am.FORMATS)
def test_run_points_repeats_run_on_an_untouched_copy(vali, gpu, pd, fmt):
    cc = pm.cc_ctx_of(vali, ROWS_601)
    kpts = torch.from_numpy(pc.kpts(P, "float32", seed=1, n=2, k=K, sizes=SIZES, rects=RECTS)).to(f"cuda:{gpu}")
    dets = dev_i32(DETS, gpu)
    a, hosts = make_frames(vali, gpu, fmt, SIZES, seed=40)
    b, _ = make_frames(vali, gpu, fmt, SIZES, seed=40)
    pts = torch.zeros((len(SIZES) * D, P, 4), dtype=torch.int32, device=f"cuda:{gpu}")
    pb = pd.Prepare(a, kpts, dets, max_det=D, limbs=pc.LIMBS, points=pts)
    assert pd.Run(pb, RECTS, pc.LIMB_COLOURS, pc.JOINT_COLOURS, kpt_thr=pc.THR, thickness=3, diameter=7, alpha=160, cc_ctx=cc)[0]
    drawn = [download(vali, gpu, s) for s in a]
    assert (pts[..., 3] != 0).sum() > 20 and not all(np.array_equal(d, h) for d, h in zip(drawn, hosts))
    qb = pd.PreparePoints(b, pts, max_det=D, limbs=pc.LIMBS)
    ok, info = pd.RunPoints(qb, pc.LIMB_COLOURS, pc.JOINT_COLOURS, thickness=3, diameter=7, alpha=160, cc_ctx=cc)
    assert ok and info == vali.TaskExecInfo.SUCCESS, info
    same(vali, gpu, b, drawn, fmt)
    # ... and the model agrees with both
    kd.paint_points(hosts, fmt, SIZES, pts.cpu().numpy(), D, pc.LIMBS, pc.LIMB_COLOURS, pc.JOINT_COLOURS, 3, 7, 160,
                    pm.matrices()[ROWS_601])
    same(vali, gpu, b, hosts, (fmt, "model"))


@pytest.mark.parametrize("fmt", ["NV12", "RGB", "BGR", "RGB_PLANAR"])
def test_offset_and_pitched_views_and_the_canary_around_them(vali, gpu, pd, fmt):
    cc = pm.cc_ctx_of(vali, ROWS_601)
    kpts = torch.from_numpy(pc.kpts(P, "float32", seed=2, n=2, k=K, sizes=SIZES, rects=RECTS)).to(f"cuda:{gpu}")
    hosts = [am.noise_frame(fmt, w, h, 4100 + i) for i, (w, h) in enumerate(SIZES)]
    a, _ = offset_views(vali, gpu, fmt, hosts)
    b, bufs = offset_views(vali, gpu, fmt, hosts, x0=1, extra=1)
    assert b[0].PixelPtr(0) % 2 == 1 and b[0].Pitch % 16
    pts = torch.zeros((len(SIZES) * D, P, 4), dtype=torch.int32, device=f"cuda:{gpu}")
    pb = pd.Prepare(a, kpts, dev_i32(DETS, gpu), max_det=D, limbs=pc.LIMBS, points=pts)
    assert pd.Run(pb, RECTS, pc.LIMB_COLOURS, pc.JOINT_COLOURS, kpt_thr=pc.THR, thickness=4, diameter=9, cc_ctx=cc)[0]
    qb = pd.PreparePoints(b, pts, max_det=D, limbs=pc.LIMBS)
    assert pd.RunPoints(qb, pc.LIMB_COLOURS, pc.JOINT_COLOURS, thickness=4, diameter=9, cc_ctx=cc)[0]
    same(vali, gpu, b, [download(vali, gpu, s) for s in a], fmt)
    kd.paint_points(hosts, fmt, SIZES, pts.cpu().numpy(), D, pc.LIMBS, pc.LIMB_COLOURS, pc.JOINT_COLOURS, 4, 9, None,
                    pm.matrices()[ROWS_601])
    for i, (w, h) in enumerate(SIZES):
        (prows, cols), = am.plane_shapes(fmt, w, h)
        buf = bufs[i].cpu().numpy()
        assert np.array_equal(buf[2:2 + prows, 1:1 + cols].reshape(-1), hosts[i]), i
        buf[2:2 + prows, 1:1 + cols] = 0xA5
        assert (buf == 0xA5).all(), (i, np.argwhere(buf != 0xA5)[:4])


# ---- (b) caller-made points -------------------------------------------------------------------------------------------------
def hostile_points(seed):
    """(N * D, P, 4) with P = 8: every flag 0..7 on points inside the frames, coordinates at the ends of the visible range
    and one beyond, and random int32 rows"""
    rng = np.random.default_rng(seed)
    p = 8
    pts = np.zeros((len(SIZES) * D, p, 4), np.int64)
    for r in range(pts.shape[0]):
        w, h = SIZES[r // D]
        pts[r, :, 0], pts[r, :, 1] = rng.integers(2, w - 2, p), rng.integers(2, h - 2, p)
        pts[r, :, 2] = rng.integers(-(1 << 31), 1 << 31, p)
        pts[r, :, 3] = (np.arange(p) + r) % 8                   # every flag on every keypoint index over the rows
    lo, hi = -65536, 131071
    pts[1, 0], pts[1, 1] = (lo, 10, 0, 1), (30, 12, 0, 1)       # a limb from the far left into the frame
    pts[1, 2], pts[1, 3] = (lo - 1, 10, 0, 1), (30, 20, 0, 3)   # one beyond: no limb, the joint at (30, 20) alone
    pts[2, 0], pts[2, 1] = (hi, hi, 0, 1), (20, 5, 0, 1)
    pts[2, 2], pts[2, 3] = (hi + 1, 5, 0, 1), (5, hi + 1, 0, 1)
    pts[5, 0], pts[5, 1] = (40, lo, 0, 1), (90, hi, 0, 5)       # from far above to far below
    pts[5, 2], pts[5, 3] = (40, lo - 1, 0, 1), ((1 << 31) - 1, -(1 << 31), 0, 1)
    pts[6] = rng.integers(-(1 << 31), 1 << 31, (p, 4))          # random int32 rows
    pts[7] = rng.integers(-(1 << 31), 1 << 31, (p, 4))
    pts[7, :, 3] |= 1
    return pts.astype(np.int32)


LIMBS8 = ((0, 1), (2, 3), (1, 3), (4, 5), (6, 7), (0, 7), (2, 5))


@pytest.mark.parametrize("fmt", ["NV12", "YUV444", "RGB"])
def test_caller_made_points_of_every_flag_and_value(vali, gpu, pd, fmt):
    cc = pm.cc_ctx_of(vali, ROWS_601)
    for seed, (t, dia, alpha) in enumerate(((3, 7, 160), (1, 1, None), (64, 64, 90))):
        host_pts = hostile_points(seed)
        surfs, hosts = make_frames(vali, gpu, fmt, SIZES, seed=50 + seed)
        qb = pd.PreparePoints(surfs, dev_i32(host_pts, gpu), max_det=D, limbs=LIMBS8)
        ok, info = pd.RunPoints(qb, pc.LIMB_COLOURS, pc.JOINT_COLOURS, thickness=t, diameter=dia, alpha=alpha, cc_ctx=cc)
        assert ok and info == vali.TaskExecInfo.SUCCESS, info
        n = kd.paint_points(hosts, fmt, SIZES, host_pts, D, LIMBS8, pc.LIMB_COLOURS, pc.JOINT_COLOURS, t, dia, alpha,
                            pm.matrices()[ROWS_601])
        assert n > 20
        same(vali, gpu, surfs, hosts, (fmt, t, dia))


# ---- (c) nothing else is written --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", am.FORMATS)
def test_padding_and_frames_without_visible_points_keep_their_bytes(vali, gpu, pd, fmt):
    from vali_amd._native import shim

    surfs = [vali.Surface.Make(getattr(vali, fmt), w, h, gpu) for w, h in SIZES]
    stream = pd.Stream
    for s in surfs:
        for p in s._planes:
            shim.memset2d_async(gpu, p.GpuMem, p.Pitch, 0x5A, p.Pitch, p.Height, stream)
    shim.stream_sync(gpu, stream)
    hosts = [am.noise_frame(fmt, w, h, 4200 + i) for i, (w, h) in enumerate(SIZES)]
    for s, host in zip(surfs, hosts):
        assert vali.PyFrameUploader(gpu).Run(host, s)[0]
    pts = hostile_points(3)
    pts[:D, :, 3] &= ~1                     # frame 0: no visible point
    untouched = hosts[0].copy()
    qb = pd.PreparePoints(surfs, dev_i32(pts, gpu), max_det=D, limbs=LIMBS8)
    assert pd.RunPoints(qb, pc.LIMB_COLOURS, pc.JOINT_COLOURS, thickness=5, diameter=11, alpha=200,
                        cc_ctx=pm.cc_ctx_of(vali, ROWS_601))[0]
    kd.paint_points(hosts, fmt, SIZES, pts, D, LIMBS8, pc.LIMB_COLOURS, pc.JOINT_COLOURS, 5, 11, 200, pm.matrices()[ROWS_601])
    assert np.array_equal(hosts[0], untouched) and not np.array_equal(hosts[1], am.noise_frame(fmt, *SIZES[1], 4201))
    same(vali, gpu, surfs, hosts, fmt)
    for i, s in enumerate(surfs):
        for p in s._planes:
            raw = np.zeros((p.Height, p.Pitch), np.uint8)
            hp, _, _ = shim.buffer_info(raw, True)
            shim.memcpy2d_async(gpu, hp, p.Pitch, p.GpuMem, p.Pitch, p.Pitch, p.Height, 1, stream)
            shim.stream_sync(gpu, stream)
            used = p.Width * p.ElemSize
            assert p.Pitch > used
            assert (raw[:, used:] == 0x5A).all(), i


def test_prepare_points_says_what_is_wrong(vali, gpu, pd):
    surfs = [vali.Surface.Make(vali.RGB, w, h, gpu) for w, h in SIZES]
    pts = torch.zeros((len(SIZES) * D, P, 4), dtype=torch.int32, device=f"cuda:{gpu}")
    for args, kw, word in (((surfs, pts), dict(), "max_det is required"), ((surfs, pts), dict(max_det=3), "rows"),
                           ((surfs, pts.float()), dict(max_det=D), "int32"), ((surfs, pts[..., :3]), dict(max_det=D), "shape"),
                           ((surfs, pts), dict(max_det=D, limbs=((0, P),)), "limbs"), ((surfs, None), dict(max_det=D), "points")):
        with pytest.raises(ValueError, match=word):
            pd.PreparePoints(*args, **{"limbs": pc.LIMBS, **kw})
    with pytest.raises(ValueError, match=r"limbs: pair 0 = \(15, 13\)"):
        pd.PreparePoints(surfs, pts, max_det=D)                 # COCO_SKELETON, the default, needs 17 keypoints
    with pytest.raises(ValueError, match="PointsBatch"):
        pd.RunPoints(None, pc.LIMB_COLOURS, pc.JOINT_COLOURS)
