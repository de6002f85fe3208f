"""PyPoseDrawer on the GPU against tests/pose_model.py, bit for bit: the frames and the points.

The fixtures are those of tests/pose_cases.py (tests/test_pose_host.py checks on the CPU that every drawn row of them has
at least 3 visible keypoints and paints 1 to 60 % of its frame): two frames of 96 x 80 and 70 x 50 -- several tiles,
partial tiles, a ragged right edge -- four rows each, a letterbox and a zoomed crop."""
import numpy as np
import pytest

import annotate_model as am
import pose_cases as pc
import pose_model as po
import postproc_model as pm
from test_gpu_annotate import device_marks, download, make_frames

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ROWS_601 = "601_JPEG"
DT = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


@pytest.fixture(scope="module")
def pd(vali, gpu):
    return vali.PyPoseDrawer(gpu)


def to_device(host, dtype, gpu):
    t = torch.from_numpy(np.ascontiguousarray(host)).to(f"cuda:{gpu}").to(DT[dtype])
    assert np.array_equal(t.float().cpu().numpy(), host, equal_nan=True)       # the fixture is exact in its dtype
    return t


def head_slice(host, dtype, gpu):
    """the keypoints as the last 3 P channels of a YOLOv8-pose head (N, 4 + 1 + 3 P, K), transposed and unflattened
    without a copy"""
    n, k, p, c = host.shape
    assert c == 3
    pred = torch.full((n, 5 + 3 * p, k), 1e4, dtype=DT[dtype], device=f"cuda:{gpu}")
    pred[:, 5:] = to_device(host, dtype, gpu).reshape(n, k, 3 * p).transpose(1, 2)
    view = pred[:, 5:].transpose(1, 2).unflatten(2, (p, 3))
    assert not view.is_contiguous() and view.stride() == ((5 + 3 * p) * k, 1, 3 * k, k)
    assert view.data_ptr() == pred.data_ptr() + 5 * k * pred.element_size()
    return view


def compare(vali, gpu, surfs, hosts, what, sizes=pc.SIZES):
    for i, s in enumerate(surfs):
        got = download(vali, gpu, s)
        if not np.array_equal(got, hosts[i]):
            bad = np.flatnonzero(got != hosts[i])
            raise AssertionError(f"{what} frame {i} {sizes[i]}: {bad.size} bytes differ, first at {bad[:6]}: "
                                 f"got {got[bad[:6]]}, want {hosts[i][bad[:6]]}")


def check(vali, gpu, pd, fmt, dets, kpts=None, dtype="float32", limbs=pc.LIMBS, alpha=None, rects=pc.RECTS, thr=pc.THR,
          thickness=3, diameter=7, head=False, expand=False, seed=0, dev_args=False, given_points=True):
    """draw `dets` on fresh noise frames and compare every frame and the points with the model; returns the model's
    (points, drawn)"""
    kpts = pc.kpts(pc.P, dtype) if kpts is None else kpts
    n, p = len(pc.SIZES), kpts.shape[2]
    if expand:
        kt = to_device(kpts[:1], dtype, gpu).expand(n, -1, -1, -1)
        assert kt.stride(0) == 0
        kpts = np.repeat(kpts[:1], n, 0)
    else:
        kt = head_slice(kpts, dtype, gpu) if head else to_device(kpts, dtype, gpu)
    surfs, hosts = make_frames(vali, gpu, fmt, pc.SIZES, seed)
    points = None
    if given_points:
        points = torch.full((n * pc.D, p, 4), -7, dtype=torch.int32, device=f"cuda:{gpu}")
    pb = pd.Prepare(surfs, kt, device_marks(dets, gpu), max_det=pc.D, limbs=limbs, points=points)
    assert pb.ws_bytes == n * pc.D * (1 + p) * 16
    r, lc, jc = rects, pc.LIMB_COLOURS, pc.JOINT_COLOURS
    if dev_args:
        r = torch.tensor(np.asarray(rects, np.int32), dtype=torch.int32, device=f"cuda:{gpu}")
        lc = torch.tensor(np.asarray(lc, np.int32), dtype=torch.int32, device=f"cuda:{gpu}")
        jc = torch.tensor(np.asarray(jc, np.int32), dtype=torch.int32, device=f"cuda:{gpu}")
        torch.cuda.synchronize()
    ok, info = pd.Run(pb, r, lc, jc, kpt_thr=thr, thickness=thickness, diameter=diameter, alpha=alpha,
                      cc_ctx=pm.cc_ctx_of(vali, ROWS_601))
    assert ok and info == vali.TaskExecInfo.SUCCESS, info
    want, drawn = po.apply(hosts, fmt, pc.SIZES, dets, pc.D, kpts, rects, limbs, pc.LIMB_COLOURS, pc.JOINT_COLOURS, thr,
                           thickness, diameter, alpha, pm.matrices()[ROWS_601])
    if given_points:
        got = points.cpu().numpy()
        assert np.array_equal(got, want), (fmt, dtype, np.argwhere(got != want)[:6])
    compare(vali, gpu, surfs, hosts, (fmt, dtype, thickness, diameter, alpha))
    return want, drawn


# ---- formats, records, dtypes, layouts --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", am.FORMATS)
def test_every_format_on_both_records(vali, gpu, pd, fmt):
    points, drawn = check(vali, gpu, pd, fmt, pc.PLACEMENTS)
    assert {d[0] for d in drawn} == set(range(8)) and {d[2] for d in drawn} == {0, 1}


@pytest.mark.parametrize("dtype", list(DT))
@pytest.mark.parametrize("fmt", ["NV12", "RGB"])
def test_every_dtype(vali, gpu, pd, fmt, dtype):
    check(vali, gpu, pd, fmt, pc.PLACEMENTS, dtype=dtype, alpha=128, seed=1)


@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_a_transposed_unflattened_head_slice(vali, gpu, pd, dtype):
    check(vali, gpu, pd, "NV12", pc.PLACEMENTS, dtype=dtype, head=True, seed=2)
    check(vali, gpu, pd, "BGR", pc.PLACEMENTS, dtype=dtype, head=True, seed=2)


def test_keypoints_without_a_confidence(vali, gpu, pd):
    points, _ = check(vali, gpu, pd, "YUV420", pc.PLACEMENTS, kpts=pc.kpts(pc.P, kdim=2), seed=3)
    assert (points[:, :, 2] == 0x3F800000).all() and (points[:, :, 3] == 3).sum() >= 35
    check(vali, gpu, pd, "RGB", pc.PLACEMENTS, kpts=pc.kpts(pc.P, "float16", kdim=2), dtype="float16", seed=3)


def test_keypoints_expanded_with_stride_0(vali, gpu, pd):
    check(vali, gpu, pd, "RGB_PLANAR", pc.PLACEMENTS, expand=True, seed=4)
    check(vali, gpu, pd, "NV12", pc.PLACEMENTS, dtype="bfloat16", expand=True, seed=4)


def test_device_rects_and_colours(vali, gpu, pd):
    check(vali, gpu, pd, "NV12", pc.PLACEMENTS, dev_args=True, seed=5)
    check(vali, gpu, pd, "RGB_PLANAR", pc.PLACEMENTS, dev_args=True, alpha=255, seed=5)


# ---- widths, alphas -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 3, 64])
@pytest.mark.parametrize("fmt", ["NV12", "RGB"])
def test_thickness_and_diameter(vali, gpu, pd, fmt, width):
    check(vali, gpu, pd, fmt, pc.PLACEMENTS, thickness=width, diameter=3, seed=6)
    check(vali, gpu, pd, fmt, pc.PLACEMENTS, thickness=2, diameter=width, seed=6)


@pytest.mark.parametrize("alpha", [0, 1, 255, None])
def test_alphas(vali, gpu, pd, alpha):
    check(vali, gpu, pd, "YUV444", pc.PLACEMENTS, alpha=alpha, seed=7)
    check(vali, gpu, pd, "NV12", pc.PLACEMENTS, alpha=alpha, seed=7)


# ---- geometry -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", am.FORMATS)
def test_limbs_across_tile_corners(vali, gpu, pd, fmt):
    """PLACEMENTS[0] and [4] hold the limbs through (64, 64) and across x = 64 (tests/test_pose_host.py); alone on their
    frames, thick and thin"""
    dets = [pc.PLACEMENTS[0]] + [(-1, 0, 0, 0, 0, 0, 0, 0)] * 3 + [pc.PLACEMENTS[4]] + [(-1, 0, 0, 0, 0, 0, 0, 0)] * 3
    for t in (1, 9):
        points, drawn = check(vali, gpu, pd, fmt, dets, thickness=t, diameter=5, seed=8)
        assert {d[0] for d in drawn} == {0, 4}
        first = next(d for d in drawn if d[0] == 0 and d[1] == 0)[3]
        assert first[:64, :64].any() and first[64:, 64:].any() and first[64, 64]  # through the corner four tiles share


@pytest.mark.parametrize("fmt", ["NV12", "YUV420", "RGB"])
@pytest.mark.parametrize("t", [1, 3, 64])
def test_limbs_with_one_end_far_off_the_frame(vali, gpu, pd, fmt, t):
    """ends at -65536 and 131071 in x and in y, the limits of a visible keypoint; a keypoint one pixel beyond is invisible"""
    points, drawn = check(vali, gpu, pd, fmt, pc.PLACEMENTS, kpts=pc.far_kpts(), thickness=t, seed=9)
    assert points[0, 0, 0] == -65536 and points[1, 1, 0] == 131071 and points[2, 0, 1] == -65536 and points[3, 1, 1] == 131071
    assert (points[:4, 2] == [0, 0, 0x3F666666, 0]).all()
    for row, kp in ((0, 0), (1, 1), (2, 0), (3, 1)):
        far = [d for d in drawn if d[0] == row and d[1] < len(pc.LIMBS) and kp in pc.LIMBS[d[1]]]
        assert far and all(d[3].any() for d in far), row                         # the far limbs reach the frame


@pytest.mark.parametrize("fmt", ["NV12", "BGR"])
@pytest.mark.parametrize("dtype", list(DT))
def test_invisible_keypoints_by_threshold_nan_and_inf(vali, gpu, pd, fmt, dtype):
    points, drawn = check(vali, gpu, pd, fmt, pc.PLACEMENTS, kpts=pc.odd_kpts(dtype), dtype=dtype, seed=10)
    assert ((points[:, :, 3] != 0).sum(1) == 2).all()
    assert {d[0] for d in drawn} == set(range(8)) and len(drawn) == 8 * 3
    points, drawn = check(vali, gpu, pd, fmt, pc.PLACEMENTS, dtype=dtype, thr=0.8, seed=10)
    assert 0 < (points[:, :, 3] != 0).sum() < 30
    points, drawn = check(vali, gpu, pd, fmt, pc.PLACEMENTS, dtype=dtype, thr=float("inf"), seed=10)
    assert not drawn and not points[:, :, [0, 1, 3]].any()


# ---- rows that must be skipped --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", am.FORMATS)
def test_skipped_rows(vali, gpu, pd, fmt):
    """frame -1, the frame field of another slot, k = K, k = -1, w = 0, int32 extremes that miss and that meet the frame"""
    points, drawn = check(vali, gpu, pd, fmt, pc.SKIPS, seed=11)
    assert {d[0] for d in drawn} == pc.SKIPS_PAINTED
    for idx in range(8):
        assert points[idx].any() == (idx in pc.SKIPS_PAINTED)


@pytest.mark.parametrize("fmt", ["NV12", "RGB"])
def test_a_record_with_dst_w_0_leaves_its_frame_alone(vali, gpu, pd, fmt):
    points, drawn = check(vali, gpu, pd, fmt, pc.PLACEMENTS, rects=pc.RECTS_DST_W_0, seed=12)
    assert {d[0] for d in drawn} == {0, 1, 2, 3} and not points[4:].any()


# ---- the sizes of the tables ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["NV12", "RGB"])
def test_no_limbs_one_keypoint_64_keypoints(vali, gpu, pd, fmt):
    points, drawn = check(vali, gpu, pd, fmt, pc.PLACEMENTS, limbs=(), seed=13)
    assert drawn and all(d[1] < pc.P for d in drawn)
    points, drawn = check(vali, gpu, pd, fmt, pc.PLACEMENTS, kpts=pc.kpts(1), limbs=((0, 0),), seed=13)
    assert len(drawn) == 16
    rng = np.random.default_rng(14)
    limbs = tuple((int(a), int(b)) for a, b in rng.integers(0, 64, (128, 2)))
    points, drawn = check(vali, gpu, pd, fmt, pc.PLACEMENTS, kpts=pc.kpts(64), limbs=limbs, thickness=1, diameter=2, seed=13)
    assert len(drawn) > 8 * 150


def test_points_in_the_workspace(vali, gpu, pd):
    check(vali, gpu, pd, "NV12", pc.PLACEMENTS, given_points=False, seed=15)
    check(vali, gpu, pd, "RGB", pc.SKIPS, given_points=False, seed=15)


# ---- the annotator gives the same bytes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", am.FORMATS)
def test_the_annotator_stamps_the_same_bytes_from_the_models_atlas(vali, gpu, pd, fmt):
    kpts = pc.kpts()
    a, hosts = make_frames(vali, gpu, fmt, pc.SIZES, seed=16)
    b, _ = make_frames(vali, gpu, fmt, pc.SIZES, seed=16)
    pb = pd.Prepare(a, to_device(kpts, "float32", gpu), device_marks(pc.PLACEMENTS, gpu), max_det=pc.D, limbs=pc.LIMBS)
    assert pd.Run(pb, pc.RECTS, pc.LIMB_COLOURS, pc.JOINT_COLOURS, cc_ctx=pm.cc_ctx_of(vali, ROWS_601))[0]
    _, drawn = po.apply(hosts, fmt, pc.SIZES, pc.PLACEMENTS, pc.D, kpts, pc.RECTS, pc.LIMBS, pc.LIMB_COLOURS,
                        pc.JOINT_COLOURS, rows=pm.matrices()[ROWS_601])
    atlas, marks = po.stamp_atlas(drawn)
    at = torch.from_numpy(atlas).to(f"cuda:{gpu}")
    torch.cuda.synchronize()
    ann = vali.PySurfaceAnnotator(gpu)
    assert ann.RunBatch(ann.PrepareBatch(b), device_marks(marks, gpu), pm.cc_ctx_of(vali, ROWS_601),
                        atlas=vali.Surface.from_dlpack(at, vali.Y))[0]
    for i, (sa, sb) in enumerate(zip(a, b)):
        got = download(vali, gpu, sa)
        assert np.array_equal(got, download(vali, gpu, sb)) and np.array_equal(got, hosts[i]), (fmt, i)


# ---- nothing else is written ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", am.FORMATS)
def test_pitched_frames_keep_their_padding_and_a_frame_without_shapes_its_bytes(vali, gpu, pd, fmt):
    from vali_amd._native import shim

    kpts = pc.kpts()
    surfs = [vali.Surface.Make(getattr(vali, fmt), w, h, gpu) for w, h in pc.SIZES]
    stream = pd.Stream
    for s in surfs:
        for p in s._planes:
            shim.memset2d_async(gpu, p.GpuMem, p.Pitch, 0x5A, p.Pitch, p.Height, stream)
    shim.stream_sync(gpu, stream)
    hosts = pc.noise_frames(fmt, seed=17)
    for s, host in zip(surfs, hosts):
        assert vali.PyFrameUploader(gpu).Run(host, s)[0]
    dets = list(pc.PLACEMENTS[:4]) + [(-1, 0, 0, 0, 0, 0, 0, 0)] * 4            # frame 1 has no detection
    pb = pd.Prepare(surfs, to_device(kpts, "float32", gpu), device_marks(dets, gpu), max_det=pc.D, limbs=pc.LIMBS)
    assert pd.Run(pb, pc.RECTS, pc.LIMB_COLOURS, pc.JOINT_COLOURS, alpha=200, cc_ctx=pm.cc_ctx_of(vali, ROWS_601))[0]
    untouched = hosts[1].copy()
    po.apply(hosts, fmt, pc.SIZES, dets, pc.D, kpts, pc.RECTS, pc.LIMBS, pc.LIMB_COLOURS, pc.JOINT_COLOURS, alpha=200,
             rows=pm.matrices()[ROWS_601])
    assert np.array_equal(hosts[1], untouched)
    compare(vali, gpu, surfs, hosts, fmt)
    for i, s in enumerate(surfs):
        for p in s._planes:
            raw = np.zeros((p.Height, p.Pitch), np.uint8)
            hp, _, _ = shim.buffer_info(raw, True)
            shim.memcpy2d_async(gpu, hp, p.Pitch, p.GpuMem, p.Pitch, p.Pitch, p.Height, 1, stream)
            shim.stream_sync(gpu, stream)
            used = p.Width * p.ElemSize
            assert p.Pitch > used
            assert (raw[:, used:] == 0x5A).all(), i


@pytest.mark.parametrize("fmt", ["NV12", "RGB", "BGR", "RGB_PLANAR"])
def test_frames_at_odd_addresses_and_the_canary_around_them(vali, gpu, pd, fmt):
    kpts = pc.kpts()
    kt = to_device(kpts, "float32", gpu)
    dets = device_marks(pc.PLACEMENTS, gpu)
    for x0, extra in ((3, 9), (1, 1)):
        bufs, views, hosts = [], [], pc.noise_frames(fmt, seed=18)
        for i, (w, h) in enumerate(pc.SIZES):
            (prows, cols), = am.plane_shapes(fmt, w, h)
            pitch = (cols + x0 + extra) | 1
            buf = torch.full((prows + 4, pitch), 0xA5, dtype=torch.uint8, device=f"cuda:{gpu}")
            buf[2:2 + prows, x0:x0 + cols] = torch.from_numpy(hosts[i].reshape(prows, cols)).to(buf.device)
            bufs.append(buf)
            views.append(buf[2:2 + prows, x0:x0 + cols])
        torch.cuda.synchronize()
        surfs = [vali.Surface.from_dlpack(v, getattr(vali, fmt)) for v in views]
        assert surfs[0].PixelPtr(0) % 2 == 1 and surfs[0].Pitch % 16
        pb = pd.Prepare(surfs, kt, dets, max_det=pc.D, limbs=pc.LIMBS)
        assert pd.Run(pb, pc.RECTS, pc.LIMB_COLOURS, pc.JOINT_COLOURS, thickness=5, cc_ctx=pm.cc_ctx_of(vali, ROWS_601))[0]
        po.apply(hosts, fmt, pc.SIZES, pc.PLACEMENTS, pc.D, kpts, pc.RECTS, pc.LIMBS, pc.LIMB_COLOURS, pc.JOINT_COLOURS,
                 thickness=5, rows=pm.matrices()[ROWS_601])
        for i, (w, h) in enumerate(pc.SIZES):
            (prows, cols), = am.plane_shapes(fmt, w, h)
            buf = bufs[i].cpu().numpy()
            assert np.array_equal(buf[2:2 + prows, x0:x0 + cols].reshape(-1), hosts[i]), (x0, i)
            buf[2:2 + prows, x0:x0 + cols] = 0xA5
            assert (buf == 0xA5).all(), (x0, i, np.argwhere(buf != 0xA5)[:4])


# ---- capture ----------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay_after_everything_was_rewritten_in_place(vali, gpu):
    from vali_amd._native import shim

    fmt, dev = "NV12", f"cuda:{gpu}"
    stream = shim.stream_create(gpu)
    pd = vali.PyPoseDrawer(gpu, stream)
    sets = [(pc.PLACEMENTS, pc.kpts(seed=0), pc.RECTS), (pc.SKIPS, pc.kpts(seed=1), pc.RECTS),
            (list(reversed(pc.PLACEMENTS[:4])) + list(pc.PLACEMENTS[4:]), pc.kpts(seed=2), [pc.RECTS[0], (0, 0, 70, 50, 0, 9, 64, 46)])]
    kt = to_device(sets[0][1], "float32", gpu)
    dets = device_marks(sets[0][0], gpu)
    rects = torch.tensor(np.asarray(pc.RECTS, np.int32), dtype=torch.int32, device=dev)
    lc = torch.tensor(np.asarray(pc.LIMB_COLOURS, np.int32), dtype=torch.int32, device=dev)
    jc = torch.tensor(np.asarray(pc.JOINT_COLOURS, np.int32), dtype=torch.int32, device=dev)
    points = torch.zeros((2 * pc.D, pc.P, 4), dtype=torch.int32, device=dev)
    surfs, _ = make_frames(vali, gpu, fmt, pc.SIZES, seed=19)
    torch.cuda.synchronize()
    pb = pd.Prepare(surfs, kt, dets, max_det=pc.D, limbs=pc.LIMBS, points=points)
    cap = vali.StreamCapture(stream, gpu)
    with cap:
        assert pd.RunAsync(pb, rects, lc, jc, alpha=128)[0]
    cap.Keep(pb)
    for k, (rows, kpts, recs) in enumerate(sets):
        hosts = pc.noise_frames(fmt, seed=20 + k)
        for s, host in zip(surfs, hosts):
            assert vali.PyFrameUploader(gpu).Run(host, s)[0]
        dets.copy_(device_marks(rows, gpu))                       # rewritten in place
        kt.copy_(to_device(kpts, "float32", gpu))
        rects.copy_(torch.tensor(np.asarray(recs, np.int32), dtype=torch.int32, device=dev))
        torch.cuda.synchronize()
        cap.Launch()
        shim.stream_sync(gpu, stream)
        want, _ = po.apply(hosts, fmt, pc.SIZES, rows, pc.D, kpts, recs, pc.LIMBS, pc.LIMB_COLOURS, pc.JOINT_COLOURS,
                           alpha=128, rows=pm.matrices()[ROWS_601])
        compare(vali, gpu, surfs, hosts, ("replay", k))
        assert np.array_equal(points.cpu().numpy(), want), k


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_prepare_and_run_say_what_is_wrong(vali, gpu, pd):
    kt = to_device(pc.kpts(), "float32", gpu)
    dets = device_marks(pc.PLACEMENTS, gpu)
    surfs, _ = make_frames(vali, gpu, "NV12", pc.SIZES, seed=21)
    kw = dict(max_det=pc.D, limbs=pc.LIMBS)
    with pytest.raises(ValueError, match="4-D"):
        pd.Prepare(surfs, kt[:, :, :, 0], dets, **kw)
    with pytest.raises(ValueError, match="last dimension"):
        pd.Prepare(surfs, kt[:, :, :, :1], dets, **kw)
    with pytest.raises(ValueError, match="dets"):
        pd.Prepare(surfs, kt, dets[:7], **kw)
    with pytest.raises(ValueError, match="3 surfaces"):
        pd.Prepare(surfs + surfs[:1], kt, dets, **kw)
    with pytest.raises(ValueError, match="dtype"):
        pd.Prepare(surfs, kt.double(), dets, **kw)
    with pytest.raises(ValueError, match="GPU"):
        pd.Prepare(surfs, kt.cpu(), dets, **kw)
    with pytest.raises(ValueError, match="pair 1"):
        pd.Prepare(surfs, kt, dets, max_det=pc.D, limbs=[(0, 1), (2, 5)])
    with pytest.raises(ValueError, match="points"):
        pd.Prepare(surfs, kt, dets, points=torch.zeros((8, 5, 3), dtype=torch.int32, device=kt.device), **kw)
    with pytest.raises(ValueError, match="points"):
        pd.Prepare(surfs, kt, dets, points=torch.zeros((8, 5, 4), dtype=torch.float32, device=kt.device), **kw)
    mixed = [surfs[0], vali.Surface.Make(vali.RGB, 70, 50, gpu)]
    with pytest.raises(ValueError, match="one format per batch"):
        pd.Prepare(mixed, kt, dets, **kw)
    pb = pd.Prepare(surfs, kt, dets, **kw)
    with pytest.raises(ValueError, match="rects"):
        pd.Run(pb, pc.RECTS[:1], pc.LIMB_COLOURS, pc.JOINT_COLOURS)
    with pytest.raises(ValueError, match="alpha"):
        pd.Run(pb, pc.RECTS, pc.LIMB_COLOURS, pc.JOINT_COLOURS, alpha=300)
    with pytest.raises(ValueError, match="thickness"):
        pd.Run(pb, pc.RECTS, pc.LIMB_COLOURS, pc.JOINT_COLOURS, thickness=65)
    with pytest.raises(ValueError, match="joint_colours"):
        pd.Run(pb, pc.RECTS, pc.LIMB_COLOURS, [])
    with pytest.raises(ValueError, match="PoseBatch"):
        pd.Run(None, pc.RECTS, pc.LIMB_COLOURS, pc.JOINT_COLOURS)
