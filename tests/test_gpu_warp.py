"""PySurfaceWarper on the GPU against tests/warp_model.py, bit for bit: the crops and the fitted matrices.

Frames are 64 x 48 and 50 x 38 (RGB family; odd sizes) and 64 x 48 and 34 x 26 (NV12); canvases 16 x 16, 7 x 5, 33 x 9 and
130 x 70, which is larger than a workgroup's tile both ways (16 lanes of 8 or 4 pixels, 16 rows)."""
import numpy as np
import pytest

import annotate_model as am
import mask_cases as mc
import pose_cases as pc
import warp_model as wm
from test_gpu_annotate import device_marks, make_frames

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

F32 = np.float32
DT = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
FORMATS = ["NV12", "RGB", "BGR", "RGB_PLANAR"]
CANVASES = [(16, 16), (7, 5), (33, 9), (130, 70)]
NORM = (2.0, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
CANARY = -7.0
I32_MIN = -(1 << 31)


def sizes_of(fmt):
    return [(64, 48), (34, 26)] if fmt == "NV12" else [(64, 48), (50, 38)]


def csc_of(vali, cc_ctx):
    from vali_amd import tasks

    return tasks._nv12_variant(cc_ctx)


def mpeg709(vali):
    return vali.ColorspaceConversionContext(vali.ColorSpace.BT_709, vali.ColorRange.MPEG)


def similarity(rng, W, H, w, h, lo=0.3, hi=2.5, spread=0.5):
    """a random similarity that takes the canvas centre to a point around the frame's centre: the crop hangs over the
    frame's edges in most draws"""
    s, th = rng.uniform(lo, hi) * min(W / w, H / h), rng.uniform(0, 2 * np.pi)
    a, d = s * np.cos(th), s * np.sin(th)
    cx, cy = W / 2 + rng.uniform(-spread, spread) * W / 2, H / 2 + rng.uniform(-spread, spread) * H / 2
    return [a, -d, cx - (a * w / 2 - d * h / 2), d, a, cy - (d * w / 2 + a * h / 2)]


def coverage_rows(sizes, canvas, seed):
    """six rows: both frames under random similarities, frame 0 again, an integer shift, a strong down-scale"""
    rng = np.random.default_rng(seed)
    w, h = canvas
    (W0, H0), (W1, H1) = sizes
    co = [similarity(rng, W0, H0, w, h), similarity(rng, W1, H1, w, h), similarity(rng, W0, H0, w, h, spread=1.0),
          [1, 0, 5, 0, 1, 3], similarity(rng, W1, H1, w, h, 2.6, 3.0, 0.1), similarity(rng, W1, H1, w, h, 0.2, 0.3)]
    return wm.pack_rows([0, 1, 0, 1, 1, 0], co, status=[9, -1, 0, 3, I32_MIN, 7])


def out_tensor(m, canvas, dtype, layout, gpu):
    """(big, out): `out` is the (m, 3, h, w) tensor the task writes, `big` the allocation around it, all canary.
    layouts: planar, packed (channels last), slice (guard bands on every side and between the items)"""
    w, h = canvas
    dev = f"cuda:{gpu}"
    if layout == "slice":
        big = torch.full((2 * m, 3, h + 2, w + 3), CANARY, dtype=DT[dtype], device=dev)
        return big, big[::2, :, 1:1 + h, 1:1 + w]
    big = torch.full((m, 3, h, w), CANARY, dtype=DT[dtype], device=dev)
    if layout == "packed":
        big = big.contiguous(memory_format=torch.channels_last)
        assert big.stride() == (3 * h * w, 1, 3 * w, 3)
    return big, big


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.int32)


def compare(big, out_view_of, want, what):
    """every element of the allocation: the model's inside the view, the canary outside"""
    torch.cuda.synchronize()
    got = big.float().cpu().numpy()
    full = np.full(got.shape, CANARY, F32)
    out_view_of(full)[...] = want
    if not np.array_equal(bits(got), bits(full)):
        bad = np.argwhere(bits(got) != bits(full))
        raise AssertionError(f"{what}: {len(bad)} elements differ, first at {bad[:5].tolist()}: got "
                             f"{got[tuple(bad[0])]}, want {full[tuple(bad[0])]}")


def view_of(layout, canvas):
    w, h = canvas
    if layout == "slice":
        return lambda a: a[::2, :, 1:1 + h, 1:1 + w]
    return lambda a: a


def run_matrices(vali, gpu, fmt, rows, canvas, dtype="float32", layout="planar", norm=wm.IDENTITY, pad=(0, 0, 0), cc_ctx=None,
                 surfs=None, hosts=None, seed=0):
    sizes = sizes_of(fmt)
    if surfs is None:
        surfs, hosts = make_frames(vali, gpu, fmt, sizes, seed)
    wp = vali.PySurfaceWarper(gpu, mean=norm[1], std=norm[2], div=norm[0])
    big, out = out_tensor(len(rows), canvas, dtype, layout, gpu)
    mats = device_marks(rows, gpu)
    wb = wp.PrepareMatrices(surfs, out, mats)
    ok, info = wp.Run(wb, pad=pad, cc_ctx=cc_ctx)
    assert ok and info == vali.TaskExecInfo.SUCCESS, info
    init = np.full((len(rows), 3, canvas[1], canvas[0]), CANARY, F32)
    want, inside = wm.warp(hosts, fmt, sizes, rows, canvas, norm, pad, csc_of(vali, cc_ctx) if fmt == "NV12" else None, dtype,
                           init)
    compare(big, view_of(layout, canvas), want, (fmt, canvas, dtype, layout, pad))
    return want, inside


# ---- the sampler: formats, dtypes, layouts, canvases ----------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["planar", "packed"])
@pytest.mark.parametrize("dtype", list(DT))
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format_dtype_and_layout_over_the_canvases(vali, gpu, fmt, dtype, layout):
    sizes = sizes_of(fmt)
    surfs, hosts = make_frames(vali, gpu, fmt, sizes, 1)
    for k, canvas in enumerate(CANVASES):
        rows = coverage_rows(sizes, canvas, 10 * k + len(fmt))
        _, inside = run_matrices(vali, gpu, fmt, rows, canvas, dtype, layout, NORM, (10, 200, 90), mpeg709(vali), surfs, hosts)
        assert 0.2 < inside.mean() < 0.98 and inside[3].any()


@pytest.mark.parametrize("dtype", list(DT))
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_slice_with_guard_bands_and_no_pad(vali, gpu, fmt, dtype):
    """out = big[::2, :, 1:1 + h, 1:1 + w]: rows start off the 16-byte grid; pad=None leaves the canary wherever nothing
    is sampled, and nothing outside the view changes"""
    sizes = sizes_of(fmt)
    surfs, hosts = make_frames(vali, gpu, fmt, sizes, 2)
    for k, canvas in enumerate(CANVASES):
        rows = coverage_rows(sizes, canvas, 100 + 10 * k + len(fmt))
        want, inside = run_matrices(vali, gpu, fmt, rows, canvas, dtype, "slice", NORM, None, None, surfs, hosts)
        assert (want[:, 0][~inside] == CANARY).all() and (~inside).sum() > 0
        run_matrices(vali, gpu, fmt, rows, canvas, dtype, "slice", wm.IDENTITY, (255, 0, 7), None, surfs, hosts)


@pytest.mark.parametrize("layout", ["planar", "packed"])
def test_no_pad_in_both_layouts(vali, gpu, layout):
    for fmt in ("NV12", "BGR"):
        for canvas in ((33, 9), (130, 70)):
            rows = coverage_rows(sizes_of(fmt), canvas, 7)
            run_matrices(vali, gpu, fmt, rows, canvas, "float16", layout, NORM, None, seed=3)
            run_matrices(vali, gpu, fmt, rows, canvas, "float32", layout, NORM, None, seed=3)


@pytest.mark.parametrize("fmt", FORMATS)
def test_frames_at_odd_addresses(vali, gpu, fmt):
    sizes = sizes_of(fmt)
    hosts = [am.noise_frame(fmt, w, h, 40 + i) for i, (w, h) in enumerate(sizes)]
    for x0, extra in ((3, 9), (1, 1)):
        bufs, views = [], []
        for i, (w, h) in enumerate(sizes):
            (prows, cols), = am.plane_shapes(fmt, w, h)
            pitch = (cols + x0 + extra) | 1
            buf = torch.full((prows + 4, pitch), 0xA5, dtype=torch.uint8, device=f"cuda:{gpu}")
            buf[2:2 + prows, x0:x0 + cols] = torch.from_numpy(hosts[i].reshape(prows, cols)).to(buf.device)
            bufs.append(buf)
            views.append(buf[2:2 + prows, x0:x0 + cols])
        torch.cuda.synchronize()
        surfs = [vali.Surface.from_dlpack(v, getattr(vali, fmt)) for v in views]
        assert surfs[0].PixelPtr(0) % 2 == 1 and surfs[0].Pitch % 16
        for canvas in ((16, 16), (33, 9)):
            run_matrices(vali, gpu, fmt, coverage_rows(sizes, canvas, 5), canvas, "float16", "planar", NORM, (1, 2, 3), None,
                         surfs, hosts)
        for i, (w, h) in enumerate(sizes):                       # the frames are read only
            (prows, cols), = am.plane_shapes(fmt, w, h)
            buf = bufs[i].cpu().numpy()
            assert np.array_equal(buf[2:2 + prows, x0:x0 + cols].reshape(-1), hosts[i])
            buf[2:2 + prows, x0:x0 + cols] = 0xA5
            assert (buf == 0xA5).all()


@pytest.mark.parametrize("pad", [None, (9, 8, 7)])
def test_skipped_slots_and_repeated_frames(vali, gpu, pad):
    """frame indices -1, N and INT32_MIN are skipped: all pad, or untouched; one frame feeds several slots"""
    for fmt in ("NV12", "RGB_PLANAR"):
        ident = [1, 0, 2, 0, 1, 4]
        rows = wm.pack_rows([-1, 1, 2, 1, I32_MIN, 1, (1 << 31) - 1, 0], [ident] * 8)
        want, inside = run_matrices(vali, gpu, fmt, rows, (16, 16), "bfloat16", "planar", NORM, pad, seed=4)
        assert not inside[[0, 2, 4, 6]].any() and inside[[1, 3, 5, 7]].all()
        assert np.array_equal(want[1], want[3]) and np.array_equal(want[1], want[5])


# ---- hostile rows ----------------------------------------------------------------------------------------------------------------
def hostile_rows(W, H):
    nan, inf = np.nan, np.inf
    below = lambda v: float(np.nextafter(F32(v), F32(-inf)))
    above = lambda v: float(np.nextafter(F32(v), F32(inf)))
    co = [
        [nan, 0, 0, 0, 1, 0], [1, 0, nan, 0, 1, 0], [1, 0, 0, 0, nan, 0], [1, 0, 0, 0, 1, nan],
        [inf, 0, 0, 0, 1, 0], [1, -inf, 0, 0, 1, 0], [inf, -inf, 0, 0, 1, 0], [1, 0, inf, 0, 1, -inf], [1, 0, -inf, 0, 1, 0],
        [1e30, 0, 0, 0, 1, 0], [1e30, -1e30, 0, 0, 1, 0], [1, 0, 0, 1e30, -1e30, 5], [3e38, 3e38, 3e38, 1, 0, 0],
        [1e-42, 0, 0, 0, 1e-42, 0], [1, 0, -1e-45, 0, 1, 0], [1e-40, 1e-40, 3, 1e-40, 0, 2],
        [0, 0, 0, 0, 0, 0],                                   # every pixel samples (0, 0)
        [0, 0, 7.25, 0, 0, 3.75],                             # ... and one point between four texels
        [0, 0, W, 0, 0, 0], [0, 0, 0, 0, 0, H],               # exactly on W, on H: outside
        [0, 0, below(W), 0, 0, below(H)],                     # just inside the far corner
        [0, 0, above(W), 0, 0, 1], [0, 0, below(0), 0, 0, 1], [0, 0, -0.0, 0, 0, -0.0],
        [1, 0, -0.5, 0, 1, -0.5], [1, 0, W - 15.5, 0, 1, H - 15.5],  # a first column exactly on 0 (inside), a last on W (outside)
        [-1, 0, 16, 0, -1, 16],                               # a half turn
    ]
    return wm.pack_rows([0] * len(co), co)


@pytest.mark.parametrize("fmt", FORMATS)
def test_hostile_rows(vali, gpu, fmt):
    W, H = sizes_of(fmt)[0]
    rows = hostile_rows(W, H)
    want, inside = run_matrices(vali, gpu, fmt, rows, (16, 16), "float32", "planar", NORM, (4, 5, 6), seed=5)
    assert not inside[:10].any() and not inside[12].any() and inside[13:18].all() and not inside[18].any() and not inside[19].any()
    assert np.array_equal(inside[10], np.eye(16, dtype=bool)) and np.array_equal(inside[11], np.eye(16, dtype=bool))
    assert inside[20].all() and not inside[21].any() and not inside[22].any() and inside[23].all() and inside[24].all()
    assert inside[25, :15, :15].all() and not inside[25, 15].any() and not inside[25, :, 15].any()
    run_matrices(vali, gpu, fmt, rows, (16, 16), "float16", "packed", NORM, None, seed=5)


# ---- two independent kernels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_an_integer_shift_is_the_preprocessors_same_size_rectangle(vali, gpu, fmt, dtype):
    """PySurfacePreprocessor.RunTensorBatch of a same-size rectangle and an integer shift at scale 1 are the same texels
    through the same normalisation; NV12 on frames whose chroma planes are flat (there the two differ in chroma siting)"""
    sizes = sizes_of(fmt)
    hosts = [am.noise_frame(fmt, w, h, 60 + i) for i, (w, h) in enumerate(sizes)]
    if fmt == "NV12":
        for host, (w, h), uv in zip(hosts, sizes, ((90, 170), (200, 40))):
            host[w * h:] = np.tile(np.array(uv, np.uint8), w * h // 4)
    up = vali.PyFrameUploader(gpu)
    surfs = [vali.Surface.Make(getattr(vali, fmt), w, h, gpu) for w, h in sizes]
    for s, host in zip(surfs, hosts):
        assert up.Run(host, s)[0]
    w, h = 16, 12
    shifts = [(0, 0, 0), (1, 4, 2), (0, 48, 36), (1, 18, 14)] if fmt == "NV12" else [(0, 0, 0), (1, 5, 3), (0, 48, 36), (1, 33, 25)]
    mean, std, div = NORM[1], NORM[2], NORM[0]
    wp = vali.PySurfaceWarper(gpu, mean=mean, std=std, div=div)
    pp = vali.PySurfacePreprocessor(gpu, mean=mean, std=std, div=div)
    a = torch.full((4, 3, h, w), CANARY, dtype=DT[dtype], device=f"cuda:{gpu}")
    b = torch.full((4, 3, h, w), CANARY, dtype=DT[dtype], device=f"cuda:{gpu}")
    rows = wm.pack_rows([f for f, _, _ in shifts], [[1, 0, x, 0, 1, y] for _, x, y in shifts])
    cc = mpeg709(vali)
    wb = wp.PrepareMatrices(surfs, a, device_marks(rows, gpu))
    assert wp.Run(wb, pad=None, cc_ctx=cc)[0]
    tb = pp.PrepareTensorBatch([surfs[f] for f, _, _ in shifts], b, [(x, y, w, h) for _, x, y in shifts], [(0, 0, w, h)] * 4)
    assert pp.RunTensorBatch(tb, None, cc)[0]
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not (a == CANARY).any()


# ---- the fit -----------------------------------------------------------------------------------------------------------------------
SIZES = [(64, 48), (34, 26)]
RECTS = [(0, 0, 64, 48, 0, 4, 32, 24), (4, 2, 24, 18, 1, 3, 30, 22)]
N, D, K = 2, 3, 40
T5 = [(u / 7, v / 7) for u, v in wm.ARCFACE_112]             # the ArcFace points on a 16 x 16 canvas
T17 = [(float("nan"), float("nan"))] + [T5[0], T5[1]] + [(float("nan"), 50.0)] * 14   # the eyes alone


def row(frame, x, y, w, h, k):
    return (frame, x, y, w, h, 0, 0x3F000000, k)


DETS = [row(0, 5, 7, 40, 30, 3), row(0, 20, 10, 30, 30, 39), row(0, -5, -4, 90, 70, 17),
        row(1, 3, 5, 20, 15, 0), row(1, 10, 6, 20, 18, 21), row(1, 0, 0, 34, 26, 8)]
# rows PyPoseDrawer skips (a foreign frame field, k = K, w = 0, frame -1, a box beside the frame) and one it draws
DETS_SKIPS = [row(1, 5, 7, 40, 30, 3), row(0, 20, 10, 30, 30, K), row(0, 5, 7, 0, 30, 2),
              row(-1, 3, 5, 20, 15, 0), row(1, 40, 6, 20, 18, 21), row(1, 0, 0, 34, 26, 8)]


def to_device(host, dtype, gpu):
    t = torch.from_numpy(np.ascontiguousarray(host)).to(f"cuda:{gpu}").to(DT[dtype])
    assert np.array_equal(t.float().cpu().numpy(), host, equal_nan=True)
    return t


def run_fit(vali, gpu, kpts, dets, template, fmt="NV12", dtype="float32", thr=0.5, min_points=2, given=True, transposed=False,
            dev_rects=False, canvas=(16, 16), pad=(0, 0, 0), seed=0):
    """fit and sample; compares the matrices (when given) and the crops with the model run on the model's matrices"""
    surfs, hosts = make_frames(vali, gpu, fmt, SIZES, seed)
    wp = vali.PySurfaceWarper(gpu, mean=NORM[1], std=NORM[2], div=NORM[0])
    kt = to_device(kpts, dtype, gpu)
    if transposed:                              # (N, P, kdim, K) in memory, seen as (N, K, P, kdim)
        kt = kt.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert not kt.is_contiguous() and kt.stride(1) == 1
    big, out = out_tensor(N * D, canvas, "float16", "planar", gpu)
    mats = torch.full((N * D, 8), 77, dtype=torch.int32, device=f"cuda:{gpu}") if given else None
    wb = wp.PrepareKeypoints(surfs, out, kt, device_marks(dets, gpu), max_det=D, template=template, matrices=mats)
    rects = torch.tensor(np.asarray(RECTS, np.int32), dtype=torch.int32, device=f"cuda:{gpu}") if dev_rects else RECTS
    torch.cuda.synchronize()
    ok, info = wp.Run(wb, rects, kpt_thr=thr, min_points=min_points, pad=pad)
    assert ok and info == vali.TaskExecInfo.SUCCESS, info
    want_rows = wm.fit(SIZES, dets, D, kpts, RECTS, template, thr, min_points)
    if given:
        got = mats.cpu().numpy()
        assert np.array_equal(got, want_rows), np.argwhere(got != want_rows)[:6].tolist()
    init = np.full((N * D, 3, canvas[1], canvas[0]), CANARY, F32)
    want, inside = wm.warp(hosts, fmt, SIZES, want_rows, canvas, NORM, pad, csc_of(vali, None) if fmt == "NV12" else None,
                           "float16", init)
    compare(big, lambda a: a, want, ("fit", fmt, dtype, given))
    return want_rows, inside


def kpts_for(p, dtype="float32", seed=0, kdim=3):
    return pc.kpts(p, dtype, seed, kdim, N, K, SIZES, RECTS)


@pytest.mark.parametrize("dtype", list(DT))
def test_five_points_in_every_dtype(vali, gpu, dtype):
    rows, inside = run_fit(vali, gpu, kpts_for(5, dtype), DETS, T5, dtype=dtype, seed=1)
    assert (rows[:, 0] == [0, 0, 0, 1, 1, 1]).all() and set(rows[:, 7]) <= {4, 5} and inside.any()
    run_fit(vali, gpu, kpts_for(5, dtype, 2), DETS, T5, fmt="RGB", dtype=dtype, given=False, dev_rects=True, seed=2)


def test_seventeen_points_aligned_by_two(vali, gpu):
    rows, _ = run_fit(vali, gpu, kpts_for(17), DETS, T17, canvas=(33, 9), seed=3)
    assert (rows[:, 7] == 2).all()
    full = [(3.0 + 5 * (j % 5), 2.0 + 4 * (j // 5)) for j in range(17)]
    rows, _ = run_fit(vali, gpu, kpts_for(17, seed=1), DETS, full, fmt="BGR", seed=3)
    assert (rows[:, 7] >= 16).all()


def test_invisible_and_non_finite_keypoints_and_min_points(vali, gpu):
    k = kpts_for(5).copy()
    k[:, 0::4, 0, 2] = 0.2                  # below the threshold
    k[:, 1::4, 1, 0] = np.nan
    k[:, 2::4, 2, 1] = np.inf
    k[:, 3::4, 3, 2] = np.nan
    k[:, 3::4, 0, 0] = -np.inf
    k[:, 3::4, 1, 2] = 0.5                  # exactly the threshold: invisible
    rows, _ = run_fit(vali, gpu, k, DETS, T5, seed=4)
    # k = 3 and 39 keep one keypoint: skipped; 17 and 21 keep three, 0 and 8 four
    assert (rows[:2, 0] == -1).all() and rows[2:, 7].tolist() == [3, 4, 3, 4]
    rows, _ = run_fit(vali, gpu, k, DETS, T5, min_points=4, pad=None, seed=4)
    assert (rows[:, 0] == -1).any() and (rows[:, 0] >= 0).any()
    rows, _ = run_fit(vali, gpu, k, DETS, T5, thr=0.99, min_points=5, seed=4)
    assert (rows[:, 0] == -1).all() and not rows[:, 1:].any()


def test_coincident_points(vali, gpu):
    rows, _ = run_fit(vali, gpu, kpts_for(5), DETS, [T5[0]] * 5, seed=5)     # Dn == 0
    assert (rows[:, 0] == -1).all()
    k = kpts_for(5).copy()
    k[:, :, :, :2] = k[:, :, :1, :2]                                                     # al = be = 0
    rows, inside = run_fit(vali, gpu, k, DETS, T5, seed=5)
    assert (rows[:, 0] >= 0).all() and not (rows[:, [1, 2, 4, 5]] & 0x7FFFFFFF).any() and inside.any()


def test_keypoints_without_a_confidence_and_a_transposed_head(vali, gpu):
    run_fit(vali, gpu, kpts_for(5, kdim=2), DETS, T5, seed=6)
    run_fit(vali, gpu, kpts_for(5, "float16"), DETS, T5, dtype="float16", transposed=True, seed=6)
    run_fit(vali, gpu, kpts_for(17, "bfloat16"), DETS, T17, dtype="bfloat16", transposed=True, given=False, seed=6)


def test_the_rows_the_pose_drawer_skips(vali, gpu):
    rows, inside = run_fit(vali, gpu, kpts_for(5), DETS_SKIPS, T5, seed=7)
    assert (rows[:5, 0] == -1).all() and rows[5, 0] == 1 and not inside[:5].any()
    rows, _ = run_fit(vali, gpu, kpts_for(5), DETS_SKIPS, T5, pad=None, given=False, seed=7)


# ---- capture ---------------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay_after_everything_was_rewritten_in_place(vali, gpu):
    from vali_amd._native import shim

    fmt, dev = "NV12", f"cuda:{gpu}"
    stream = shim.stream_create(gpu)
    wp = vali.PySurfaceWarper(gpu, stream, mean=NORM[1], std=NORM[2], div=NORM[0])
    sets = [(DETS, kpts_for(5, seed=0)), (DETS_SKIPS, kpts_for(5, seed=1)), (list(reversed(DETS[:3])) + DETS[3:], kpts_for(5, seed=2))]
    kt = to_device(sets[0][1], "float32", gpu)
    dets = device_marks(sets[0][0], gpu)
    rects = torch.tensor(np.asarray(RECTS, np.int32), dtype=torch.int32, device=dev)
    surfs, _ = make_frames(vali, gpu, fmt, SIZES, seed=12)
    canvas = (16, 16)
    big, out = out_tensor(N * D, canvas, "float32", "planar", gpu)
    mats = torch.zeros((N * D, 8), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    wb = wp.PrepareKeypoints(surfs, out, kt, dets, max_det=D, template=T5, matrices=mats)
    cap =vali.StreamCapture(stream, gpu)
    with cap:
        with pytest.raises(RuntimeError, match="capturing"):
            wp.PrepareMatrices(surfs, out, mats)
        assert wp.RunAsync(wb, rects, pad=(1, 2, 3))[0]
    cap.Keep(wb)
    for k, (drows, kp) in enumerate(sets):
        hosts = [am.noise_frame(fmt, w, h, 300 + 10 * k + i) for i, (w, h) in enumerate(SIZES)]
        for s, host in zip(surfs, hosts):
            assert vali.PyFrameUploader(gpu).Run(host, s)[0]
        dets.copy_(device_marks(drows, gpu))                       # rewritten in place
        kt.copy_(to_device(kp, "float32", gpu))
        mats.fill_(5)
        torch.cuda.synchronize()
        cap.Launch()
        shim.stream_sync(gpu, stream)
        want_rows = wm.fit(SIZES, drows, D, kp, RECTS, T5)
        assert np.array_equal(mats.cpu().numpy(), want_rows), k
        want, _ = wm.warp(hosts, fmt, SIZES, want_rows, canvas, NORM, (1, 2, 3), csc_of(vali, None))
        compare(big, lambda a: a, want, ("replay", k))
    # form (a): the matrices rewritten in place between replays
    wb2 = wp.PrepareMatrices(surfs, out, mats)
    cap2 = vali.StreamCapture(stream, gpu)
    with cap2:
        assert wp.RunAsync(wb2, pad=(0, 0, 0))[0]
    cap2.Keep(wb2)
    for k in range(2):
        rows = coverage_rows(SIZES, canvas, 50 + k)
        mats.copy_(device_marks(rows, gpu))
        torch.cuda.synchronize()
        cap2.Launch()
        shim.stream_sync(gpu, stream)
        want, _ = wm.warp(hosts, fmt, SIZES, rows, canvas, NORM, (0, 0, 0), csc_of(vali, None))
        compare(big, lambda a: a, want, ("replay of matrices", k))


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_prepare_and_run_say_what_is_wrong(vali, gpu):
    wp = vali.PySurfaceWarper(gpu)
    dev = f"cuda:{gpu}"
    surfs, _ = make_frames(vali, gpu, "NV12", SIZES, 13)
    out = torch.zeros((6, 3, 16, 16), dtype=torch.float16, device=dev)
    mats = torch.zeros((6, 8), dtype=torch.int32, device=dev)
    kt, dets = to_device(kpts_for(5), "float32", gpu), device_marks(DETS, gpu)
    with pytest.raises(ValueError, match="std must be non-zero"):
        vali.PySurfaceWarper(gpu, std=(1, 0, 1))
    with pytest.raises(ValueError, match="matrices: need an int32"):
        wp.PrepareMatrices(surfs, out, mats.float())
    with pytest.raises(ValueError, match="matrices: need an int32"):
        wp.PrepareMatrices(surfs, out, mats[:5])
    with pytest.raises(ValueError, match="contiguous"):
        wp.PrepareMatrices(surfs, out, torch.zeros((6, 16), dtype=torch.int32, device=dev)[:, ::2])
    with pytest.raises(ValueError, match="16-byte aligned"):
        wp.PrepareMatrices(surfs, out, torch.zeros(50, dtype=torch.int32, device=dev)[1:49].view(6, 8))
    with pytest.raises(ValueError, match="GPU"):
        wp.PrepareMatrices(surfs, out, mats.cpu())
    with pytest.raises(ValueError, match="neither planar"):
        wp.PrepareMatrices(surfs, out.transpose(2, 3), mats)
    with pytest.raises(ValueError, match="one format per batch"):
        wp.PrepareMatrices([surfs[0], vali.Surface.Make(vali.RGB, 34, 26, gpu)], out, mats)
    with pytest.raises(ValueError, match="supported"):
        wp.PrepareMatrices([vali.Surface.Make(vali.YUV420, 34, 26, gpu)], out, mats)
    with pytest.raises(ValueError, match="M = 6 slots"):
        wp.PrepareKeypoints(surfs, out, kt, dets, max_det=2)
    with pytest.raises(ValueError, match="3 surfaces"):
        wp.PrepareKeypoints(surfs + surfs[:1], out, kt, dets, max_det=D)
    with pytest.raises(ValueError, match="4 pairs"):
        wp.PrepareKeypoints(surfs, out, kt, dets, max_det=D, template=T5[:4])
    wa, wb = wp.PrepareMatrices(surfs, out, mats), wp.PrepareKeypoints(surfs, out, kt, dets, max_det=D)
    with pytest.raises(ValueError, match="rects"):
        wp.Run(wa, RECTS)
    with pytest.raises(ValueError, match="rects"):
        wp.Run(wb)
    with pytest.raises(ValueError, match="rects"):
        wp.Run(wb, RECTS[:1])
    with pytest.raises(ValueError, match="min_points = 6"):
        wp.Run(wb, RECTS, min_points=6)
    with pytest.raises(ValueError, match="kpt_thr"):
        wp.Run(wb, RECTS, kpt_thr=float("nan"))
    with pytest.raises(ValueError, match="WarpBatch"):
        wp.Run(5)
    assert wp.Run(wa, pad=(1, 2)) == (False, vali.TaskExecInfo.INVALID_INPUT)
    bt601_mpeg = vali.ColorspaceConversionContext(vali.ColorSpace.BT_601, vali.ColorRange.MPEG)
    assert wp.Run(wa, cc_ctx=bt601_mpeg) == (False, vali.TaskExecInfo.UNSUPPORTED_FMT_CONV_PARAMS)
    rgb, _ = make_frames(vali, gpu, "RGB", SIZES, 13)
    assert wp.Run(wp.PrepareMatrices(rgb, out, mats), cc_ctx=bt601_mpeg)[0]          # accepted and ignored
