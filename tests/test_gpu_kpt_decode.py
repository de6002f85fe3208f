"""PyKeypointDecoder on the GPU against tests/kpt_decode_model.py: points bit for bit, kpts bit for bit but for which NaN a
NaN is.  Every dtype, form, mapping, alignment and refinement; the shapes at which the kernel takes another path (no
16-byte row body, more than one pass per lane, a wave or the workgroup per map: 8192 elements is the threshold); rows off
the 16-byte grid; planted ties, NaN maps, hostile mapping rows; a captured call replayed after its tensors were rewritten."""
import numpy as np
import pytest

import kpt_decode_model as kd

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DT = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
SIZES = [(640, 480), (66, 34), (1920, 1080)]
N, D = 3, 4
CANVAS = (192, 256)
PAD = 3.0e4            # what surrounds a view's rows: greater than every element, finite in float16


@pytest.fixture(scope="module")
def frames(vali, gpu):
    return [vali.Surface.Make(vali.RGB, w, h, gpu) for w, h in SIZES]


@pytest.fixture(scope="module")
def dec(vali, gpu):
    return vali.PyKeypointDecoder(gpu)


def exact(host, dtype):
    """the float32 values a tensor of `dtype` holds"""
    return torch.from_numpy(np.ascontiguousarray(host, np.float32)).to(DT[dtype]).float().numpy()


def place(host, dtype, gpu, layout="plain"):
    """`host` (its last dimension the rows) on the device in `dtype` as a view of the given layout"""
    dev = f"cuda:{gpu}"
    t = torch.from_numpy(np.ascontiguousarray(host, np.float32)).to(dev).to(DT[dtype])
    if layout == "plain":
        return t
    if layout == "offset":            # the base and every row one element off
        big = torch.full(t.shape[:-1] + (t.shape[-1] + 1,), PAD, dtype=DT[dtype], device=dev)
        big[..., 1:] = t
        view = big[..., 1:]
        assert view.data_ptr() % 16 == t.element_size()
        return view
    if layout == "pitched":           # a slice of a wider tensor with more keypoints
        shape = list(t.shape)
        shape[1] += 2
        shape[-1] += 5
        big = torch.full(shape, PAD, dtype=DT[dtype], device=dev)
        big[:, 1:1 + t.shape[1], ..., 3:3 + t.shape[-1]] = t
        view = big[:, 1:1 + t.shape[1], ..., 3:3 + t.shape[-1]]
        assert not view.is_contiguous() or t.shape[-1] == 1
        return view
    assert layout == "expanded"
    view = t[:1].expand(host.shape[0], *[-1] * (t.dim() - 1))
    assert view.stride(0) == 0
    return view


def similarity_rows(rng, m, n=N):
    """random similarities from the canvas into the frames, frames in turn"""
    s, th = rng.uniform(0.3, 4.0, m), rng.uniform(0, 2 * np.pi, m)
    mats = np.stack([s * np.cos(th), -s * np.sin(th), rng.uniform(-50, 600, m), s * np.sin(th), s * np.cos(th),
                     rng.uniform(-50, 400, m)], 1)
    return kd.matrix_rows(np.arange(m) % n, mats)


def roi_rows(rng, m):
    rows = np.zeros((m, 8), np.int32)
    rows[:, 0], rows[:, 1] = rng.integers(-20, 500, m), rng.integers(-20, 300, m)
    rows[:, 2], rows[:, 3] = rng.integers(1, 400, m), rng.integers(1, 400, m)
    rows[:, 4], rows[:, 5] = rng.integers(-8, 8, m), rng.integers(-8, 8, m)
    rows[:, 6], rows[:, 7] = rng.integers(1, 300, m), rng.integers(1, 300, m)
    return rows


def run(vali, gpu, dec, frames, rows, rois, canvas, heat=None, simcc=None, dtype="float32", layout="plain", thr=0.3,
        refine="quarter", align="centre", with_kpts=True, what=None):
    """one Prepare and Run against the model; `heat` / `simcc` are float32 host arrays exact in `dtype`"""
    dev = f"cuda:{gpu}"
    m = len(rows)
    n = len(frames)
    p = (heat if heat is not None else simcc[0]).shape[1]
    dr = torch.from_numpy(np.ascontiguousarray(rows, np.int32)).to(dev)
    points = torch.full((m, p, 4), -7, dtype=torch.int32, device=dev)
    kpts = torch.full((m, p, 3), -7.0, dtype=torch.float32, device=dev) if with_kpts else None
    mapping = dict(rois=dr, max_det=m // n) if rois else dict(matrices=dr)
    if heat is not None:
        full = heat if layout != "expanded" else np.repeat(heat[:1], m, 0)
        kb = dec.PrepareHeatmaps(frames, place(heat, dtype, gpu, layout), points, canvas=canvas, kpts=kpts, **mapping)
        want = kd.decode(SIZES[:n], rows, m // n if rois else 0, canvas, heat=full, thr=thr, refine=refine, align=align)
    else:
        kb = dec.PrepareSimcc(frames, place(simcc[0], dtype, gpu, layout), place(simcc[1], dtype, gpu, layout), points,
                              canvas=canvas, kpts=kpts, **mapping)
        full = simcc if layout != "expanded" else tuple(np.repeat(v[:1], m, 0) for v in simcc)
        want = kd.decode(SIZES[:n], rows, m // n if rois else 0, canvas, simcc=full, thr=thr, refine=refine, align=align)
    torch.cuda.synchronize()
    ok, info = dec.Run(kb, kpt_thr=thr, refine=refine, align=align)
    assert ok and info == vali.TaskExecInfo.SUCCESS, info
    got = points.cpu().numpy()
    if not np.array_equal(got, want[0]):
        bad = np.argwhere((got != want[0]).any(2))
        raise AssertionError(f"{what}: {len(bad)} points differ, first (m, j) = {bad[0]}: got {got[tuple(bad[0])]}, "
                             f"want {want[0][tuple(bad[0])]}")
    if with_kpts:
        gk = kpts.cpu().numpy()
        assert kd.same_floats(gk, want[1]), (what, np.argwhere(gk.view(np.int32) != want[1].view(np.int32))[:4])
    return want


def random_maps(rng, shape, dtype):
    return exact(rng.standard_normal(shape) * 0.5 + 0.2, dtype)


# ---- the table --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rois", [False, True], ids=["matrices", "rois"])
@pytest.mark.parametrize("dtype", list(DT))
def test_heatmaps_every_dtype_mapping_alignment_and_refinement(vali, gpu, dec, frames, dtype, rois):
    rng = np.random.default_rng(1)
    m = N * D
    heat = random_maps(rng, (m, 17, 64, 48), dtype)
    rows = roi_rows(rng, m) if rois else similarity_rows(rng, m)
    visible = 0
    for align in ("centre", "index"):
        for refine in ("quarter", "none"):
            pts, _ = run(vali, gpu, dec, frames, rows, rois, CANVAS, heat=heat, dtype=dtype, refine=refine, align=align,
                         what=(dtype, rois, align, refine))
            visible += int((pts[..., 3] == 3).sum())
    assert visible > 100            # the case is not vacuous


@pytest.mark.parametrize("rois", [False, True], ids=["matrices", "rois"])
@pytest.mark.parametrize("dtype", list(DT))
def test_simcc_every_dtype_mapping_and_alignment(vali, gpu, dec, frames, dtype, rois):
    rng = np.random.default_rng(2)
    m = N * D
    rows = roi_rows(rng, m) if rois else similarity_rows(rng, m)
    for wx, wy in ((1, 9), (9, 1), (384, 512), (383, 9)):
        sim = (random_maps(rng, (m, 17, wx), dtype), random_maps(rng, (m, 17, wy), dtype))
        for align in ("centre", "index"):
            run(vali, gpu, dec, frames, rows, rois, CANVAS, simcc=sim, dtype=dtype, refine="none", align=align,
                what=(dtype, rois, wx, wy, align))


# ---- shapes -----------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 7), (5, 3), (17, 13), (64, 48), (72, 96), (130, 257)]       # (Hh, Wh); 72 x 96 < 8192 < 130 x 257


@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("hh,wh", SHAPES, ids=lambda v: str(v))
def test_shapes_slots_and_keypoint_counts(vali, gpu, dec, frames, hh, wh, dtype):
    assert 72 * 96 <= 8192 < 130 * 257          # one shape on each side of the wave / workgroup threshold
    rng = np.random.default_rng(3)
    combos = [(1, 1), (1, 17), (N * D, 64)] if hh * wh <= 72 * 96 else [(1, 17), (N * D, 3)]
    for m, p in combos:
        heat = random_maps(rng, (m, p, hh, wh), dtype)
        n = 1 if m == 1 else N
        for rois in (False, True):
            rows = roi_rows(rng, m) if rois else similarity_rows(rng, m, n)
            run(vali, gpu, dec, frames[:n], rows, rois, CANVAS, heat=heat, dtype=dtype, what=(hh, wh, m, p, rois))


# ---- layouts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["offset", "pitched", "expanded"])
@pytest.mark.parametrize("dtype", list(DT))
def test_views_off_the_16_byte_grid_and_expanded_tensors(vali, gpu, dec, frames, dtype, layout):
    """what surrounds a view's rows is greater than every element: a load outside a row would move the peak"""
    rng = np.random.default_rng(4)
    m = N * D
    rows = similarity_rows(rng, m)
    for hh, wh in ((17, 13), (64, 48), (72, 96), (130, 257)):
        p = 5 if hh * wh > 8192 else 17
        heat = random_maps(rng, (m, p, hh, wh), dtype)
        assert heat.max() < PAD
        run(vali, gpu, dec, frames, rows, False, CANVAS, heat=heat, dtype=dtype, layout=layout, what=(layout, hh, wh))
    sim = (random_maps(rng, (m, 17, 383), dtype), random_maps(rng, (m, 17, 9), dtype))
    run(vali, gpu, dec, frames, rows, False, CANVAS, simcc=sim, dtype=dtype, layout=layout, refine="none", what=layout)


# ---- data -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("hh,wh", [(64, 48), (72, 96), (130, 257)], ids=lambda v: str(v))
def test_equal_maxima_in_other_lanes_waves_and_passes_the_lowest_index_wins(vali, gpu, dec, frames, hh, wh, dtype):
    rng = np.random.default_rng(5)
    p = 24
    heat = random_maps(rng, (1, p, hh, wh), dtype)
    flat = heat.reshape(p, hh * wh)
    total = hh * wh
    winners = []
    for j in range(p):
        if j == 0:
            idx = [total - 1]                                   # the peak at the last element
        elif j == 1:
            idx = [total - 1, total - 2, total // 2]
        elif j == 2:
            idx = [0, total - 1]
        elif j == 3:
            idx = list(range(5, total, 64))                     # one in every stretch of 64 elements
        else:
            idx = [int(v) for v in rng.choice(total, rng.integers(2, 7), replace=False)]
        flat[j, idx] = 7.0
        if j % 5 == 4:
            flat[j, idx[0]] = np.nan                            # a NaN among them never wins
            idx = idx[1:]
        winners.append(min(idx))
    pts, kp = run(vali, gpu, dec, frames[:1], kd.matrix_rows([0], [[1, 0, 0, 0, 1, 0]]), False, (wh, hh), heat=heat,
                  dtype=dtype, refine="none", what=(hh, wh))
    assert [int(v) for v in kp[0, :, 0] - 0.5 + wh * (kp[0, :, 1] - 0.5)] == winners


@pytest.mark.parametrize("hh,wh", [(5, 3), (64, 48), (130, 257)], ids=lambda v: str(v))
def test_nan_maps_infinities_and_signed_zeros(vali, gpu, dec, frames, hh, wh):
    rng = np.random.default_rng(6)
    heat = random_maps(rng, (2, 8, hh, wh), "float16")
    heat[0, 0] = np.nan
    heat[1, 3] = np.nan
    heat[0, 1] = -np.inf
    heat[0, 2, hh // 2, wh // 2] = np.inf
    heat[0, 3] = np.where(rng.random((hh, wh)) < 0.5, -0.0, 0.0)
    heat[0, 4] = np.nan
    heat[0, 4, hh - 1, wh - 1] = -3.0
    heat[1, 5, :, : wh // 2 + 1] = np.nan
    rows = similarity_rows(rng, 2, 2)
    for thr in (-np.inf, -1.0, 0.3):
        pts, kp = run(vali, gpu, dec, frames[:2], rows, False, CANVAS, heat=heat, dtype="float16", thr=thr, what=(hh, wh, thr))
        assert tuple(pts[0, 0]) == (0, 0, kd.NAN_BITS, 0) and np.isnan(kp[1, 3, 2])
    x, y = random_maps(rng, (2, 8, 33), "float16"), random_maps(rng, (2, 8, 9), "float16")
    x[0, 0], y[0, 1], x[1, 2], y[1, 2] = np.nan, np.nan, np.nan, np.nan
    x[0, 3], y[0, 3, 4] = -np.inf, np.inf
    run(vali, gpu, dec, frames[:2], rows, False, CANVAS, simcc=(x, y), dtype="float16", refine="none", thr=-1.0, what="simcc")


def test_hostile_mapping_rows(vali, gpu, dec, frames):
    rng = np.random.default_rng(7)
    m = N * D
    heat = random_maps(rng, (m, 17, 17, 13), "float32")
    rows = similarity_rows(rng, m)
    rows[0, 0], rows[1, 0], rows[2, 0], rows[3, 0] = -1, N, 1 << 30, -(1 << 31)          # frames outside 0..N-1
    f = rows[4:10, 1:7].view(np.float32)
    f[0, 0], f[1, 1], f[2, 2], f[3, 3], f[4, 4], f[5, 5] = np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan
    f[5, 0] = 3e38                                                                      # overflows in the product
    pts, kp = run(vali, gpu, dec, frames, rows, False, CANVAS, heat=heat, thr=-1.0, what="matrices")
    assert not pts[:4].any() and not kp[:4].any() and not pts[4:10, :, 3].any() and pts[10:, :, 3].any()
    rows = roi_rows(rng, m)
    rows[0] = 0                                                                         # all-zero rows: empty items
    rows[5] = 0
    rows[2, 2], rows[3, 3], rows[6, 6], rows[7, 7] = 0, -5, 0, -(1 << 31)
    pts, kp = run(vali, gpu, dec, frames, rows, True, CANVAS, heat=heat, what="rois")
    assert not pts[[0, 2, 3, 5, 6, 7]].any() and not kp[[0, 2, 3, 5, 6, 7]].any()
    for k in range(3):                                                                  # random int32 rows, both readings
        rows = rng.integers(-(1 << 31), 1 << 31, (m, 8)).astype(np.int32)
        rows[::3, 0] = np.arange(0, m, 3) % N
        run(vali, gpu, dec, frames, rows, False, CANVAS, heat=heat, what=("random matrices", k))
        rows[::2, [2, 3, 6, 7]] = np.abs(rows[::2, [2, 3, 6, 7]] >> rng.integers(0, 31, (len(rows[::2]), 4)))
        run(vali, gpu, dec, frames, rows, True, CANVAS, heat=heat, what=("random rois", k))


def test_without_kpts_only_points_are_written(vali, gpu, dec, frames):
    rng = np.random.default_rng(8)
    heat = random_maps(rng, (N * D, 5, 17, 13), "float32")
    run(vali, gpu, dec, frames, similarity_rows(rng, N * D), False, CANVAS, heat=heat, with_kpts=False, what="no kpts")


# ---- capture ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hh,wh", [(64, 48), (130, 257)], ids=lambda v: str(v))
def test_capture_and_replay_after_the_tensors_were_rewritten_in_place(vali, gpu, frames, hh, wh):
    from vali_amd._native import shim

    dev = f"cuda:{gpu}"
    rng = np.random.default_rng(9)
    m, p = N * D, 5
    stream = shim.stream_create(gpu)
    dec = vali.PyKeypointDecoder(gpu, stream)
    heat = torch.zeros((m, p, hh, wh), dtype=torch.float16, device=dev)
    rows = torch.zeros((m, 8), dtype=torch.int32, device=dev)
    points = torch.zeros((m, p, 4), dtype=torch.int32, device=dev)
    kpts = torch.zeros((m, p, 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    kb = dec.PrepareHeatmaps(frames, heat, points, canvas=CANVAS, matrices=rows, kpts=kpts)
    cap = vali.StreamCapture(stream, gpu)
    with cap:
        assert dec.RunAsync(kb, kpt_thr=0.3, refine="quarter", align="index")[0]
    cap.Keep(kb)
    for k in range(3):
        host = random_maps(rng, (m, p, hh, wh), "float16")
        hrows = similarity_rows(rng, m)
        if k == 1:
            hrows[::2, 0] = -1
            host[3] = np.nan
        heat.copy_(torch.from_numpy(host).to(dev))
        rows.copy_(torch.from_numpy(hrows).to(dev))
        torch.cuda.synchronize()
        cap.Launch()
        shim.stream_sync(gpu, stream)
        want = kd.decode(SIZES, hrows, 0, CANVAS, heat=host, thr=0.3, refine="quarter", align="index")
        assert np.array_equal(points.cpu().numpy(), want[0]), k
        assert kd.same_floats(kpts.cpu().numpy(), want[1]), k


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_prepare_and_run_say_what_is_wrong(vali, gpu, dec, frames):
    dev = f"cuda:{gpu}"
    m, p = N * D, 5
    heat = torch.zeros((m, p, 8, 8), dtype=torch.float16, device=dev)
    rows = torch.zeros((m, 8), dtype=torch.int32, device=dev)
    points = torch.zeros((m, p, 4), dtype=torch.int32, device=dev)
    for kw, word in ((dict(), "neither"), (dict(matrices=rows, rois=rows, max_det=D), "both"),
                     (dict(rois=rows), "max_det is required"), (dict(rois=rows, max_det=5), "slots"),
                     (dict(matrices=rows[:5]), "matrices"), (dict(matrices=rows.float()), "int32"),
                     (dict(matrices=rows, kpts=torch.zeros((m, p, 4), device=dev)), "kpts"),
                     (dict(matrices=rows, kpts=torch.zeros((m, p, 3), dtype=torch.float16, device=dev)), "kpts")):
        with pytest.raises(ValueError, match=word):
            dec.PrepareHeatmaps(frames, heat, points, canvas=CANVAS, **kw)
    with pytest.raises(ValueError, match="stride 1"):
        dec.PrepareHeatmaps(frames, heat.transpose(2, 3), points, canvas=CANVAS, matrices=rows)
    with pytest.raises(ValueError, match="dtype"):
        dec.PrepareHeatmaps(frames, heat.double(), points, canvas=CANVAS, matrices=rows)
    with pytest.raises(ValueError, match="points"):
        dec.PrepareHeatmaps(frames, heat, points[:, :4], canvas=CANVAS, matrices=rows)
    with pytest.raises(ValueError, match="16-byte"):
        dec.PrepareHeatmaps(frames, heat, torch.zeros(m * p * 4 + 1, dtype=torch.int32, device=dev)[1:].view(m, p, 4),
                            canvas=CANVAS, matrices=rows)
    with pytest.raises(ValueError, match="one dtype"):
        dec.PrepareSimcc(frames, heat[:, :, 0], heat[:, :, 1].float(), points, canvas=CANVAS, matrices=rows)
    kb = dec.PrepareHeatmaps(frames, heat, points, canvas=CANVAS, matrices=rows)
    ks = dec.PrepareSimcc(frames, heat[:, :, 0], heat[:, :, 1], points, canvas=CANVAS, matrices=rows)
    for args, word in (((kb, float("nan")), "NaN"), ((kb, 0.3, "dark"), "refine"), ((kb, 0.3, "none", "center"), "align"),
                       ((ks, 0.3, "quarter"), "SimCC"), ((ks,), "SimCC"), ((None,), "KeypointBatch")):
        with pytest.raises(ValueError, match=word):
            dec.Run(*args)
    assert dec.Run(ks, refine="none")[0]
