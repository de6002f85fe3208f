"""PySurfaceAnnotator on the GPU against tests/annotate_model.py, bit for bit.

Frame sizes are the smallest at which the kernel can go wrong: with T its tile side, 2 x 2, (T - 2)^2, T^2, (T + 2)^2 and
(2T + 2) x (T + 6); 1 x 1 and (T + 1) x (T - 1) for the formats that take odd sizes."""
import numpy as np
import pytest

import annotate_model as am
import postproc_model as pm

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

T = am.TILE
BATCHES = {"small": [(2, 2), (T - 2, T - 2), (2 * T + 2, T + 6)], "tile": [(T, T), (T + 2, T + 2), (2 * T + 2, T + 6)]}
ODD_BATCH = [(1, 1), (T + 1, T - 1), (T + 2, T + 2)]
ODD_OK = ("YUV444", "RGB", "BGR", "RGB_PLANAR")
KINDS = {"box": am.BOX, "fill": am.FILL, "pixelate": am.PIXELATE}
ROWS_601 = "601_JPEG"


# ---- helpers -----------------------------------------------------------------------------------------------------------
def make_frames(vali, gpu, fmt, sizes, seed=0):
    """Surface.Make frames holding seeded noise; returns (surfaces, their host images)"""
    up = vali.PyFrameUploader(gpu)
    surfs, hosts = [], []
    for i, (w, h) in enumerate(sizes):
        s = vali.Surface.Make(getattr(vali, fmt), w, h, gpu)
        host = am.noise_frame(fmt, w, h, seed * 100 + i)
        assert up.Run(host, s)[0]
        surfs.append(s)
        hosts.append(host)
    return surfs, hosts


def download(vali, gpu, s):
    host = np.zeros(s.HostSize, np.uint8)
    ok, info = vali.PySurfaceDownloader(gpu).Run(s, host)
    assert ok, info
    return host


def device_marks(rows, gpu):
    a = np.asarray(rows, np.int64).reshape(-1, 8)
    assert (a >= -(1 << 31)).all() and (a < (1 << 31)).all()
    t = torch.tensor(a.astype(np.int32), dtype=torch.int32, device=f"cuda:{gpu}")
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def ann(vali, gpu):
    return vali.PySurfaceAnnotator(gpu)


def check(vali, gpu, ann, fmt, sizes, rows, matrix=ROWS_601, seed=0, marks=None):
    """draw `rows` on fresh noise frames and compare every frame with the model; returns the model's list of drawn rows"""
    surfs, hosts = make_frames(vali, gpu, fmt, sizes, seed)
    ab = ann.PrepareBatch(surfs)
    ok, info = ann.RunBatch(ab, device_marks(rows, gpu) if marks is None else marks, pm.cc_ctx_of(vali, matrix))
    assert ok and info == vali.TaskExecInfo.SUCCESS, info
    drawn = am.apply(hosts, fmt, sizes, rows, pm.matrices()[matrix])
    for i, s in enumerate(surfs):
        got = download(vali, gpu, s)
        if not np.array_equal(got, hosts[i]):
            bad = np.flatnonzero(got != hosts[i])
            raise AssertionError(f"{fmt} frame {i} {sizes[i]}: {bad.size} bytes differ, first at {bad[:6]}: "
                                 f"got {got[bad[:6]]}, want {hosts[i][bad[:6]]}")
    return drawn


def colour(k, a=255):
    return am.pack_colour((k * 67 + 20) % 256, (k * 29 + 200) % 256, (k * 151 + 90) % 256, a)


def rects_for(w, h):
    """rectangles that straddle tile borders, lie partly and wholly outside, start at negative x, y, and overflow int32"""
    return [(T - 5, T - 7, 11, 13), (w - 3, h - 3, 10, 10), (w + 4, 0, 5, 5), (-10, -10, 5, 5), (-3, -5, 9, 11),
            (1, 1, 2**31 - 1, 3), (2**31 - 8, 0, 2**31 - 1, 2**31 - 1), (-2**31, -2**31, 2**31 - 1, 2**31 - 1),
            (0, 0, w, h), (w // 3, h // 4, max(w // 2, 1), max(h // 2, 1)), (T - 1, 0, 2, h), (0, T - 1, w, 2),
            (5, 3, 37, 41), (w - 1, h - 1, 1, 1)]


def rows_for(kind, sizes):
    args = {am.BOX: (1, 3, 40, 2), am.FILL: (0,), am.PIXELATE: am.CELLS}[kind]
    alphas = (255, 128, 77, 1, 0, 254)
    rows, k = [], 0
    for f, (w, h) in enumerate(sizes):
        for x, y, rw, rh in rects_for(w, h):
            rows.append((f, x, y, rw, rh, kind, args[k % len(args)], colour(k, alphas[k % len(alphas)])))
            k += 1
    return rows


# ---- every format x every kind -------------------------------------------------------------------------------------------
def _format_cases():
    for fmt in am.FORMATS:
        for kind in KINDS:
            for b in BATCHES:
                yield fmt, kind, b
            if fmt in ODD_OK:
                yield fmt, kind, "odd"


@pytest.mark.parametrize("fmt,kind,batch", list(_format_cases()), ids=lambda v: str(v))
def test_every_format_and_kind(vali, gpu, ann, fmt, kind, batch):
    sizes = ODD_BATCH if batch == "odd" else BATCHES[batch]
    rows = rows_for(KINDS[kind], sizes)
    drawn = check(vali, gpu, ann, fmt, sizes, rows)
    assert len(drawn) >= len(rows) // 2           # the set holds rows that miss on purpose, not mostly


# ---- order -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["NV12", "RGB", "YUV444"])
def test_marks_are_applied_in_row_order(vali, gpu, ann, fmt):
    sizes = [(T, T)]
    rows = [(0, 0, 0, T, T, am.FILL, 0, am.pack_colour(250, 20, 30, 120)),
            (0, 8, 8, 40, 40, am.PIXELATE, 16, 0),
            (0, 4, 4, 50, 50, am.BOX, 6, am.pack_colour(10, 240, 90, 200))]
    results = []
    for order in (rows, rows[::-1]):
        surfs, hosts = make_frames(vali, gpu, fmt, sizes, seed=3)
        assert ann.RunBatch(ann.PrepareBatch(surfs), device_marks(order, gpu))[0]
        assert am.apply(hosts, fmt, sizes, order, pm.matrices()[ROWS_601]) == [0, 1, 2]
        got = download(vali, gpu, surfs[0])
        assert np.array_equal(got, hosts[0])
        results.append(got)
    assert not np.array_equal(results[0], results[1])


# ---- skipped rows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["NV12", "BGR"])
def test_skipped_rows_change_nothing(vali, gpu, ann, fmt):
    sizes = [(T + 2, T + 2), (T - 2, T - 2)]
    real = [(0, 3, 5, 30, 20, am.FILL, 0, colour(1, 130)), (1, 10, 10, 30, 30, am.PIXELATE, 8, 0),
            (0, 20, 2, 44, 60, am.BOX, 3, colour(2)), (1, -4, 30, 90, 9, am.FILL, 0, colour(3, 60))]
    c = colour(9)
    skipped = [(0, 0, 0, 20, 20, 0, 1, c), (0, 0, 0, 20, 20, 7, 1, c), (-1, 0, 0, 20, 20, am.FILL, 0, c),
               (2, 0, 0, 20, 20, am.FILL, 0, c), (0, 0, 0, 0, 20, am.FILL, 0, c), (0, 0, 0, 20, 20, am.PIXELATE, 5, c),
               (0, 0, 0, 20, 20, am.BOX, 0, c), (1, 0, 0, 20, -3, am.FILL, 0, c), (0, 0, 0, 20, 20, -1, 4, c)]
    rows = []
    for i in range(len(skipped)):
        rows.append(skipped[i])
        rows.append(real[i % len(real)])
    surfs, hosts = make_frames(vali, gpu, fmt, sizes, seed=4)
    assert ann.RunBatch(ann.PrepareBatch(surfs), device_marks(rows, gpu))[0]
    only_real = [r for r in rows if r in real]
    assert len(am.apply(hosts, fmt, sizes, only_real, pm.matrices()[ROWS_601])) == len(only_real)
    for i, s in enumerate(surfs):
        assert np.array_equal(download(vali, gpu, s), hosts[i]), i


# ---- nothing else is written ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", am.FORMATS)
def test_pitched_surfaces_keep_their_padding_and_unnamed_frames_their_bytes(vali, gpu, ann, fmt):
    from vali_amd._native import shim

    sizes = [(T + 2, T + 6), (T - 2, T - 2), (T + 2, T + 2)]
    surfs = [vali.Surface.Make(getattr(vali, fmt), w, h, gpu) for w, h in sizes]
    stream = ann.Stream
    for s in surfs:
        for p in s._planes:
            shim.memset2d_async(gpu, p.GpuMem, p.Pitch, 0x5A, p.Pitch, p.Height, stream)
    shim.stream_sync(gpu, stream)
    hosts = []
    for i, (s, (w, h)) in enumerate(zip(surfs, sizes)):
        hosts.append(am.noise_frame(fmt, w, h, 50 + i))
        assert vali.PyFrameUploader(gpu).Run(hosts[i], s)[0]
    rows = [r for r in rows_for(am.FILL, sizes) + rows_for(am.PIXELATE, sizes) + rows_for(am.BOX, sizes) if r[0] != 1]
    assert ann.RunBatch(ann.PrepareBatch(surfs), device_marks(rows, gpu))[0]
    before1 = hosts[1].copy()
    am.apply(hosts, fmt, sizes, rows, pm.matrices()[ROWS_601])
    assert np.array_equal(hosts[1], before1)
    for i, s in enumerate(surfs):
        assert np.array_equal(download(vali, gpu, s), hosts[i]), i
        for p in s._planes:
            raw = np.zeros((p.Height, p.Pitch), np.uint8)
            hp, _, _ = shim.buffer_info(raw, True)
            shim.memcpy2d_async(gpu, hp, p.Pitch, p.GpuMem, p.Pitch, p.Pitch, p.Height, 1, stream)
            shim.stream_sync(gpu, stream)
            used = p.Width * p.ElemSize
            assert p.Pitch > used
            assert (raw[:, used:] == 0x5A).all(), i


@pytest.mark.parametrize("fmt", ["NV12", "RGB", "BGR", "RGB_PLANAR"])
def test_views_at_odd_addresses_and_the_canary_around_them(vali, gpu, ann, fmt):
    """from_dlpack views cut out of a larger canary-filled tensor at odd byte offsets and odd pitches"""
    sizes = [(T + 2, T + 6), (2 * T + 2, T - 2), (T - 2, T + 2)]
    rows = [r for r in rows_for(am.FILL, sizes) + rows_for(am.PIXELATE, sizes) + rows_for(am.BOX, sizes) if r[0] != 2]
    marks = device_marks(rows, gpu)
    for x0, extra in ((3, 9), (1, 1), (0, 7)):
        bufs, views, hosts = [], [], []
        for i, (w, h) in enumerate(sizes):
            (prows, cols), = am.plane_shapes(fmt, w, h)
            pitch = (cols + x0 + extra) | 1
            buf = torch.full((prows + 4, pitch), 0xA5, dtype=torch.uint8, device=f"cuda:{gpu}")
            hosts.append(am.noise_frame(fmt, w, h, 70 + i))
            buf[2:2 + prows, x0:x0 + cols] = torch.from_numpy(hosts[i].reshape(prows, cols)).to(buf.device)
            bufs.append(buf)
            views.append(buf[2:2 + prows, x0:x0 + cols])
        torch.cuda.synchronize()
        surfs = [vali.Surface.from_dlpack(v, getattr(vali, fmt)) for v in views]
        assert [(s.Width, s.Height) for s in surfs] == sizes
        assert ann.RunBatch(ann.PrepareBatch(surfs), marks)[0]
        untouched = hosts[2].copy()
        am.apply(hosts, fmt, sizes, rows, pm.matrices()[ROWS_601])
        assert np.array_equal(hosts[2], untouched)
        for i, (w, h) in enumerate(sizes):
            (prows, cols), = am.plane_shapes(fmt, w, h)
            buf = bufs[i].cpu().numpy()
            assert np.array_equal(buf[2:2 + prows, x0:x0 + cols].reshape(-1), hosts[i]), (x0, i)
            buf[2:2 + prows, x0:x0 + cols] = 0xA5
            assert (buf == 0xA5).all(), (x0, i, np.argwhere(buf != 0xA5)[:4])


# ---- colour ----------------------------------------------------------------------------------------------------------------
def _colour_lattice():
    """4096 colours: the corners of the cube, a lattice through it, and near-ties of the four matrices (Y close to k + 0.5)"""
    cols = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)]
    k = np.arange(4096 - len(cols))
    lattice = np.stack([(k * 37) % 256, (k * 101 + 255) % 256, (k * 17 + (k // 256) * 85) % 256], -1)
    cols += [tuple(int(v) for v in c) for c in lattice]
    found = 0
    for name, rows in pm.matrices().items():
        m = np.asarray(rows, np.float64)
        rng = np.random.default_rng(len(name))
        c = rng.integers(0, 256, (20000, 3))
        y = c @ m[0, :3] + m[0, 3]
        near = np.argsort(np.abs(y - np.floor(y) - 0.5))[:64]
        for idx in near:
            cols[8 + found] = tuple(int(v) for v in c[idx])
            found += 1
    return np.asarray(cols, np.uint8)


@pytest.mark.parametrize("matrix", ["601_JPEG", "601_MPEG", "709_JPEG", "709_MPEG"])
@pytest.mark.parametrize("fmt", am.YUV)
def test_colours_equal_the_postprocessor(vali, gpu, ann, fmt, matrix):
    w, h = 8192, 2
    cols = _colour_lattice()
    cc = pm.cc_ctx_of(vali, matrix)
    rows = [(0, 2 * i, 0, 2, 2, am.FILL, 0, am.pack_colour(*(int(v) for v in cols[i]))) for i in range(4096)]
    frame = vali.Surface.Make(getattr(vali, fmt), w, h, gpu)
    assert vali.PyFrameUploader(gpu).Run(np.zeros(frame.HostSize, np.uint8), frame)[0]
    ok, info = ann.RunBatch(ann.PrepareBatch([frame]), device_marks(rows, gpu), cc)
    assert ok, info
    px = np.repeat(cols, 2, axis=0)                                     # (8192, 3)
    t = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(px.T[None, :, None, :], (1, 3, h, w)))).to(f"cuda:{gpu}")
    torch.cuda.synchronize()
    want = vali.Surface.Make(getattr(vali, fmt), w, h, gpu)
    post = vali.PySurfacePostprocessor(gpu)
    ok, info = post.RunTensorBatch(post.PrepareTensorBatch(t, [want]), cc_ctx=cc)
    assert ok, info
    assert np.array_equal(download(vali, gpu, frame), download(vali, gpu, want))


@pytest.mark.parametrize("fmt", am.YUV)
def test_an_unsupported_cc_ctx_draws_nothing(vali, gpu, ann, fmt):
    sizes = [(T, T)]
    surfs, hosts = make_frames(vali, gpu, fmt, sizes, seed=8)
    cc = vali.ColorspaceConversionContext(vali.ColorSpace.UNSPEC, vali.ColorRange.JPEG)
    ok, info = ann.RunBatch(ann.PrepareBatch(surfs), device_marks([(0, 0, 0, T, T, am.FILL, 0, colour(1))], gpu), cc)
    assert (ok, info) == (False, vali.TaskExecInfo.UNSUPPORTED_FMT_CONV_PARAMS)
    assert np.array_equal(download(vali, gpu, surfs[0]), hosts[0])


def test_cc_ctx_is_ignored_for_rgb(vali, gpu, ann):
    sizes = [(T, T)]
    rows = [(0, 5, 5, 20, 20, am.FILL, 0, colour(1, 99))]
    surfs, hosts = make_frames(vali, gpu, "RGB", sizes, seed=8)
    cc = vali.ColorspaceConversionContext(vali.ColorSpace.UNSPEC, vali.ColorRange.UDEF)
    assert ann.RunBatch(ann.PrepareBatch(surfs), device_marks(rows, gpu), cc)[0]
    am.apply(hosts, "RGB", sizes, rows)
    assert np.array_equal(download(vali, gpu, surfs[0]), hosts[0])


# ---- random ----------------------------------------------------------------------------------------------------------------
def random_rows(sizes, count, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(count):
        f = int(rng.integers(0, len(sizes)))
        w, h = sizes[f]
        x, y = int(rng.integers(-(w // 4), w)), int(rng.integers(-(h // 4), h))
        rw, rh = int(rng.integers(1, max(w // 2, 1) + 1)), int(rng.integers(1, max(h // 2, 1) + 1))
        kind = int(rng.integers(1, 4))
        arg = int(rng.choice(am.CELLS)) if kind == am.PIXELATE else int(rng.integers(1, 12))
        rows.append((f, x, y, rw, rh, kind, arg, am.pack_colour(*(int(v) for v in rng.integers(0, 256, 4)))))
    return rows


@pytest.mark.parametrize("fmt", am.FORMATS)
def test_random_marks(vali, gpu, ann, fmt):
    sizes = [(T + 2, T + 2), (2 * T + 2, T + 6), (T - 2, T - 2)]
    rows = random_rows(sizes, 300, seed=am.FORMATS.index(fmt))
    drawn = check(vali, gpu, ann, fmt, sizes, rows, matrix="709_MPEG", seed=6)
    assert len(drawn) >= 0.8 * len(rows), len(drawn)      # a condition on the inputs: most rows meet their frame


# ---- sizes of M and N -------------------------------------------------------------------------------------------------------
def test_no_marks_and_no_frames(vali, gpu, ann):
    sizes = [(T + 2, T + 2)]
    surfs, hosts = make_frames(vali, gpu, "NV12", sizes, seed=9)
    empty = torch.zeros((0, 8), dtype=torch.int32, device=f"cuda:{gpu}")
    ok, info = ann.RunBatch(ann.PrepareBatch(surfs), empty)
    assert ok and info == vali.TaskExecInfo.SUCCESS
    assert ann.RunBatch(ann.PrepareBatch(surfs), [])[0]
    assert np.array_equal(download(vali, gpu, surfs[0]), hosts[0])
    none = ann.PrepareBatch([])
    assert len(none) == 0
    assert ann.RunBatch(none, empty)[0]
    assert ann.RunBatch(none, device_marks([(0, 0, 0, 4, 4, am.FILL, 0, 0)], gpu))[0]     # frame 0 is outside 0..-1: skipped


@pytest.mark.parametrize("fmt", ["NV12", "RGB"])
def test_4096_marks(vali, gpu, ann, fmt):
    sizes = [(2 * T + 2, T + 6), (T + 2, T + 2)]
    rows = random_rows(sizes, 4096, seed=11)
    drawn = check(vali, gpu, ann, fmt, sizes, rows, seed=7)
    assert len(drawn) >= 3000
    with pytest.raises(ValueError, match="4096"):
        ann.RunBatch(ann.PrepareBatch(make_frames(vali, gpu, fmt, sizes)[0]),
                     torch.zeros((4097, 8), dtype=torch.int32, device=f"cuda:{gpu}"))


# ---- host marks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["YUV420", "RGB_PLANAR"])
def test_host_marks_give_the_same_bytes(vali, gpu, ann, fmt):
    sizes = [(T + 2, T + 2), (2 * T + 2, T + 6)]
    rows = [r for r in random_rows(sizes, 120, seed=21) if am.resolve(r, len(sizes), sizes, fmt) is not None]
    rows.insert(5, (0, 1, 1, 5, 5, 0, 0, 0))                       # kind 0 and unknown kinds pass the host check
    rows.insert(9, (7, 1, 1, 5, 5, 9, 0, 0))
    a, _ = make_frames(vali, gpu, fmt, sizes, seed=12)
    b, _ = make_frames(vali, gpu, fmt, sizes, seed=12)
    assert ann.RunBatch(ann.PrepareBatch(a), device_marks(rows, gpu))[0]
    assert ann.RunBatch(ann.PrepareBatch(b), rows)[0]
    check(vali, gpu, ann, fmt, sizes, rows, seed=12, marks=rows)
    for sa, sb in zip(a, b):
        assert np.array_equal(download(vali, gpu, sa), download(vali, gpu, sb))


# ---- capture --------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay_with_rewritten_marks(vali, gpu):
    from vali_amd._native import shim

    fmt, sizes = "NV12", [(2 * T + 2, T + 6), (T + 2, T + 2)]
    stream = shim.stream_create(gpu)
    ann = vali.PySurfaceAnnotator(gpu, stream)
    sets = [random_rows(sizes, 64, seed=s) for s in (31, 32)]
    marks = device_marks(sets[0], gpu)
    surfs, _ = make_frames(vali, gpu, fmt, sizes, seed=13)
    ab = ann.PrepareBatch(surfs)
    cap = vali.StreamCapture(stream, gpu)
    with cap:
        with pytest.raises(RuntimeError, match="capturing"):
            ann.PrepareBatch(surfs)
        assert ann.RunBatchAsync(ab, marks)[0]
    cap.Keep(ab)
    for k in (0, 1):
        hosts = [am.noise_frame(fmt, w, h, 40 + k * 10 + i) for i, (w, h) in enumerate(sizes)]
        for s, host in zip(surfs, hosts):
            assert vali.PyFrameUploader(gpu).Run(host, s)[0]
        marks.copy_(device_marks(sets[k], gpu))                   # rewritten in place
        torch.cuda.synchronize()
        cap.Launch()
        shim.stream_sync(gpu, stream)
        am.apply(hosts, fmt, sizes, sets[k], pm.matrices()[ROWS_601])
        for i, s in enumerate(surfs):
            assert np.array_equal(download(vali, gpu, s), hosts[i]), (k, i)
