"""MARK_STAMP on the GPU against tests/annotate_stamp_model.py, bit for bit.

Frames: two per batch, (2T + 2) x (T + 6) and (T + 2) x (T + 2) with T the kernel's tile side: several tiles, ragged right
and bottom edges, a tile of 2 columns.  The atlas is 97 x 45, a view at an odd byte offset inside a larger tensor whose
row pitch is no multiple of 16 and whose every other byte is 255: a read outside the atlas's area shows as wrong pixels."""
import numpy as np
import pytest

import annotate_model as am
import annotate_stamp_model as sm
import postproc_model as pm
from test_gpu_annotate import colour, device_marks, download, make_frames

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

T = am.TILE
SIZES = [(2 * T + 2, T + 6), (T + 2, T + 2)]
AW, AH = 97, 45
ROWS_601 = "601_JPEG"
uv = sm.pack_uv


def noise_atlas(aw=AW, ah=AH, seed=17):
    """noise with runs of 0 and of 255 in it"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (ah, aw), dtype=np.uint8)
    a[rng.random((ah, aw)) < 0.15] = 0
    a[rng.random((ah, aw)) < 0.15] = 255
    return a


def upload_atlas(vali, gpu, host, x0=3, extra=11):
    """(surface, the tensor it views): the atlas at an odd address inside a tensor of 255s with an odd pitch"""
    ah, aw = host.shape
    pitch = (aw + x0 + extra) | 1
    assert pitch % 16 and x0 % 2
    buf = torch.full((ah + 4, pitch), 255, dtype=torch.uint8, device=f"cuda:{gpu}")
    buf[2:2 + ah, x0:x0 + aw] = torch.from_numpy(host).to(buf.device)
    torch.cuda.synchronize()
    view = buf[2:2 + ah, x0:x0 + aw]
    surf = vali.Surface.from_dlpack(view, vali.Y)
    assert (surf.Width, surf.Height, surf.Pitch) == (aw, ah, pitch) and surf.PixelPtr(0) % 2 == 1
    return surf, buf


@pytest.fixture(scope="module")
def ann(vali, gpu):
    return vali.PySurfaceAnnotator(gpu)


@pytest.fixture(scope="module")
def atlas(vali, gpu):
    host = noise_atlas()
    surf, buf = upload_atlas(vali, gpu, host)
    return host, surf, buf


def compare(vali, gpu, surfs, hosts, fmt, sizes):
    for i, s in enumerate(surfs):
        got = download(vali, gpu, s)
        if not np.array_equal(got, hosts[i]):
            bad = np.flatnonzero(got != hosts[i])
            raise AssertionError(f"{fmt} frame {i} {sizes[i]}: {bad.size} bytes differ, first at {bad[:6]}: "
                                 f"got {got[bad[:6]]}, want {hosts[i][bad[:6]]}")


def check(vali, gpu, ann, fmt, rows, atlas, sizes=SIZES, matrix=ROWS_601, seed=0, marks=None):
    """draw `rows` on fresh noise frames with the atlas and compare every frame with the model; returns the rows drawn"""
    host_atlas, surf = atlas[0], atlas[1]
    surfs, hosts = make_frames(vali, gpu, fmt, sizes, seed)
    ab = ann.PrepareBatch(surfs)
    ok, info = ann.RunBatch(ab, device_marks(rows, gpu) if marks is None else marks, pm.cc_ctx_of(vali, matrix), atlas=surf)
    assert ok and info == vali.TaskExecInfo.SUCCESS, info
    drawn = sm.apply(hosts, fmt, sizes, rows, pm.matrices()[matrix], host_atlas)
    compare(vali, gpu, surfs, hosts, fmt, sizes)
    return drawn


def hand_picked():
    """(frame, x, y, w, h, u, v): see the names"""
    w0, h0 = SIZES[0]
    cases = {
        "inside one tile": (0, 5, 7, 20, 12, 10, 3),
        "across a tile corner": (0, T - 9, T - 7, 20, 12, 0, 0),
        "odd x and y": (0, 71, 9, 13, 11, 2, 2),
        "odd everything on the small frame": (1, 33, 21, 15, 9, 13, 7),
        "clipped left and top": (0, -7, -5, 30, 20, 5, 5),
        "past the right and bottom edge": (0, w0 - 10, h0 - 10, 30, 20, 1, 1),
        "the last two columns": (1, T - 3, 3, 30, 30, 0, 8),
        "width 1": (1, 33, 40, 1, 9, 9, 9),
        "height 1": (1, 3, 33, 40, 1, 30, 44),
        "width 17": (1, 3, 50, 17, 5, 40, 20),
        "the atlas's first column at odd x": (0, 21, 40, 33, 9, 0, 11),
        "the atlas's last columns": (0, 90, 30, 20, 12, AW - 20, AH - 12),
        "off the atlas's right and bottom": (1, 10, 4, 40, 30, AW - 17, AH - 15),
        "off the atlas's right, from its column 1": (0, 2, 50, 120, 6, 1, 40),
        "u >= AW": (0, 0, 0, 10, 10, AW, 0),
        "v >= AH": (0, 0, 0, 10, 10, 0, AH),
        "x = -2^31, w = 2^31 - 1": (0, -2**31, 3, 2**31 - 1, 9, 0, 0),
        "y = -2^31, h = 2^31 - 1": (1, 3, -2**31, 9, 2**31 - 1, 0, 0),
        "from -2^31 + 3 into the frame": (0, -2**31 + 3, 3, 2**31 - 1, 2**31 - 1, 3, 3),
        "the whole frame": (1, 0, 0, T + 2, T + 2, 20, 0),
        "huge, from inside": (0, 100, 50, 2**31 - 1, 2**31 - 1, 7, 9),
    }
    rows = []
    for k, (name, (f, x, y, w, h, u, v)) in enumerate(cases.items()):
        rows.append((f, x, y, w, h, sm.STAMP, uv(u, v), colour(k, (255, 128, 0)[k % 3])))
    # the first three again with the other alphas, so that each is drawn with 0, 128 and 255
    for k in range(3):
        for j in (1, 2):
            f, x, y, w, h, kind, arg, _ = rows[k]
            rows.append((1, x % 40, y % 40, w, h, kind, arg, colour(k + 30, (255, 128, 0)[(k + j) % 3])))
    return rows


# ---- hand-picked stamps --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", am.FORMATS)
def test_hand_picked_stamps(vali, gpu, ann, atlas, fmt):
    rows = hand_picked()
    drawn = check(vali, gpu, ann, fmt, rows, atlas)
    skipped = set(range(len(rows))) - set(drawn)
    assert skipped == {14, 15, 16, 17}, skipped          # u >= AW, v >= AH and the two that end at -1


@pytest.mark.parametrize("fmt", am.FORMATS)
def test_each_hand_picked_stamp_alone(vali, gpu, ann, atlas, fmt):
    """one call per stamp on the same frames: a wrong one is named, and no later stamp paints over it"""
    host_atlas, surf = atlas[0], atlas[1]
    surfs, hosts = make_frames(vali, gpu, fmt, SIZES, seed=2)
    ab = ann.PrepareBatch(surfs)
    for i, row in enumerate(hand_picked()):
        assert ann.RunBatch(ab, device_marks([row], gpu), atlas=surf)[0]
        sm.apply(hosts, fmt, SIZES, [row], pm.matrices()[ROWS_601], host_atlas)
        for k, s in enumerate(surfs):
            assert np.array_equal(download(vali, gpu, s), hosts[k]), (i, row, k)


@pytest.mark.parametrize("aw,ah", [(5, 3), (11, 4), (16, 2), (1, 1)])
@pytest.mark.parametrize("fmt", am.FORMATS)
def test_atlases_narrower_than_a_vector(vali, gpu, ann, fmt, aw, ah):
    """below 16 (packed RGB: 8) columns the kernel reads the atlas byte by byte"""
    host = noise_atlas(aw, ah, seed=aw) | 1
    small = (host, *upload_atlas(vali, gpu, host))
    rows = [(0, 3, 3, 40, 40, sm.STAMP, 0, colour(1)), (0, T - 2, T - 1, aw, ah, sm.STAMP, 0, colour(2, 128)),
            (1, 7, 9, 3, 2, sm.STAMP, uv(aw - 1, ah - 1), colour(3)), (1, -2, -1, 9, 9, sm.STAMP, uv(aw // 2, 0), colour(4, 200)),
            (1, T, T, 9, 9, sm.STAMP, 0, colour(5)), (0, 2 * T - 1, 5, 9, 9, sm.STAMP, 0, colour(6))]
    assert len(check(vali, gpu, ann, fmt, rows, small)) == len(rows)


# ---- identities ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", am.FORMATS)
def test_full_coverage_is_fill_on_the_gpu(vali, gpu, ann, fmt):
    host = np.full((AH, AW), 255, np.uint8)
    surf, _buf = upload_atlas(vali, gpu, host)
    rects = [(0, 4, 2, 60, 40), (0, T - 6, T - 8, 30, 14), (1, 0, 0, T + 2, 42), (1, 20, 30, 2, 2), (0, 100, 60, 92, 40)]
    assert all(k + w <= AW and k + h <= AH for k, (_, _, _, w, h) in enumerate(rects))     # each lies inside the atlas from (k, k)
    stamps =[(f, x, y, w, h, sm.STAMP, uv(k, k), colour(k, (255, 128, 77, 1, 0)[k])) for k, (f, x, y, w, h) in enumerate(rects)]
    fills = [(f, x, y, w, h, am.FILL, 0, c) for f, x, y, w, h, _, _, c in stamps]
    a, _ = make_frames(vali, gpu, fmt, SIZES, seed=3)
    b, hosts = make_frames(vali, gpu, fmt, SIZES, seed=3)
    assert ann.RunBatch(ann.PrepareBatch(a), device_marks(stamps, gpu), atlas=surf)[0]
    assert ann.RunBatch(ann.PrepareBatch(b), device_marks(fills, gpu))[0]
    am.apply(hosts, fmt, SIZES, fills, pm.matrices()[ROWS_601])
    for sa, sb, host_frame in zip(a, b, hosts):
        got = download(vali, gpu, sa)
        assert np.array_equal(got, download(vali, gpu, sb)) and np.array_equal(got, host_frame)


def stampless_rows(count, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(count):
        f = int(rng.integers(0, len(SIZES)))
        w, h = SIZES[f]
        kind = int(rng.integers(1, 4))
        arg = int(rng.choice(am.CELLS)) if kind == am.PIXELATE else int(rng.integers(1, 12))
        rows.append((f, int(rng.integers(-20, w + 10)), int(rng.integers(-20, h + 10)), int(rng.integers(1, 61)),
                     int(rng.integers(1, 61)), kind, arg, am.pack_colour(*(int(v) for v in rng.integers(0, 256, 4)))))
    return rows


@pytest.mark.parametrize("fmt", am.FORMATS)
def test_an_atlas_without_stamp_rows_changes_nothing(vali, gpu, ann, atlas, fmt):
    rows = stampless_rows(120, seed=5)
    a, _ = make_frames(vali, gpu, fmt, SIZES, seed=4)
    b, _ = make_frames(vali, gpu, fmt, SIZES, seed=4)
    marks = device_marks(rows, gpu)
    assert ann.RunBatch(ann.PrepareBatch(a), marks, atlas=atlas[1])[0]
    assert ann.RunBatch(ann.PrepareBatch(b), marks)[0]
    for sa, sb in zip(a, b):
        assert np.array_equal(download(vali, gpu, sa), download(vali, gpu, sb))
    check(vali, gpu, ann, fmt, rows, atlas, seed=4)


@pytest.mark.parametrize("fmt", ["NV12", "RGB"])
def test_a_stamp_row_without_an_atlas_draws_nothing(vali, gpu, ann, fmt):
    rows = [(0, 5, 5, 30, 30, sm.STAMP, 0, colour(1)), (1, 0, 0, 66, 66, sm.STAMP, uv(3, 3), colour(2, 128))]
    surfs, hosts = make_frames(vali, gpu, fmt, SIZES, seed=5)
    assert ann.RunBatch(ann.PrepareBatch(surfs), device_marks(rows, gpu))[0]
    assert ann.RunBatch(ann.PrepareBatch(surfs), rows)[0]                  # host rows: unknown kinds pass the check
    compare(vali, gpu, surfs, hosts, fmt, SIZES)


# ---- random ------------------------------------------------------------------------------------------------------------------
def random_rows(count, seed, kinds=(1, 2, 3, 4)):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(count):
        f = int(rng.integers(0, len(SIZES)))
        w, h = SIZES[f]
        x, y = int(rng.integers(-20, w + 10)), int(rng.integers(-20, h + 10))
        rw, rh = int(rng.integers(1, 61)), int(rng.integers(1, 61))
        kind = int(rng.choice(kinds))
        arg = {am.BOX: int(rng.integers(1, 12)), am.FILL: 0, am.PIXELATE: int(rng.choice(am.CELLS)),
               sm.STAMP: uv(int(rng.integers(0, AW + 3)), int(rng.integers(0, AH + 2)))}[kind]
        rows.append((f, x, y, rw, rh, kind, arg, am.pack_colour(*(int(v) for v in rng.integers(0, 256, 4)))))
    return rows


@pytest.mark.parametrize("fmt", am.FORMATS)
def test_random_rows_of_all_four_kinds(vali, gpu, ann, atlas, fmt):
    rows = random_rows(300, seed=40 + am.FORMATS.index(fmt))
    assert {r[5] for r in rows} == {1, 2, 3, 4}
    drawn = check(vali, gpu, ann, fmt, rows, atlas, matrix="709_MPEG", seed=6)
    assert len(drawn) >= 200, len(drawn)                 # a condition on the inputs: skips cannot hide a failure
    assert sum(rows[i][5] == sm.STAMP for i in drawn) >= 40


@pytest.mark.parametrize("fmt", ["NV12", "RGB"])
def test_4096_stamps(vali, gpu, ann, atlas, fmt):
    rows = random_rows(4096, seed=11, kinds=(4,))
    drawn = check(vali, gpu, ann, fmt, rows, atlas, seed=7)
    # a condition on the inputs, from their distributions: u < AW for 97 of 100 rows, v < AH for 45 of 47, and a position
    # from [-20, W + 10) with a size of 1 .. 60 meets a side of W with probability 1 - 13.5 / (W + 30) (10 starts beyond
    # it, 3.5 end before it on average): 0.97 * 0.957 * (0.916 * 0.865 + 0.859 * 0.859) / 2 = 0.71 of 4096 = 2910, with a
    # standard deviation of 29
    assert len(drawn) >= 2800


# ---- host marks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["YUV420", "RGB_PLANAR"])
def test_host_marks_give_the_same_bytes(vali, gpu, ann, atlas, fmt):
    rows = [r for r in random_rows(160, seed=21) if sm.resolve(r, len(SIZES), SIZES, fmt, atlas[0]) is not None]
    assert sum(r[5] == sm.STAMP for r in rows) >= 20
    a, _ = make_frames(vali, gpu, fmt, SIZES, seed=12)
    b, _ = make_frames(vali, gpu, fmt, SIZES, seed=12)
    assert ann.RunBatch(ann.PrepareBatch(a), device_marks(rows, gpu), atlas=atlas[1])[0]
    assert ann.RunBatch(ann.PrepareBatch(b), rows, atlas=atlas[1])[0]
    for sa, sb in zip(a, b):
        assert np.array_equal(download(vali, gpu, sa), download(vali, gpu, sb))
    check(vali, gpu, ann, fmt, rows, atlas, seed=12, marks=rows)
    with pytest.raises(ValueError, match="row 1: the stamp's origin"):
        ann.RunBatch(ann.PrepareBatch(a), [rows[0], (0, 0, 0, 5, 5, sm.STAMP, uv(AW, 0), 0)], atlas=atlas[1])


# ---- nothing else is written ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", am.FORMATS)
def test_pitched_frames_keep_their_padding(vali, gpu, ann, atlas, fmt):
    from vali_amd._native import shim

    surfs = [vali.Surface.Make(getattr(vali, fmt), w, h, gpu) for w, h in SIZES]
    stream = ann.Stream
    for s in surfs:
        for p in s._planes:
            shim.memset2d_async(gpu, p.GpuMem, p.Pitch, 0x5A, p.Pitch, p.Height, stream)
    shim.stream_sync(gpu, stream)
    hosts = [am.noise_frame(fmt, w, h, 50 + i) for i, (w, h) in enumerate(SIZES)]
    for s, host in zip(surfs, hosts):
        assert vali.PyFrameUploader(gpu).Run(host, s)[0]
    rows = hand_picked() + random_rows(60, seed=8)
    assert ann.RunBatch(ann.PrepareBatch(surfs), device_marks(rows, gpu), atlas=atlas[1])[0]
    sm.apply(hosts, fmt, SIZES, rows, pm.matrices()[ROWS_601], atlas[0])
    compare(vali, gpu, surfs, hosts, fmt, SIZES)
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
def test_frames_at_odd_addresses_and_the_canary_around_them(vali, gpu, ann, atlas, fmt):
    rows = hand_picked() + random_rows(60, seed=9, kinds=(4,))
    marks = device_marks(rows, gpu)
    for x0, extra in ((3, 9), (1, 1)):
        bufs, views, hosts = [], [], []
        for i, (w, h) in enumerate(SIZES):
            (prows, cols), = am.plane_shapes(fmt, w, h)
            pitch = (cols + x0 + extra) | 1
            buf = torch.full((prows + 4, pitch), 0xA5, dtype=torch.uint8, device=f"cuda:{gpu}")
            hosts.append(am.noise_frame(fmt, w, h, 70 + i))
            buf[2:2 + prows, x0:x0 + cols] = torch.from_numpy(hosts[i].reshape(prows, cols)).to(buf.device)
            bufs.append(buf)
            views.append(buf[2:2 + prows, x0:x0 + cols])
        torch.cuda.synchronize()
        surfs = [vali.Surface.from_dlpack(v, getattr(vali, fmt)) for v in views]
        assert ann.RunBatch(ann.PrepareBatch(surfs), marks, atlas=atlas[1])[0]
        sm.apply(hosts, fmt, SIZES, rows, pm.matrices()[ROWS_601], atlas[0])
        for i, (w, h) in enumerate(SIZES):
            (prows, cols), = am.plane_shapes(fmt, w, h)
            buf = bufs[i].cpu().numpy()
            assert np.array_equal(buf[2:2 + prows, x0:x0 + cols].reshape(-1), hosts[i]), (x0, i)
            buf[2:2 + prows, x0:x0 + cols] = 0xA5
            assert (buf == 0xA5).all(), (x0, i, np.argwhere(buf != 0xA5)[:4])
    # the atlas and the bytes around it are as they were
    whole = atlas[2].cpu().numpy()
    assert np.array_equal(whole[2:2 + AH, 3:3 + AW], atlas[0])
    whole[2:2 + AH, 3:3 + AW] = 255
    assert (whole == 255).all()


# ---- capture --------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay_with_rewritten_marks_and_atlas(vali, gpu):
    from vali_amd._native import shim

    fmt = "NV12"
    stream = shim.stream_create(gpu)
    ann = vali.PySurfaceAnnotator(gpu, stream)
    sets = [random_rows(64, seed=s) for s in (31, 32)]
    atlases = [noise_atlas(seed=s) for s in (61, 62)]
    marks = device_marks(sets[0], gpu)
    surf, buf = upload_atlas(vali, gpu, atlases[0])
    surfs, _ = make_frames(vali, gpu, fmt, SIZES, seed=13)
    ab = ann.PrepareBatch(surfs)
    cap = vali.StreamCapture(stream, gpu)
    with cap:
        assert ann.RunBatchAsync(ab, marks, atlas=surf)[0]
    cap.Keep(ab)
    for k in (0, 1):
        hosts = [am.noise_frame(fmt, w, h, 40 + k * 10 + i) for i, (w, h) in enumerate(SIZES)]
        for s, host in zip(surfs, hosts):
            assert vali.PyFrameUploader(gpu).Run(host, s)[0]
        marks.copy_(device_marks(sets[k], gpu))                                       # rewritten in place
        buf[2:2 + AH, 3:3 + AW] = torch.from_numpy(atlases[k]).to(buf.device)           # ... and so is the atlas
        torch.cuda.synchronize()
        cap.Launch()
        shim.stream_sync(gpu, stream)
        sm.apply(hosts, fmt, SIZES, sets[k], pm.matrices()[ROWS_601], atlases[k])
        for i, s in enumerate(surfs):
            assert np.array_equal(download(vali, gpu, s), hosts[i]), (k, i)


# ---- labels ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["NV12", "BGR"])
def test_label_atlas_end_to_end(vali, gpu, ann, fmt):
    pytest.importorskip("PIL")
    labels = ["person", "dog 0.87", "kite"]
    la = vali.LabelAtlas(gpu, labels)
    host_atlas, rects = vali.render_labels(labels)
    assert la.labels == labels and np.array_equal(la.rects, rects)
    assert (la.surface.Width, la.surface.Height) == host_atlas.shape[::-1] and la.surface.Format == vali.Y
    # class ids and box corners stay on the GPU: the rows are gathered there
    dev = f"cuda:{gpu}"
    boxes = torch.tensor([[0, 9, 31, 50, 30, 0], [0, 70, 5, 40, 60, 2], [1, 3, 41, 50, 20, 1]], dtype=torch.int32, device=dev)
    r = torch.from_numpy(rects).to(dev)[boxes[:, 5].long()]
    marks = torch.zeros((3, 8), dtype=torch.int32, device=dev)
    marks[:, 0], marks[:, 1], marks[:, 2] = boxes[:, 0], boxes[:, 1], boxes[:, 2] - r[:, 3]
    marks[:, 3], marks[:, 4], marks[:, 5] = r[:, 2], r[:, 3], vali.MARK_STAMP
    marks[:, 6], marks[:, 7] = r[:, 0] | r[:, 1] << 16, vali.pack_colour(255, 255, 0)
    torch.cuda.synchronize()
    surfs, hosts = make_frames(vali, gpu, fmt, SIZES, seed=14)
    assert ann.RunBatch(ann.PrepareBatch(surfs), marks, atlas=la.surface)[0]
    rows = [tuple(int(v) for v in row) for row in marks.cpu().numpy()]
    assert sm.apply(hosts, fmt, SIZES, rows, pm.matrices()[ROWS_601], host_atlas) == [0, 1, 2]
    compare(vali, gpu, surfs, hosts, fmt, SIZES)
    assert not np.array_equal(hosts[0], am.noise_frame(fmt, *SIZES[0], 1400))       # something was drawn
