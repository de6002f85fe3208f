"""PySemanticPainter on the GPU against tests/semantic_model.py, bit for bit: frames and labels.

The fixtures are those of tests/semantic_cases.py (tests/test_semantic_host.py checks their conditions on the CPU): two
frames of 96 x 80 and 70 x 50 -- several tiles, partial tiles, a ragged right edge -- a letterbox that upsamples and a zoomed
crop whose region is smaller than its frame, starts at odd coordinates and, with fine logits, takes the kernel's direct
path."""
import numpy as np
import pytest

import annotate_model as am
import postproc_model as pm
import semantic_cases as sc
import semantic_model as sm
from test_gpu_annotate import device_marks, download, make_frames

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ROWS_601 = "601_JPEG"
DT = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
DTS = list(DT)
COLOURS = sc.palette(7)          # fewer than most C: classes share colours


@pytest.fixture(scope="module")
def sp(vali, gpu):
    return vali.PySemanticPainter(gpu)


def to_device(host, dtype, gpu):
    t = torch.from_numpy(np.ascontiguousarray(host)).to(f"cuda:{gpu}").to(DT[dtype])
    assert np.array_equal(t.float().cpu().numpy(), host, equal_nan=True)       # the fixture is exact in its dtype
    return t


def sliced_head(host, dtype, gpu):
    """the logits as a slice of a larger head: c and y strides larger than dense, a non-zero offset"""
    n, c, hs, ws = host.shape
    big = torch.full((n, c + 3, hs + 2, ws + 5), 1e4, dtype=DT[dtype], device=f"cuda:{gpu}")
    big[:, 2:2 + c, 1:1 + hs, 3:3 + ws] = to_device(host, dtype, gpu)
    view = big[:, 2:2 + c, 1:1 + hs, 3:3 + ws]
    assert not view.is_contiguous() and view.stride() == ((c + 3) * (hs + 2) * (ws + 5), (hs + 2) * (ws + 5), ws + 5, 1)
    return view


def label_surfaces(vali, gpu, sizes):
    """Y surfaces of the frames' sizes holding 0x5A: every pixel has to be rewritten"""
    out = []
    for w, h in sizes:
        s = vali.Surface.Make(vali.Y, w, h, gpu)
        assert vali.PyFrameUploader(gpu).Run(np.full(w * h, 0x5A, np.uint8), s)[0]
        out.append(s)
    return out


def compare(vali, gpu, surfs, hosts, what):
    for i, s in enumerate(surfs):
        got = download(vali, gpu, s)
        want = np.asarray(hosts[i]).reshape(-1)
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{what} {i} {sc.SIZES[i]}: {bad.size} bytes differ, first at {bad[:6]}: "
                                 f"got {got[bad[:6]]}, want {want[bad[:6]]}")


def check(vali, gpu, sp, fmt, c=19, size=(24, 20), dtype="float32", alpha=128, rects=sc.RECTS, colours=COLOURS,
          labels=True, seed=0, logits=None, expand=False, sliced=False, dev_args=False):
    """paint fresh noise frames and compare every frame and label surface with the model; returns (the model's label
    maps, the frames before, the frames after)"""
    ws, hs = size
    host = sc.logits(c, ws, hs, dtype, seed=seed) if logits is None else logits
    if expand:
        host = host[:1]
    lt = sliced_head(host, dtype, gpu) if sliced else to_device(host, dtype, gpu)
    if expand:
        lt = lt.expand(len(sc.SIZES), -1, -1, -1)
        assert lt.stride(0) == 0
    surfs, hosts = make_frames(vali, gpu, fmt, sc.SIZES, seed)
    before = [h.copy() for h in hosts]
    lab = label_surfaces(vali, gpu, sc.SIZES) if labels else None
    sb = sp.Prepare(surfs, lt, lab, net_size=sc.NET)
    r, col = rects, colours
    if dev_args:
        r = torch.tensor(np.asarray(rects, np.int32), dtype=torch.int32, device=f"cuda:{gpu}")
        col = torch.tensor(np.asarray(colours, np.int32), dtype=torch.int32, device=f"cuda:{gpu}")
        torch.cuda.synchronize()
    ok, info = sp.Run(sb, r, col, alpha=alpha, cc_ctx=pm.cc_ctx_of(vali, ROWS_601))
    assert ok and info == vali.TaskExecInfo.SUCCESS, info
    maps = sm.apply(hosts, fmt, sc.SIZES, host, rects, colours, alpha, sc.NET, pm.matrices()[ROWS_601])
    compare(vali, gpu, surfs, hosts, ("frame", fmt, c, size, dtype))
    if labels:
        compare(vali, gpu, lab, maps, ("labels", fmt, c, size, dtype))
    return maps, before, hosts


def paths(size):
    """the kernel's path for every pass of both frames, by the model's footprint rule"""
    return [set(sm.tile_paths(s, r, size[1], size[0], sc.NET).values()) for s, r in zip(sc.SIZES, sc.RECTS)]


# ---- both logit paths, every format x dtype instantiation ---------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(sc.LOGIT_SIZES)), ids=[f"{w}x{h}" for w, h in sc.LOGIT_SIZES])
@pytest.mark.parametrize("fi", range(len(am.FORMATS)), ids=am.FORMATS)
def test_every_format_and_dtype_on_both_paths(vali, gpu, sp, fi, si):
    size = sc.LOGIT_SIZES[si]
    want = [{"staged"}, {"direct"}] if size == (160, 120) else [{"staged"}, {"staged"}]
    assert paths(size) == want
    maps, before, after = check(vali, gpu, sp, am.FORMATS[fi], size=size, dtype=DTS[(fi + si) % 3], seed=fi)
    for m, b, a in zip(maps, before, after):
        assert len(set(np.unique(m).tolist()) - {255}) >= 3          # several classes are on every frame
        assert (a != b).mean() > 0.05


@pytest.mark.parametrize("size", sc.SWITCH_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt,dtype", [("NV12", "float16"), ("RGB", "float32")])
def test_either_side_of_the_switch_over(vali, gpu, sp, fmt, dtype, size):
    assert paths(size)[1] == ({"staged"} if size == sc.SWITCH_SIZES[0] else {"direct"})
    check(vali, gpu, sp, fmt, size=size, dtype=dtype, seed=1)


@pytest.mark.parametrize("c", sc.CS)
@pytest.mark.parametrize("fmt,dtype,size", [("NV12", "float16", (24, 20)), ("RGB", "bfloat16", (16, 16)),
                                            ("YUV420", "float32", (160, 120))])
def test_every_c(vali, gpu, sp, fmt, dtype, size, c):
    maps, _, _ = check(vali, gpu, sp, fmt, c=c, size=size, dtype=dtype, alpha=None, seed=2)
    if c == 1:
        assert set(np.unique(maps[0]).tolist()) == {0, 1}


# ---- colours and alpha -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["NV12", "YUV444", "BGR"])
def test_the_colours_own_alpha_leaves_a_class_with_alpha_0_alone(vali, gpu, sp, fmt):
    maps, before, after = check(vali, gpu, sp, fmt, c=3, alpha=None, colours=sc.PALETTE_OWN_ALPHA, seed=3)
    if fmt == "YUV444":
        for m, b, a in zip(maps, before, after):
            w, h = m.shape[1], m.shape[0]
            same = a.reshape(3, h, w) == b.reshape(3, h, w)
            assert same[:, m == 0].all() and not same[:, m == 2].all()


@pytest.mark.parametrize("alpha", [0, 1, 255])
def test_an_alpha_override(vali, gpu, sp, alpha):
    check(vali, gpu, sp, "YUV420", alpha=alpha, colours=sc.PALETTE_OWN_ALPHA, seed=4)


def test_device_rects_and_colours(vali, gpu, sp):
    check(vali, gpu, sp, "NV12", dev_args=True, seed=5)
    check(vali, gpu, sp, "RGB_PLANAR", dev_args=True, alpha=255, size=(160, 120), seed=5)


def test_host_colours_that_change_between_runs(vali, gpu, sp):
    fmt, host = "RGB", sc.logits(5, 24, 20)
    surfs, hosts = make_frames(vali, gpu, fmt, sc.SIZES, seed=6)
    sb = sp.Prepare(surfs, to_device(host, "float32", gpu), net_size=sc.NET)
    for colours in (sc.palette(5, 1), sc.palette(2, 2), sc.palette(5, 1)):
        assert sp.Run(sb, sc.RECTS, colours, alpha=100)[0]
        sm.apply(hosts, fmt, sc.SIZES, host, sc.RECTS, colours, 100, sc.NET)
        compare(vali, gpu, surfs, hosts, ("frame", len(colours)))


# ---- labels only, paint only, skipped frames, extreme records, non-finite logits -------------------------------------------
@pytest.mark.parametrize("fmt", ["NV12", "RGB"])
def test_labels_only_leaves_the_frames_alone(vali, gpu, sp, fmt):
    _, before, after = check(vali, gpu, sp, fmt, colours=None, seed=7)
    assert all(np.array_equal(b, a) for b, a in zip(before, after))


@pytest.mark.parametrize("fmt", ["YUV420", "BGR"])
def test_paint_only(vali, gpu, sp, fmt):
    check(vali, gpu, sp, fmt, labels=False, seed=8)


@pytest.mark.parametrize("fmt", ["NV12", "RGB"])
def test_a_record_with_dst_w_0_leaves_its_frame_alone_and_its_labels_255(vali, gpu, sp, fmt):
    maps, before, after = check(vali, gpu, sp, fmt, rects=sc.RECTS_DST_W_0, seed=9)
    assert (maps[1] == 255).all() and np.array_equal(before[1], after[1]) and not np.array_equal(before[0], after[0])


@pytest.mark.parametrize("fmt", ["NV12", "RGB_PLANAR"])
def test_records_with_int32_extremes(vali, gpu, sp, fmt):
    maps, _, _ = check(vali, gpu, sp, fmt, rects=sc.EXTREME_RECTS, seed=10)
    assert (maps[0][3:, :44] != 255).all() and (maps[0][:, 44:] == 255).all() and (maps[0][:3] == 255).all()
    assert (maps[1][:39, 8:] != 255).all() and (maps[1][39:] == 255).all() and (maps[1][:, :8] == 255).all()
    maps, before, after = check(vali, gpu, sp, fmt, rects=sc.EXTREME_RECTS_MISS, seed=10)
    assert all((m == 255).all() for m in maps) and all(np.array_equal(b, a) for b, a in zip(before, after))


@pytest.mark.parametrize("dtype", DTS)
@pytest.mark.parametrize("fmt,size", [("NV12", (24, 20)), ("RGB", (160, 120))])
def test_nan_and_infinite_logits(vali, gpu, sp, fmt, size, dtype):
    host = sc.nonfinite_logits(6, size[0], size[1], dtype)
    maps, _, _ = check(vali, gpu, sp, fmt, c=6, size=size, dtype=dtype, logits=host, seed=11)
    assert not np.isin(maps[0], (1, 5)).any()          # the NaN and the -inf plane never win


def test_an_all_nan_head_is_class_0(vali, gpu, sp):
    maps, _, _ = check(vali, gpu, sp, "NV12", c=3, logits=np.full((2, 3, 20, 24), np.nan, np.float32), seed=12)
    assert set(np.unique(maps[0]).tolist()) == {0} and set(np.unique(maps[1]).tolist()) == {0, 255}


# ---- strides ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_broadcast_logits_and_a_sliced_head(vali, gpu, sp, dtype):
    check(vali, gpu, sp, "NV12", dtype=dtype, expand=True, seed=13)
    check(vali, gpu, sp, "BGR", dtype=dtype, sliced=True, seed=13)
    check(vali, gpu, sp, "YUV420", dtype=dtype, size=(160, 120), sliced=True, expand=True, seed=13)


# ---- the annotator gives the same bytes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", am.FORMATS)
def test_the_annotator_stamps_the_same_bytes_from_the_models_atlas(vali, gpu, sp, fmt):
    host = sc.logits(19, 24, 20)
    a, hosts = make_frames(vali, gpu, fmt, sc.SIZES, seed=14)
    b, _ = make_frames(vali, gpu, fmt, sc.SIZES, seed=14)
    sb = sp.Prepare(a, to_device(host, "float32", gpu), net_size=sc.NET)
    assert sp.Run(sb, sc.RECTS, COLOURS, alpha=128, cc_ctx=pm.cc_ctx_of(vali, ROWS_601))[0]
    maps = sm.apply(hosts, fmt, sc.SIZES, host, sc.RECTS, COLOURS, 128, sc.NET, pm.matrices()[ROWS_601])
    atlas, marks = sm.stamp_atlas(maps, COLOURS, 128)
    at = torch.from_numpy(atlas).to(f"cuda:{gpu}")
    torch.cuda.synchronize()
    ann = vali.PySurfaceAnnotator(gpu)
    assert ann.RunBatch(ann.PrepareBatch(b), device_marks(marks, gpu), pm.cc_ctx_of(vali, ROWS_601),
                        atlas=vali.Surface.from_dlpack(at, vali.Y))[0]
    for i, (sa, sb_) in enumerate(zip(a, b)):
        got = download(vali, gpu, sa)
        assert np.array_equal(got, download(vali, gpu, sb_)) and np.array_equal(got, hosts[i]), (fmt, i)


# ---- nothing else is written ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["NV12", "RGB", "BGR", "RGB_PLANAR"])
def test_frames_and_labels_at_odd_addresses_and_the_canary_around_them(vali, gpu, sp, fmt):
    host = sc.logits(19, 24, 20)
    lt = to_device(host, "float32", gpu)

    def guarded(rows, cols, x0, extra, fill):
        pitch = (cols + x0 + extra) | 1
        buf = torch.full((rows + 4, pitch), 0xA5, dtype=torch.uint8, device=f"cuda:{gpu}")
        buf[2:2 + rows, x0:x0 + cols] = fill
        return buf, buf[2:2 + rows, x0:x0 + cols]

    for x0, extra in ((3, 9), (1, 1)):
        hosts = sc.noise_frames(fmt, seed=15)
        bufs, views, lbufs, lviews = [], [], [], []
        for i, (w, h) in enumerate(sc.SIZES):
            (prows, cols), = am.plane_shapes(fmt, w, h)
            buf, view = guarded(prows, cols, x0, extra, torch.from_numpy(hosts[i].reshape(prows, cols)).to(f"cuda:{gpu}"))
            bufs.append(buf), views.append(view)
            buf, view = guarded(h, w, x0 + 2, extra, 0x5A)
            lbufs.append(buf), lviews.append(view)
        torch.cuda.synchronize()
        surfs = [vali.Surface.from_dlpack(v, getattr(vali, fmt)) for v in views]
        labs = [vali.Surface.from_dlpack(v, vali.Y) for v in lviews]
        assert surfs[0].PixelPtr(0) % 2 == 1 and surfs[0].Pitch % 16 and labs[0].Pitch % 16
        sb = sp.Prepare(surfs, lt, labs, net_size=sc.NET)
        assert sp.Run(sb, sc.RECTS, COLOURS, alpha=128, cc_ctx=pm.cc_ctx_of(vali, ROWS_601))[0]
        maps = sm.apply(hosts, fmt, sc.SIZES, host, sc.RECTS, COLOURS, 128, sc.NET, pm.matrices()[ROWS_601])
        for i, (w, h) in enumerate(sc.SIZES):
            (prows, cols), = am.plane_shapes(fmt, w, h)
            for buf, r, c, xs, want in ((bufs[i].cpu().numpy(), prows, cols, x0, hosts[i]),
                                        (lbufs[i].cpu().numpy(), h, w, x0 + 2, maps[i])):
                assert np.array_equal(buf[2:2 + r, xs:xs + c].reshape(-1), np.asarray(want).reshape(-1)), (x0, i)
                buf[2:2 + r, xs:xs + c] = 0xA5
                assert (buf == 0xA5).all(), (x0, i, np.argwhere(buf != 0xA5)[:4])


@pytest.mark.parametrize("fmt", ["NV12", "YUV420", "YUV444"])
def test_pitched_planar_frames_keep_their_padding_and_a_tile_outside_the_region_its_bytes(vali, gpu, sp, fmt):
    from vali_amd._native import shim

    host = sc.logits(19, 16, 16)
    surfs = [vali.Surface.Make(getattr(vali, fmt), w, h, gpu) for w, h in sc.SIZES]
    stream = sp.Stream
    for s in surfs:
        for p in s._planes:
            shim.memset2d_async(gpu, p.GpuMem, p.Pitch, 0x5A, p.Pitch, p.Height, stream)
    shim.stream_sync(gpu, stream)
    hosts = sc.noise_frames(fmt, seed=16)
    for s, h in zip(surfs, hosts):
        assert vali.PyFrameUploader(gpu).Run(h, s)[0]
    before = hosts[1].copy()
    sb = sp.Prepare(surfs, to_device(host, "float32", gpu), net_size=sc.NET)
    assert sp.Run(sb, sc.RECTS, COLOURS, alpha=200, cc_ctx=pm.cc_ctx_of(vali, ROWS_601))[0]
    sm.apply(hosts, fmt, sc.SIZES, host, sc.RECTS, COLOURS, 200, sc.NET, pm.matrices()[ROWS_601])
    # frame 1's second tile (columns 64 .. 69) holds no region pixel
    luma = lambda flat: flat[:70 * 50].reshape(50, 70)
    assert np.array_equal(luma(hosts[1])[:, 64:], luma(before)[:, 64:]) and not np.array_equal(hosts[1], before)
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


# ---- capture ----------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay_after_everything_was_rewritten_in_place(vali, gpu):
    from vali_amd._native import shim

    fmt, dev = "NV12", f"cuda:{gpu}"
    stream = shim.stream_create(gpu)
    sp = vali.PySemanticPainter(gpu, stream)
    sets = [(sc.logits(19, 24, 20, seed=0), sc.RECTS), (sc.logits(19, 24, 20, seed=1), sc.RECTS_DST_W_0),
            (sc.logits(19, 24, 20, seed=2), list(reversed(sc.RECTS)))]
    lt = to_device(sets[0][0], "float32", gpu)
    rects = torch.tensor(np.asarray(sc.RECTS, np.int32), dtype=torch.int32, device=dev)
    colours = torch.tensor(np.asarray(COLOURS, np.int32), dtype=torch.int32, device=dev)
    surfs, _ = make_frames(vali, gpu, fmt, sc.SIZES, seed=17)
    lab = label_surfaces(vali, gpu, sc.SIZES)
    torch.cuda.synchronize()
    sb = sp.Prepare(surfs, lt, lab, net_size=sc.NET)
    cap = vali.StreamCapture(stream, gpu)
    with cap:
        assert sp.RunAsync(sb, rects, colours, alpha=128)[0]
    cap.Keep(sb)
    for k, (host, rc) in enumerate(sets):
        hosts = sc.noise_frames(fmt, seed=20 + k)
        for s, h in zip(surfs, hosts):
            assert vali.PyFrameUploader(gpu).Run(h, s)[0]
        lt.copy_(to_device(host, "float32", gpu))                       # rewritten in place
        rects.copy_(torch.tensor(np.asarray(rc, np.int32), dtype=torch.int32, device=dev))
        torch.cuda.synchronize()
        cap.Launch()
        shim.stream_sync(gpu, stream)
        maps = sm.apply(hosts, fmt, sc.SIZES, host, rc, COLOURS, 128, sc.NET, pm.matrices()[ROWS_601])
        compare(vali, gpu, surfs, hosts, ("replay", k))
        compare(vali, gpu, lab, maps, ("replayed labels", k))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_prepare_and_run_say_what_is_wrong(vali, gpu, sp):
    lt = to_device(sc.logits(5, 16, 16), "float32", gpu)
    surfs, _ = make_frames(vali, gpu, "NV12", sc.SIZES, seed=18)
    lab = label_surfaces(vali, gpu, sc.SIZES)
    with pytest.raises(ValueError, match="x stride"):
        sp.Prepare(surfs, lt.transpose(2, 3), net_size=sc.NET)
    with pytest.raises(ValueError, match="3 surfaces"):
        sp.Prepare(surfs + surfs[:1], lt, net_size=sc.NET)
    with pytest.raises(ValueError, match="dtype"):
        sp.Prepare(surfs, lt.double(), net_size=sc.NET)
    with pytest.raises(ValueError, match="GPU"):
        sp.Prepare(surfs, lt.cpu(), net_size=sc.NET)
    with pytest.raises(ValueError, match="C = 256"):
        sp.Prepare(surfs, torch.zeros((2, 256, 4, 4), device=lt.device), net_size=sc.NET)
    with pytest.raises(ValueError, match="net_size"):
        sp.Prepare(surfs, lt, net_size=(0, 64))
    mixed = [surfs[0], vali.Surface.Make(vali.RGB, 70, 50, gpu)]
    with pytest.raises(ValueError, match="one format per batch"):
        sp.Prepare(mixed, lt, net_size=sc.NET)
    with pytest.raises(ValueError, match="labels: surface 1 is 96x80"):
        sp.Prepare(surfs, lt, [lab[0], lab[0]], net_size=sc.NET)
    with pytest.raises(ValueError, match="need Y"):
        sp.Prepare(surfs, lt, [lab[0], vali.Surface.Make(vali.RGB, 70, 50, gpu)], net_size=sc.NET)
    with pytest.raises(ValueError, match="labels: 1 surfaces"):
        sp.Prepare(surfs, lt, lab[:1], net_size=sc.NET)
    sb = sp.Prepare(surfs, lt, net_size=sc.NET)
    with pytest.raises(ValueError, match="labels"):
        sp.Run(sb, sc.RECTS, None)
    with pytest.raises(ValueError, match="rects"):
        sp.Run(sb, sc.RECTS[:1], COLOURS)
    with pytest.raises(ValueError, match="alpha"):
        sp.Run(sb, sc.RECTS, COLOURS, alpha=300)
    with pytest.raises(ValueError, match="SemanticBatch"):
        sp.Run(None, sc.RECTS, COLOURS)
    bad = vali.ColorspaceConversionContext(vali.ColorSpace.UNSPEC, vali.ColorRange.UDEF)
    if vali.PySurfacePostprocessor.Matrix(bad) is None:
        ok, info = sp.Run(sb, sc.RECTS, COLOURS, cc_ctx=bad)
        assert not ok and info == vali.TaskExecInfo.UNSUPPORTED_FMT_CONV_PARAMS
