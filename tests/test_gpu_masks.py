"""PyInstanceMasker on the GPU against tests/mask_model.py, bit for bit.

The fixtures are those of tests/mask_cases.py (tests/test_mask_host.py checks on the CPU that every mask of them covers
5 to 95 % of its box): two frames of 96 x 80 and 70 x 50 -- several tiles, partial tiles, a ragged right edge -- four rows
each, a letterbox that upsamples and a zoomed crop that samples more coarsely than the prototypes."""
import numpy as np
import pytest

import annotate_model as am
import mask_cases as mc
import mask_model as mm
import postproc_model as pm
from test_gpu_annotate import device_marks, download, make_frames

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ROWS_601 = "601_JPEG"
DT = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
CLASSES = 3          # of the synthetic head the coefficients are sliced from


@pytest.fixture(scope="module")
def mk(vali, gpu):
    return vali.PyInstanceMasker(gpu)


def to_device(host, dtype, gpu):
    t = torch.from_numpy(np.ascontiguousarray(host)).to(f"cuda:{gpu}").to(DT[dtype])
    assert np.array_equal(t.float().cpu().numpy(), host, equal_nan=True)       # the fixture is exact in its dtype
    return t


def head_slice(host, dtype, gpu):
    """the coefficients as the last M channels of a YOLOv8-seg head (N, 4 + C + M, K), transposed without a copy"""
    n, k, m = host.shape
    pred = torch.full((n, 4 + CLASSES + m, k), 1e4, dtype=DT[dtype], device=f"cuda:{gpu}")
    pred[:, 4 + CLASSES:] = to_device(host, dtype, gpu).transpose(1, 2)
    view = pred[:, 4 + CLASSES:].transpose(1, 2)
    assert not view.is_contiguous() and view.stride() == ((4 + CLASSES + m) * k, 1, k)
    return view


def compare(vali, gpu, surfs, hosts, what):
    for i, s in enumerate(surfs):
        got = download(vali, gpu, s)
        if not np.array_equal(got, hosts[i]):
            bad = np.flatnonzero(got != hosts[i])
            raise AssertionError(f"{what} frame {i} {mc.SIZES[i]}: {bad.size} bytes differ, first at {bad[:6]}: "
                                 f"got {got[bad[:6]]}, want {hosts[i][bad[:6]]}")


def check(vali, gpu, mk, fmt, dets, m=5, proto=(24, 20), dtype="float32", alpha=128, rects=mc.RECTS, coeffs=None,
          head=False, expand=False, seed=0, poison=False, dev_args=False):
    """paint `dets` on fresh noise frames and compare every frame with the model; returns the model's drawn rows"""
    from vali_amd._native import shim

    wp, hp = proto
    protos = mc.protos(m, wp, hp, dtype)
    coeffs = mc.coeffs(m, dtype) if coeffs is None else coeffs
    if expand:
        protos = protos[:1]
    pt = to_device(protos, dtype, gpu)
    if expand:
        pt = pt.expand(len(mc.SIZES), -1, -1, -1)
        assert pt.stride(0) == 0
    ct = head_slice(coeffs, dtype, gpu) if head else to_device(coeffs, dtype, gpu)
    surfs, hosts = make_frames(vali, gpu, fmt, mc.SIZES, seed)
    dt = device_marks(dets, gpu)
    mb = mk.Prepare(surfs, pt, ct, dt, max_det=mc.D, net_size=mc.NET)
    assert mb.ws_bytes == len(mc.SIZES) * mc.D * hp * wp * 4
    if poison:
        # huge positive floats everywhere: a read of launch 2 outside what launch 1 wrote turns pixels on
        shim.memset2d_async(gpu, mb.d_ws, mb.ws_bytes, 0x7F, mb.ws_bytes, 1, mk.Stream)
        shim.stream_sync(gpu, mk.Stream)
    r, c = rects, mc.COLOURS
    if dev_args:
        r = torch.tensor(np.asarray(rects, np.int32), dtype=torch.int32, device=f"cuda:{gpu}")
        c = torch.tensor(np.asarray(mc.COLOURS, np.int32), dtype=torch.int32, device=f"cuda:{gpu}")
        torch.cuda.synchronize()
    ok, info = mk.Run(mb, r, c, alpha=alpha, cc_ctx=pm.cc_ctx_of(vali, ROWS_601))
    assert ok and info == vali.TaskExecInfo.SUCCESS, info
    drawn = mm.apply(hosts, fmt, mc.SIZES, dets, mc.D, protos, coeffs, rects, mc.COLOURS, alpha, mc.NET,
                     pm.matrices()[ROWS_601])
    compare(vali, gpu, surfs, hosts, (fmt, m, proto, dtype))
    return drawn


# ---- formats, prototype sizes, M, dtypes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("proto", mc.PROTO_SIZES, ids=lambda p: f"{p[0]}x{p[1]}")
@pytest.mark.parametrize("fmt", am.FORMATS)
def test_every_format(vali, gpu, mk, fmt, proto):
    assert len(check(vali, gpu, mk, fmt, mc.PLACEMENTS, proto=proto)) == 8


@pytest.mark.parametrize("dtype", list(DT))
@pytest.mark.parametrize("m", mc.MS)
@pytest.mark.parametrize("fmt,proto", [("NV12", (24, 20)), ("RGB", (16, 16))])
def test_every_m_and_dtype(vali, gpu, mk, fmt, proto, m, dtype):
    assert len(check(vali, gpu, mk, fmt, mc.PLACEMENTS, m=m, proto=proto, dtype=dtype, alpha=None, seed=1)) == 8


@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_a_transposed_head_slice_and_expanded_prototypes(vali, gpu, mk, dtype):
    check(vali, gpu, mk, "NV12", mc.PLACEMENTS, m=32, dtype=dtype, head=True, seed=2)
    check(vali, gpu, mk, "BGR", mc.PLACEMENTS, m=5, dtype=dtype, expand=True, seed=2)
    check(vali, gpu, mk, "YUV420", mc.PLACEMENTS, m=5, dtype=dtype, head=True, expand=True, seed=2, proto=(16, 16))


def test_device_rects_and_colours(vali, gpu, mk):
    check(vali, gpu, mk, "NV12", mc.PLACEMENTS, dev_args=True, seed=3)
    check(vali, gpu, mk, "RGB_PLANAR", mc.PLACEMENTS, dev_args=True, alpha=255, seed=3)


@pytest.mark.parametrize("alpha", [0, 1, 255, None])
def test_alphas(vali, gpu, mk, alpha):
    check(vali, gpu, mk, "YUV444", mc.PLACEMENTS, alpha=alpha, seed=4)


# ---- rows that must be skipped, non-finite inputs ------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", am.FORMATS)
def test_skipped_rows(vali, gpu, mk, fmt):
    """frame -1, the frame field of another slot, k = K, k = -1, w = 0, int32 extremes that miss and that meet the frame"""
    drawn = check(vali, gpu, mk, fmt, mc.SKIPS, seed=5)
    assert {d[0] for d in drawn} == mc.SKIPS_PAINTED


@pytest.mark.parametrize("fmt", ["NV12", "RGB"])
def test_a_record_with_dst_w_0_leaves_its_frame_alone(vali, gpu, mk, fmt):
    drawn = check(vali, gpu, mk, fmt, mc.PLACEMENTS, rects=mc.RECTS_DST_W_0, seed=6)
    assert [d[0] for d in drawn] == [0, 1, 2, 3]


@pytest.mark.parametrize("dtype", list(DT))
@pytest.mark.parametrize("fmt,m", [("NV12", 5), ("RGB", 1), ("YUV420", 32)])
def test_nan_and_infinite_coefficients(vali, gpu, mk, fmt, m, dtype):
    drawn = check(vali, gpu, mk, fmt, mc.NONFINITE, m=m, dtype=dtype, coeffs=mc.nonfinite_coeffs(m, dtype), seed=7)
    assert len(drawn) == 8
    by_row = {d[0]: d[2] for d in drawn}
    assert not by_row[1].any() and not by_row[5].any()          # a NaN coefficient: nothing is in


# ---- the workspace -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,proto", [("NV12", (16, 16)), ("YUV420", (24, 20)), ("RGB", (24, 20)), ("YUV444", (16, 16))])
def test_launch_2_reads_only_what_launch_1_wrote(vali, gpu, mk, fmt, proto):
    check(vali, gpu, mk, fmt, mc.PLACEMENTS, proto=proto, poison=True, seed=8)
    check(vali, gpu, mk, fmt, mc.SKIPS, proto=proto, poison=True, seed=8)


# ---- the annotator gives the same bytes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", am.FORMATS)
def test_the_annotator_stamps_the_same_bytes_from_the_models_atlas(vali, gpu, mk, fmt):
    protos, coeffs = mc.protos(5, 24, 20), mc.coeffs(5)
    a, hosts = make_frames(vali, gpu, fmt, mc.SIZES, seed=9)
    b, _ = make_frames(vali, gpu, fmt, mc.SIZES, seed=9)
    mb = mk.Prepare(a, to_device(protos, "float32", gpu), to_device(coeffs, "float32", gpu),
                    device_marks(mc.PLACEMENTS, gpu), max_det=mc.D, net_size=mc.NET)
    assert mk.Run(mb, mc.RECTS, mc.COLOURS, alpha=128, cc_ctx=pm.cc_ctx_of(vali, ROWS_601))[0]
    drawn = mm.apply(hosts, fmt, mc.SIZES, mc.PLACEMENTS, mc.D, protos, coeffs, mc.RECTS, mc.COLOURS, 128, mc.NET,
                     pm.matrices()[ROWS_601])
    atlas, marks = mm.stamp_atlas(drawn, mc.PLACEMENTS)
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
def test_pitched_frames_keep_their_padding_and_a_frame_without_masks_its_bytes(vali, gpu, mk, fmt):
    from vali_amd._native import shim

    protos, coeffs = mc.protos(5, 16, 16), mc.coeffs(5)
    surfs = [vali.Surface.Make(getattr(vali, fmt), w, h, gpu) for w, h in mc.SIZES]
    stream = mk.Stream
    for s in surfs:
        for p in s._planes:
            shim.memset2d_async(gpu, p.GpuMem, p.Pitch, 0x5A, p.Pitch, p.Height, stream)
    shim.stream_sync(gpu, stream)
    hosts = mc.noise_frames(fmt, seed=10)
    for s, host in zip(surfs, hosts):
        assert vali.PyFrameUploader(gpu).Run(host, s)[0]
    dets = list(mc.PLACEMENTS[:4]) + [(-1, 0, 0, 0, 0, 0, 0, 0)] * 4            # frame 1 has no detection
    mb = mk.Prepare(surfs, to_device(protos, "float32", gpu), to_device(coeffs, "float32", gpu), device_marks(dets, gpu),
                    max_det=mc.D, net_size=mc.NET)
    assert mk.Run(mb, mc.RECTS, mc.COLOURS, alpha=200, cc_ctx=pm.cc_ctx_of(vali, ROWS_601))[0]
    untouched = hosts[1].copy()
    mm.apply(hosts, fmt, mc.SIZES, dets, mc.D, protos, coeffs, mc.RECTS, mc.COLOURS, 200, mc.NET, pm.matrices()[ROWS_601])
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
def test_frames_at_odd_addresses_and_the_canary_around_them(vali, gpu, mk, fmt):
    protos, coeffs = mc.protos(5, 24, 20), mc.coeffs(5)
    pt, ct = to_device(protos, "float32", gpu), to_device(coeffs, "float32", gpu)
    dets = device_marks(mc.PLACEMENTS, gpu)
    for x0, extra in ((3, 9), (1, 1)):
        bufs, views, hosts = [], [], mc.noise_frames(fmt, seed=11)
        for i, (w, h) in enumerate(mc.SIZES):
            (prows, cols), = am.plane_shapes(fmt, w, h)
            pitch = (cols + x0 + extra) | 1
            buf = torch.full((prows + 4, pitch), 0xA5, dtype=torch.uint8, device=f"cuda:{gpu}")
            buf[2:2 + prows, x0:x0 + cols] = torch.from_numpy(hosts[i].reshape(prows, cols)).to(buf.device)
            bufs.append(buf)
            views.append(buf[2:2 + prows, x0:x0 + cols])
        torch.cuda.synchronize()
        surfs = [vali.Surface.from_dlpack(v, getattr(vali, fmt)) for v in views]
        assert surfs[0].PixelPtr(0) % 2 == 1 and surfs[0].Pitch % 16
        mb = mk.Prepare(surfs, pt, ct, dets, max_det=mc.D, net_size=mc.NET)
        assert mk.Run(mb, mc.RECTS, mc.COLOURS, alpha=128, cc_ctx=pm.cc_ctx_of(vali, ROWS_601))[0]
        mm.apply(hosts, fmt, mc.SIZES, mc.PLACEMENTS, mc.D, protos, coeffs, mc.RECTS, mc.COLOURS, 128, mc.NET,
                 pm.matrices()[ROWS_601])
        for i, (w, h) in enumerate(mc.SIZES):
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
    mk = vali.PyInstanceMasker(gpu, stream)
    sets = [(mc.PLACEMENTS, mc.coeffs(5, seed=0)), (mc.SKIPS, mc.coeffs(5, seed=1)),
            (list(reversed(mc.PLACEMENTS[:4])) + list(mc.PLACEMENTS[4:]), mc.coeffs(5, seed=2))]
    protos = mc.protos(5, 24, 20)
    pt, ct = to_device(protos, "float32", gpu), to_device(sets[0][1], "float32", gpu)
    dets = device_marks(sets[0][0], gpu)
    rects = torch.tensor(np.asarray(mc.RECTS, np.int32), dtype=torch.int32, device=dev)
    colours = torch.tensor(np.asarray(mc.COLOURS, np.int32), dtype=torch.int32, device=dev)
    surfs, _ = make_frames(vali, gpu, fmt, mc.SIZES, seed=12)
    torch.cuda.synchronize()
    mb = mk.Prepare(surfs, pt, ct, dets, max_det=mc.D, net_size=mc.NET)
    cap = vali.StreamCapture(stream, gpu)
    with cap:
        assert mk.RunAsync(mb, rects, colours, alpha=128)[0]
    cap.Keep(mb)
    for k, (rows, coeffs) in enumerate(sets):
        hosts = mc.noise_frames(fmt, seed=20 + k)
        for s, host in zip(surfs, hosts):
            assert vali.PyFrameUploader(gpu).Run(host, s)[0]
        dets.copy_(device_marks(rows, gpu))                       # rewritten in place
        ct.copy_(to_device(coeffs, "float32", gpu))
        torch.cuda.synchronize()
        cap.Launch()
        shim.stream_sync(gpu, stream)
        mm.apply(hosts, fmt, mc.SIZES, rows, mc.D, protos, coeffs, mc.RECTS, mc.COLOURS, 128, mc.NET, pm.matrices()[ROWS_601])
        compare(vali, gpu, surfs, hosts, ("replay", k))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_prepare_and_run_say_what_is_wrong(vali, gpu, mk):
    protos, coeffs = mc.protos(5, 16, 16), mc.coeffs(5)
    pt, ct = to_device(protos, "float32", gpu), to_device(coeffs, "float32", gpu)
    dets = device_marks(mc.PLACEMENTS, gpu)
    surfs, _ = make_frames(vali, gpu, "NV12", mc.SIZES, seed=13)
    with pytest.raises(ValueError, match="x stride"):
        mk.Prepare(surfs, pt.transpose(2, 3), ct, dets, max_det=mc.D, net_size=mc.NET)
    with pytest.raises(ValueError, match="disagree"):
        mk.Prepare(surfs, pt, ct[:, :, :4], dets, max_det=mc.D, net_size=mc.NET)
    with pytest.raises(ValueError, match="dets"):
        mk.Prepare(surfs, pt, ct, dets[:7], max_det=mc.D, net_size=mc.NET)
    with pytest.raises(ValueError, match="3 surfaces"):
        mk.Prepare(surfs + surfs[:1], pt, ct, dets, max_det=mc.D, net_size=mc.NET)
    with pytest.raises(ValueError, match="dtype"):
        mk.Prepare(surfs, pt.double(), ct, dets, max_det=mc.D, net_size=mc.NET)
    with pytest.raises(ValueError, match="GPU"):
        mk.Prepare(surfs, pt.cpu(), ct, dets, max_det=mc.D, net_size=mc.NET)
    mixed = [surfs[0], vali.Surface.Make(vali.RGB, 70, 50, gpu)]
    with pytest.raises(ValueError, match="one format per batch"):
        mk.Prepare(mixed, pt, ct, dets, max_det=mc.D, net_size=mc.NET)
    mb = mk.Prepare(surfs, pt, ct, dets, max_det=mc.D, net_size=mc.NET)
    with pytest.raises(ValueError, match="rects"):
        mk.Run(mb, mc.RECTS[:1], mc.COLOURS)
    with pytest.raises(ValueError, match="alpha"):
        mk.Run(mb, mc.RECTS, mc.COLOURS, alpha=300)
    with pytest.raises(ValueError, match="MaskBatch"):
        mk.Run(None, mc.RECTS, mc.COLOURS)
