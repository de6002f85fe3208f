"""RGB, BGR and RGB_PLANAR sources of the fused preprocessor on the GPU (vali_rgb_preproc_roi[_batch]).

The definition (include/vali_hip.h): inside the placement, the bilinear resize of the crop view exactly as
vali_resize(LINEAR) does it for the source's format, the channels named by colour, then step 3 of vali_nv12_preproc
(float destinations) or the bytes in the destination's memory order; outside it the pad colour through step 3, or
nothing written.  Every comparison is bit-exact (float results as bytes): the expected value is the chain of the
library's own tasks -- shim.resize on the crop view into a scratch surface, PySurfaceConverter to the destination's
layout, float32 numpy for step 3 -- and, for a subset, the CPU oracle's resize_plane."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
NORMS = {"imagenet": (255.0, MEAN, STD), "identity": (1.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))}
SENT = 0x5A
PAD = (10, 200, 77)        # not grey: catches a channel-order slip
SRC = ("RGB", "BGR", "RGB_PLANAR")
# bytes per pixel of a destination view, planes, element type, host layout
DST = {"RGB_32F_PLANAR": (4, 3, np.float32, "CHW"), "RGB_32F": (12, 1, np.float32, "HWC"),
       "RGB": (3, 1, np.uint8, "HWC"), "BGR": (3, 1, np.uint8, "HWC"), "RGB_PLANAR": (1, 3, np.uint8, "CHW")}
OUTS = [(f, n) for f in DST for n in (("imagenet", "identity") if DST[f][2] == np.float32 else ("identity",))]

# (src_w, src_h, crop, canvas_w, canvas_h, place)
GEOMS = {
    "crop_1x1_up": (64, 48, (10, 7, 1, 1), 32, 33, (5, 8, 9, 7)),
    "crop_1_wide": (64, 48, (63, 5, 1, 20), 40, 40, (3, 3, 30, 31)),
    "crop_right_bottom_edges_odd": (131, 71, (66, 30, 65, 41), 97, 65, (3, 2, 61, 51)),
    "upscale": (100, 80, (3, 2, 31, 21), 300, 201, (11, 20, 271, 171)),
    "downscale_2_32": (640, 360, (101, 51, 401, 301), 225, 224, (3, 2, 173, 131)),
    "same_size_odd_offset": (321, 241, (51, 43, 131, 91), 301, 201, (39, 91, 131, 91)),
    "same_size_whole": (257, 129, (0, 0, 257, 129), 257, 129, (0, 0, 257, 129)),
    "tall_299_to_224": (299, 299, (0, 0, 299, 299), 224, 224, (0, 0, 224, 224)),
    "wide": (1281, 721, (3, 1, 1277, 717), 1301, 741, (7, 11, 1283, 719)),
    "letterbox_501x375": (501, 375, (0, 0, 501, 375), 640, 640, (0, 80, 640, 479)),
    "letterbox_1080p": (1920, 1080, (0, 0, 1920, 1080), 640, 640, (0, 140, 640, 360)),
}
for _k in range(4):     # crop and placement at every x mod 4: the 12-byte phases of packed sources
    GEOMS[f"same_size_phase_{_k}"] = (203, 121, (20 + _k, 11, 90, 60), 161, 101, (35 - _k, 6, 90, 60))
    GEOMS[f"resize_phase_{_k}"] = (203, 121, (20 + _k, 10, 91, 61), 161, 101, (33 + _k, 6, 95, 70))


# ---- helpers ---------------------------------------------------------------------------------------------------
def colour_image(w, h, seed):
    """(h, w, 3) u8 in COLOUR order R, G, B"""
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def to_memory(img, sfmt):
    """the colour image as the source format stores it (tightly packed host layout)"""
    if sfmt == "RGB":
        return np.ascontiguousarray(img)
    if sfmt == "BGR":
        return np.ascontiguousarray(img[..., ::-1])
    return np.ascontiguousarray(img.transpose(2, 0, 1))


def upload(vali, gpu, img, sfmt):
    h, w, _ = img.shape
    s = vali.Surface.Make(getattr(vali.PixelFormat, sfmt), w, h, gpu)
    assert vali.PyFrameUploader(gpu).Run(to_memory(img, sfmt).reshape(-1), s)[0]
    return s


def fill(gpu, surf, value=SENT):
    from vali_amd._native import shim

    for pl in surf.Planes:
        shim.memset2d_async(gpu, pl.GpuMem, pl.Pitch, value, pl.Width * pl.ElemSize, pl.Height, 0)
    shim.stream_sync(gpu, 0)


def canvas(vali, gpu, fmt, w, h):
    d = vali.Surface.Make(getattr(vali.PixelFormat, fmt), w, h, gpu)
    fill(gpu, d)
    return d


def download(vali, gpu, surf):
    out = np.zeros(surf.HostSize, np.uint8)
    assert vali.PySurfaceDownloader(gpu).Run(surf, out)[0]
    return out


def as_image(raw, fmt, w, h):
    """downloaded bytes -> (3, h, w) or (h, w, 3) of the format's element type"""
    _, _, dt, lay = DST[fmt]
    a = raw.view(dt)
    return a.reshape(3, h, w) if lay == "CHW" else a.reshape(h, w, 3)


def src_view(shim, s, sfmt, x, y, w, h):
    p = s.Pitch
    if sfmt == "RGB_PLANAR":
        return shim.SurfaceDesc([s.PixelPtr(c) + y * p + x for c in range(3)], [p] * 3, w, h, int(s.Format))
    return shim.SurfaceDesc([s.PixelPtr(0) + y * p + 3 * x], [p], w, h, int(s.Format))


def step3(x, norm, layout):
    """float32 numpy: (x / div - mean[c]) / std[c] on x = q / 255.0f in colour order (what RGB -> RGB_32F leaves)"""
    div, mean, std = norm
    m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    if layout == "CHW":
        m, s = m[:, None, None], s[:, None, None]
    x = x.astype(np.float32) / np.float32(div)
    return ((x - m) / s).astype(np.float32)


def chain_rgb_surface(vali, gpu, src, sfmt, crop, dw, dh):
    """steps 1 and 2 with the library's own tasks: resize of the crop VIEW (LINEAR) in the source's format, then the
    converter to packed RGB"""
    from vali_amd._native import shim

    pf = getattr(vali.PixelFormat, sfmt)
    small = vali.Surface.Make(pf, dw, dh, gpu)
    rc = shim.resize(src_view(shim, src, sfmt, *crop), small.desc(), int(vali.Interpolation.LINEAR), 0)
    assert rc == 0, shim.last_error()
    shim.stream_sync(gpu, 0)
    if sfmt == "RGB":
        return small
    rgb = vali.Surface.Make(vali.RGB, dw, dh, gpu)
    assert vali.PySurfaceConverter(gpu).Run(small, rgb)[0]
    return rgb


def chain_output(vali, gpu, rgb, dfmt, norm):
    """packed RGB u8 surface -> what the destination format holds (host layout), through the converters + numpy"""
    dw, dh = rgb.Width, rgb.Height
    cvt = vali.PySurfaceConverter(gpu)
    if dfmt == "RGB":
        return as_image(download(vali, gpu, rgb), dfmt, dw, dh)
    if dfmt in ("BGR", "RGB_PLANAR"):
        out = vali.Surface.Make(getattr(vali.PixelFormat, dfmt), dw, dh, gpu)
        assert cvt.Run(rgb, out)[0]
        return as_image(download(vali, gpu, out), dfmt, dw, dh)
    f32 = vali.Surface.Make(vali.RGB_32F, dw, dh, gpu)
    assert cvt.Run(rgb, f32)[0]
    if dfmt == "RGB_32F_PLANAR":
        pl = vali.Surface.Make(vali.RGB_32F_PLANAR, dw, dh, gpu)
        assert cvt.Run(f32, pl)[0]
        f32 = pl
    return step3(as_image(download(vali, gpu, f32), dfmt, dw, dh), NORMS[norm], DST[dfmt][3])


def pad_pixel(fmt, norm, pad):
    """the pad colour as it lands in memory, per channel slot of the host layout"""
    if DST[fmt][2] == np.uint8:
        return np.array(pad[::-1] if fmt == "BGR" else pad, np.uint8)
    div, mean, std = NORMS[norm]
    q = np.asarray(pad, np.float32)
    return (((q / np.float32(255.0)) / np.float32(div) - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
            ).astype(np.float32)


def expected_canvas(inner, fmt, cw, ch, place, norm, pad):
    """the definition on a sentinel-filled canvas: `inner` inside `place`; outside it the pad colour or the sentinel"""
    bpp = DST[fmt][0] * DST[fmt][1]
    want = as_image(np.full(cw * ch * bpp, SENT, np.uint8), fmt, cw, ch)
    chw = DST[fmt][3] == "CHW"
    if pad is not None:
        pv = pad_pixel(fmt, norm, pad)
        if chw:
            want[:] = pv[:, None, None]
        else:
            want[:] = pv
    if inner is not None:
        x, y, w, h = place
        if chw:
            want[:, y:y + h, x:x + w] = inner
        else:
            want[y:y + h, x:x + w] = inner
    return want


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def preprocessor(vali, gpu, norm, stream=None):
    div, mean, std = NORMS[norm]
    return vali.PySurfacePreprocessor(gpu, stream, mean=mean, std=std, div=div)


# ---- the definition, case by case ------------------------------------------------------------------------------
@pytest.mark.parametrize("dfmt, norm", OUTS, ids=[f"{f}-{n}" for f, n in OUTS])
@pytest.mark.parametrize("sfmt", SRC)
@pytest.mark.parametrize("geom", list(GEOMS))
def test_roi_equals_the_chain_on_views(vali, gpu, geom, sfmt, dfmt, norm):
    sw, sh, crop, cw, ch, place = GEOMS[geom]
    img = colour_image(sw, sh, seed=sw + 3 * ch)
    src = upload(vali, gpu, img, sfmt)
    pp = preprocessor(vali, gpu, norm)
    inner = chain_output(vali, gpu, chain_rgb_surface(vali, gpu, src, sfmt, crop, place[2], place[3]), dfmt, norm)
    for pad in (PAD, None):
        got = canvas(vali, gpu, dfmt, cw, ch)
        assert pp.RunRoi(src, got, crop, place, pad) == (True, vali.TaskExecInfo.SUCCESS)
        want = expected_canvas(inner, dfmt, cw, ch, place, norm, pad)
        assert same_bits(as_image(download(vali, gpu, got), dfmt, cw, ch), want), f"pad={pad}"


def oracle_inner(oracle, img, crop, dw, dh, dfmt, norm):
    """the CPU oracle's chain on the colour image: resize_plane of the crop (3 interleaved channels), layout, step 3"""
    x, y, w, h = crop
    view = np.ascontiguousarray(img[y:y + h, x:x + w]).reshape(h, w * 3)
    q = oracle.resize_plane(view, 3, dw, dh, "linear").reshape(dh, dw, 3)
    if dfmt == "BGR":
        q = q[..., ::-1]
    if DST[dfmt][3] == "CHW":
        q = q.transpose(2, 0, 1)
    return q if DST[dfmt][2] == np.uint8 else step3(q.astype(np.float32) / np.float32(255.0), NORMS[norm], DST[dfmt][3])


@pytest.mark.parametrize("sfmt", SRC)
@pytest.mark.parametrize("geom", ["crop_1x1_up", "crop_1_wide", "crop_right_bottom_edges_odd", "resize_phase_1",
                                  "same_size_phase_3", "downscale_2_32", "letterbox_501x375", "letterbox_1080p"])
def test_roi_against_oracle(vali, gpu, oracle, geom, sfmt):
    sw, sh, crop, cw, ch, place = GEOMS[geom]
    img = colour_image(sw, sh, seed=7 * sw + 1)
    src = upload(vali, gpu, img, sfmt)
    for dfmt, norm in (("RGB_32F_PLANAR", "imagenet"), ("BGR", "identity")):
        got = canvas(vali, gpu, dfmt, cw, ch)
        assert preprocessor(vali, gpu, norm).RunRoi(src, got, crop, place, (114, 114, 114))[0]
        want = expected_canvas(oracle_inner(oracle, img, crop, place[2], place[3], dfmt, norm), dfmt, cw, ch, place,
                               norm, (114, 114, 114))
        assert same_bits(as_image(download(vali, gpu, got), dfmt, cw, ch), want), dfmt


def test_planar_oracle_is_the_packed_one(oracle):
    """channel by channel: the 3-channel resize of a packed image equals three 1-channel resizes (what RGB_PLANAR
    sources are defined by)"""
    img = colour_image(131, 71, seed=2)
    packed = oracle.resize_plane(img.reshape(71, 131 * 3), 3, 97, 50, "linear").reshape(50, 97, 3)
    for c in range(3):
        assert np.array_equal(packed[..., c], oracle.resize_plane(np.ascontiguousarray(img[..., c]), 1, 97, 50, "linear"))


# ---- whole surfaces: Run / RunBatch against the public tasks ----------------------------------------------------
def public_chain(vali, gpu, src, sfmt, dw, dh, dfmt, norm):
    pf = getattr(vali.PixelFormat, sfmt)
    cur = src
    if (src.Width, src.Height) != (dw, dh):
        cur = vali.Surface.Make(pf, dw, dh, gpu)
        assert vali.PySurfaceResizer(pf, gpu, interpolation=vali.Interpolation.LINEAR).Run(src, cur)[0]
    if sfmt != "RGB":
        rgb = vali.Surface.Make(vali.RGB, dw, dh, gpu)
        assert vali.PySurfaceConverter(gpu).Run(cur, rgb)[0]
        cur = rgb
    return chain_output(vali, gpu, cur, dfmt, norm)


@pytest.mark.parametrize("sfmt, dfmt, norm", [
    ("BGR", "RGB_32F_PLANAR", "imagenet"),      # channel naming
    ("RGB", "BGR", "identity"),
    ("RGB", "RGB_32F_PLANAR", "imagenet"),
    ("RGB_PLANAR", "RGB_32F", "imagenet"),
    ("RGB_PLANAR", "RGB", "identity"),
    ("BGR", "RGB_PLANAR", "identity"),
])
@pytest.mark.parametrize("size", [(501, 375, 299, 299), (333, 251, 333, 251), (1920, 1080, 640, 360)],
                         ids=["501x375_to_299", "333x251_same", "1080p_to_640x360"])
def test_run_and_run_batch_equal_the_public_chain(vali, gpu, size, sfmt, dfmt, norm):
    sw, sh, dw, dh = size
    pp = preprocessor(vali, gpu, norm)
    srcs = [upload(vali, gpu, colour_image(sw, sh, seed=11 + i), sfmt) for i in range(3)]
    wants = [public_chain(vali, gpu, s, sfmt, dw, dh, dfmt, norm) for s in srcs]
    cc = vali.ColorspaceConversionContext(vali.ColorSpace.BT_601, vali.ColorRange.MPEG)   # accepted and ignored
    for s, want in zip(srcs, wants):
        dst = canvas(vali, gpu, dfmt, dw, dh)
        for _ in range(2):      # the second call takes the task's memo
            assert pp.Run(s, dst, cc) == (True, vali.TaskExecInfo.SUCCESS)
        assert same_bits(as_image(download(vali, gpu, dst), dfmt, dw, dh), want)
    dsts = [canvas(vali, gpu, dfmt, dw, dh) for _ in srcs]
    assert pp.RunBatch(pp.PrepareBatch(srcs, dsts)) == (True, vali.TaskExecInfo.SUCCESS)
    for d, want in zip(dsts, wants):
        assert same_bits(as_image(download(vali, gpu, d), dfmt, dw, dh), want)


def test_errors(vali, gpu):
    I = vali.TaskExecInfo
    pp = vali.PySurfacePreprocessor(gpu)
    rgb = vali.Surface.Make(vali.RGB, 63, 47, gpu)
    dst = vali.Surface.Make(vali.RGB_32F_PLANAR, 299, 299, gpu)
    for crop in ((60, 0, 4, 4), (0, 0, 64, 4), (-1, 0, 4, 4), (0, 0, 0, 4), (0, 47, 1, 1)):
        assert pp.RunRoi(rgb, dst, crop) == (False, I.INVALID_INPUT)
    assert pp.RunRoi(rgb, dst, None, (298, 298, 2, 1)) == (False, I.INVALID_INPUT)
    assert pp.RunRoi(rgb, dst, None, None, (1, 2)) == (False, I.INVALID_INPUT)
    assert pp.RunRoi(rgb, vali.Surface.Make(vali.YUV444, 32, 32, gpu)) == (False, I.NOT_SUPPORTED)
    assert pp.Run(rgb, vali.Surface.Make(vali.NV12, 32, 32, gpu)) == (False, I.NOT_SUPPORTED)
    assert pp.RunRoi(vali.Surface.Make(vali.YUV444, 63, 47, gpu), dst) == (False, I.NOT_SUPPORTED)
    assert pp.RunRoi(vali.Surface.Make(vali.Y, 63, 47, gpu), dst) == (False, I.NOT_SUPPORTED)
    norm = vali.PySurfacePreprocessor(gpu, mean=MEAN, std=STD, div=255.0)
    assert norm.RunRoi(rgb, vali.Surface.Make(vali.BGR, 31, 31, gpu)) == (False, I.NOT_SUPPORTED)
    assert pp.RunRoi(rgb, dst, (62, 46, 1, 1), (298, 298, 1, 1), (0, 0, 0)) == (True, I.SUCCESS)
    with pytest.raises(ValueError, match="one format"):
        pp.PrepareRoiBatch([rgb, vali.Surface.Make(vali.BGR, 63, 47, gpu)], [dst, dst])


# ---- batches -----------------------------------------------------------------------------------------------------
def _batch_vs_single(vali, gpu, pp, srcs, crops, cw, ch, fmt, places, pad):
    dsts = [canvas(vali, gpu, fmt, cw, ch) for _ in srcs]
    batch = pp.PrepareRoiBatch(srcs, dsts, crops, places)
    assert pp.RunRoiBatch(batch, pad) == (True, vali.TaskExecInfo.SUCCESS)
    for s, c, p, d in zip(srcs, crops, places, dsts):
        one = canvas(vali, gpu, fmt, cw, ch)
        assert pp.RunRoi(s, one, c, p, pad)[0]
        assert np.array_equal(download(vali, gpu, d), download(vali, gpu, one))


@pytest.mark.parametrize("sfmt", SRC)
def test_batch_mixed_sources_equals_single_calls(vali, gpu, sfmt):
    sizes = [(1920, 1080), (641, 361), (1279, 719), (1, 1), (2, 5)]
    frames = [upload(vali, gpu, colour_image(w, h, seed=w), sfmt) for w, h in sizes]
    big = frames[0]
    boxes = [(0, 0, 33, 31), (1887, 1049, 33, 31), (101, 200, 511, 301), (999, 3, 1, 1), (7, 1001, 401, 79),
             (1001, 501, 919, 579), (641, 361, 224, 224), (1, 1, 1918, 1078)]
    srcs = frames + [big] * len(boxes)
    crops = [None, (11, 20, 301, 200), (3, 2, 1275, 716), None, None] + boxes
    places = [(0, 19, 224, 185)] * len(srcs)
    _batch_vs_single(vali, gpu, preprocessor(vali, gpu, "imagenet"), srcs, crops, 224, 224, "RGB_32F_PLANAR", places,
                     (114, 114, 114))
    places = [(1 + i % 4, 139, 637, 361) for i in range(len(srcs))]
    _batch_vs_single(vali, gpu, preprocessor(vali, gpu, "identity"), srcs, crops, 641, 640, "BGR", places, PAD)


def test_batch_mosaic_without_padding(vali, gpu):
    sizes = [(641, 361), (321, 239), (1279, 721), (199, 201)]
    srcs = [upload(vali, gpu, colour_image(w, h, seed=7 + w), "BGR") for w, h in sizes]
    pp = preprocessor(vali, gpu, "imagenet")
    cells = [(0, 0, 319, 319), (321, 0, 318, 319), (0, 321, 319, 318), (321, 321, 318, 318)]
    mosaic = canvas(vali, gpu, "RGB_32F", 639, 639)
    batch = pp.PrepareRoiBatch(srcs, [mosaic] * 4, None, cells)
    assert pp.RunRoiBatch(batch) == (True, vali.TaskExecInfo.SUCCESS)
    want = canvas(vali, gpu, "RGB_32F", 639, 639)
    for s, cell in zip(srcs, cells):
        assert pp.RunRoi(s, want, None, cell)[0]
    got = download(vali, gpu, mosaic)
    assert np.array_equal(got, download(vali, gpu, want))
    img = got.reshape(639, 639, 12)
    assert (img[319:321] == SENT).all() and (img[:, 319:321] == SENT).all()     # the gaps were never written
    assert not (img[:319, :319] == SENT).all()


def _torch_rects(rects):
    import torch

    t = torch.tensor(rects, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    return t


def test_device_rects_equal_uploaded_rects(vali, gpu):
    frame = upload(vali, gpu, colour_image(1919, 1079, seed=5), "RGB")
    boxes = [(0, 0, 63, 127), (501, 301, 299, 301), (1856, 1016, 63, 63), (101, 899, 801, 180), (1918, 1078, 1, 1)]
    n = len(boxes)
    place = (1, 0, 223, 224)
    pp = preprocessor(vali, gpu, "imagenet")
    d1 = [canvas(vali, gpu, "RGB_32F_PLANAR", 224, 224) for _ in boxes]
    assert pp.RunRoiBatch(pp.PrepareRoiBatch([frame] * n, d1, boxes, [place] * n), (114, 114, 114))[0]
    d2 = [canvas(vali, gpu, "RGB_32F_PLANAR", 224, 224) for _ in boxes]
    b2 = pp.PrepareRoiBatch([frame] * n, d2)                      # uploaded rects: whole frame
    t = _torch_rects([list(b) + list(place) for b in boxes])
    assert pp.RunRoiBatch(b2, (114, 114, 114), rects=t) == (True, vali.TaskExecInfo.SUCCESS)
    for a, b in zip(d1, d2):
        assert np.array_equal(download(vali, gpu, a), download(vali, gpu, b))


def test_capture_reads_rects_from_a_device_tensor(vali, gpu):
    from vali_amd._native import shim

    stream = shim.stream_create(gpu)
    pp = preprocessor(vali, gpu, "imagenet", stream)
    frame = upload(vali, gpu, colour_image(1281, 719, seed=11), "RGB_PLANAR")
    n = 6
    dsts = [canvas(vali, gpu, "RGB_32F_PLANAR", 224, 224) for _ in range(n)]
    batch = pp.PrepareRoiBatch([frame] * n, dsts)
    first = [[41 * i, 21 * i, 201, 101, 0, 61, 224, 101] for i in range(n)]
    second = [[1281 - 63 * (i + 1), 719 - 97, 63 * (i + 1), 97, 11, 3, 199, 219] for i in range(n)]
    t = _torch_rects(first)
    cap = vali.StreamCapture(stream, gpu)
    with cap:
        assert pp.RunRoiBatchAsync(batch, (114, 114, 114), rects=t)[0]
    cap.Keep(batch, t)
    # new rectangles written into the same tensor on the same stream, then one replay
    new = np.asarray(second, np.int32)
    hp, _, _ = shim.buffer_info(new, False)
    shim.memcpy2d_async(gpu, t.data_ptr(), 32 * n, hp, 32 * n, 32 * n, 1, 0, stream)
    cap.Launch()
    shim.stream_sync(gpu, stream)
    got = [download(vali, gpu, d) for d in dsts]
    ref = [canvas(vali, gpu, "RGB_32F_PLANAR", 224, 224) for _ in range(n)]
    rb = pp.PrepareRoiBatch([frame] * n, ref, [r[:4] for r in second], [r[4:] for r in second])
    assert pp.RunRoiBatch(rb, (114, 114, 114))[0]
    for g, r in zip(got, ref):
        assert np.array_equal(g, download(vali, gpu, r))
    del cap
    shim.stream_destroy(gpu, stream)


# ---- containment: malformed device rectangles inside one sentinel-filled arena -----------------------------------
class Arena:
    """one device buffer filled with the sentinel; every surface of the test is carved out of it"""

    def __init__(self, gpu, size):
        from vali_amd._native import shim

        self.shim, self.gpu, self.size = shim, gpu, size
        self.ptr = shim.mem_alloc(gpu, size)
        shim.memset2d_async(gpu, self.ptr, size, SENT, size, 1, 0)
        shim.stream_sync(gpu, 0)
        self.cursor = 0

    def carve(self, pitch, rows):
        off = ((self.cursor + 255) // 256) * 256
        self.cursor = off + pitch * rows + 256          # a gap after every region, checked for the sentinel
        assert self.cursor <= self.size
        return off

    def upload(self, off, pitch, a):
        a = np.ascontiguousarray(a)
        hp, _, _ = self.shim.buffer_info(a, False)
        self.shim.memcpy2d_async(self.gpu, self.ptr + off, pitch, hp, a.shape[1], a.shape[1], a.shape[0], 0, 0)
        self.shim.stream_sync(self.gpu, 0)

    def download(self):
        out = np.zeros(self.size, np.uint8)
        hp, _, _ = self.shim.buffer_info(out, True)
        self.shim.memcpy2d_async(self.gpu, hp, self.size, self.ptr, self.size, self.size, 1, 1, 0)
        self.shim.stream_sync(self.gpu, 0)
        return out

    def free(self):
        self.shim.mem_free(self.gpu, self.ptr)


def _sanitise(v, size):
    """the kernel's rule for one axis (include/vali_hip.h): clamping only"""
    x, w = v
    x = min(max(x, 0), size)
    w = min(max(w, 0), size - x)
    return x, w


@pytest.mark.parametrize("sfmt, pad", [("RGB", True), ("BGR", False), ("RGB_PLANAR", True)])
def test_device_rects_are_sanitised_and_contained(vali, gpu, sfmt, pad):
    from vali_amd._native import shim

    SW, SH, CW, CH = 131, 71, 63, 47
    big = 2 ** 31 - 1
    rects = [
        (100, 10, 60, 40, 0, 0, 63, 47),            # crop runs past the right edge
        (-10, 4, 50, 30, -4, -6, 40, 40),           # negative x / placement
        (5, 7, 33, 21, 3, 3, 31, 31),               # odd everything: valid here, left as it is
        (10, 10, 0, 40, 0, 0, 63, 47),              # empty crop
        (130, 70, 5, 5, 62, 46, 9, 9),              # the last texel onto the last pixel
        (0, 0, big, big, 60, 44, 100, 100),         # huge sizes, placement in the corner
        (0, 0, 64, 64, 70, 0, 10, 10),              # placement beyond the canvas: empty
        (-big - 1, -big - 1, big, big, 2, 2, -8, 20),   # negative width: empty
        (big, big, big, big, big, big, big, big),   # everything past the end: empty
        (-big - 1, -big - 1, -big - 1, -big - 1, -big - 1, -big - 1, -big - 1, -big - 1),
    ]
    n = len(rects)
    img = colour_image(SW, SH, seed=99)
    mem = to_memory(img, sfmt)
    arena = Arena(gpu, 1 << 21)
    planar = sfmt == "RGB_PLANAR"
    row_bytes = SW if planar else 3 * SW
    sp = row_bytes + 5
    soff = arena.carve(sp, SH * (3 if planar else 1))
    arena.upload(soff, sp, mem.reshape(-1, row_bytes))
    sptr = arena.ptr + soff
    src = shim.SurfaceDesc([sptr + c * SH * sp for c in range(3)] if planar else [sptr], [sp] * (3 if planar else 1),
                           SW, SH, int(getattr(vali.PixelFormat, sfmt)))
    dsts, dregions = [], []
    for _ in range(n):
        dp = CW * 4 + 20
        off = arena.carve(dp, CH * 3)
        dregions.append((off, dp))
        dsts.append(shim.SurfaceDesc([arena.ptr + off + c * CH * dp for c in range(3)], [dp] * 3, CW, CH,
                                     int(vali.RGB_32F_PLANAR)))
    pp = preprocessor(vali, gpu, "imagenet")
    p = pp._params(None)
    d_src = shim.descs_upload(gpu, [src] * n, pp.Stream)
    d_dst = shim.descs_upload(gpu, dsts, pp.Stream)
    t = _torch_rects([list(r) for r in rects])
    padc = (114, 114, 114) if pad else None
    try:
        rc = shim.rgb_preproc_roi_batch(d_src, d_dst, t.data_ptr(), n, int(getattr(vali.PixelFormat, sfmt)), CW, CH,
                                        int(vali.RGB_32F_PLANAR), p, pad, (114, 114, 114), pp.Stream)
        assert rc == 0, shim.last_error()
        shim.stream_sync(gpu, pp.Stream)
        buf = arena.download()
    finally:
        shim.mem_free(gpu, d_src)
        shim.mem_free(gpu, d_dst)
    real = upload(vali, gpu, img, sfmt)
    for r, (off, dp) in zip(rects, dregions):
        sx, sw = _sanitise((r[0], r[2]), SW)
        sy, sh = _sanitise((r[1], r[3]), SH)
        dx, dw = _sanitise((r[4], r[6]), CW)
        dy, dh = _sanitise((r[5], r[7]), CH)
        got = buf[off:off + 3 * CH * dp].reshape(3 * CH, dp)[:, :CW * 4].reshape(3, CH, CW * 4)
        if min(sw, sh, dw, dh) < 1:         # empty: all pad, or untouched
            want = expected_canvas(None, "RGB_32F_PLANAR", CW, CH, None, "imagenet", padc)
        else:
            one = canvas(vali, gpu, "RGB_32F_PLANAR", CW, CH)
            assert pp.RunRoi(real, one, (sx, sy, sw, sh), (dx, dy, dw, dh), padc)[0]
            want = as_image(download(vali, gpu, one), "RGB_32F_PLANAR", CW, CH)
        assert np.array_equal(got, np.ascontiguousarray(want).view(np.uint8).reshape(3, CH, CW * 4)), r
    # containment: every byte outside the destination rows (pitch padding, gaps, the rest of the arena) is the
    # sentinel, and the source is unchanged
    mask = np.ones(arena.size, bool)
    for off, dp in dregions:
        for row in range(3 * CH):
            mask[off + row * dp: off + row * dp + CW * 4] = False
    srows = SH * (3 if planar else 1)
    for row in range(srows):
        mask[soff + row * sp: soff + row * sp + row_bytes] = False
    assert (buf[mask] == SENT).all()
    assert np.array_equal(buf[soff:soff + sp * srows].reshape(-1, sp)[:, :row_bytes], mem.reshape(-1, row_bytes))
    arena.free()


# ---- 200 seeded random cases against the chain -------------------------------------------------------------------
def _random_case(rng):
    sfmt = SRC[int(rng.integers(3))]
    dfmt, norm = OUTS[int(rng.integers(len(OUTS)))]
    small = rng.integers(4) == 0        # a quarter of the cases live among the tiny sizes
    hi = 9 if small else 701
    sw, sh, cw, ch = (int(v) for v in rng.integers(1, hi, 4))

    def rect(W, H):
        w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
        return int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h

    crop, place = rect(sw, sh), rect(cw, ch)
    if rng.integers(4) == 0:            # equal sizes where they fit
        w, h = min(crop[2], place[2]), min(crop[3], place[3])
        crop, place = crop[:2] + (w, h), place[:2] + (w, h)
    pad = tuple(int(v) for v in rng.integers(0, 256, 3)) if rng.integers(2) else None
    return sfmt, dfmt, norm, sw, sh, cw, ch, crop, place, pad


@pytest.mark.parametrize("chunk", range(8))
def test_random_cases_against_the_chain(vali, gpu, chunk):
    rng = np.random.default_rng(1000 + chunk)
    for k in range(25):
        sfmt, dfmt, norm, sw, sh, cw, ch, crop, place, pad = case = _random_case(rng)
        src = upload(vali, gpu, colour_image(sw, sh, seed=chunk * 100 + k), sfmt)
        got = canvas(vali, gpu, dfmt, cw, ch)
        assert preprocessor(vali, gpu, norm).RunRoi(src, got, crop, place, pad) == (True, vali.TaskExecInfo.SUCCESS), case
        inner = chain_output(vali, gpu, chain_rgb_surface(vali, gpu, src, sfmt, crop, place[2], place[3]), dfmt, norm)
        want = expected_canvas(inner, dfmt, cw, ch, place, norm, pad)
        assert same_bits(as_image(download(vali, gpu, got), dfmt, cw, ch), want), case


# ---- decode -> network input ------------------------------------------------------------------------------------
def test_decoded_files_of_any_kind_become_network_input(vali, gpu, oracle):
    PIL = pytest.importorskip("PIL.Image")
    yy, xx = np.mgrid[0:375, 0:501]
    pic = np.stack([(xx + 40) % 256, (yy + xx // 3) % 256, (2 * yy + 9) % 256], -1).astype(np.uint8)
    files = []
    for img, kw in ((PIL.fromarray(pic), dict(subsampling=0)),                              # 4:4:4, odd size
                    (PIL.fromarray(pic[:251, :333]), dict(subsampling=2)),                  # 4:2:0, odd size
                    (PIL.fromarray(pic[:157, :200, 1]), {})):                               # grey
        out = io.BytesIO()
        img.save(out, "JPEG", quality=90, **kw)
        files.append(out.getvalue())
    dec = vali.PyNvJpegDecoder(gpu)
    assert [dec.Info(f).sampling for f in files[:2]] == ["444", "420"]
    frames, status = dec.Run(files, vali.RGB)
    assert status == vali.TaskExecInfo.SUCCESS
    pp = preprocessor(vali, gpu, "imagenet")
    dsts = [canvas(vali, gpu, "RGB_32F_PLANAR", 299, 299) for _ in frames]
    places = []
    for f in frames:        # centred, aspect-preserving, any integers
        s = min(299 / f.Width, 299 / f.Height)
        w, h = min(299, round(f.Width * s)), min(299, round(f.Height * s))
        places.append(((299 - w) // 2, (299 - h) // 2, w, h))
    assert pp.RunRoiBatch(pp.PrepareRoiBatch(frames, dsts, None, places), (114, 114, 114)) == (
        True, vali.TaskExecInfo.SUCCESS)
    for f, d, place in zip(files, dsts, places):
        ref = np.asarray(PIL.open(io.BytesIO(f)).convert("RGB"))
        h, w, _ = ref.shape
        inner = oracle_inner(oracle, ref, (0, 0, w, h), place[2], place[3], "RGB_32F_PLANAR", "imagenet")
        want = expected_canvas(inner, "RGB_32F_PLANAR", 299, 299, place, "imagenet", (114, 114, 114))
        assert same_bits(as_image(download(vali, gpu, d), "RGB_32F_PLANAR", 299, 299), want)
