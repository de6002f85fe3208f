"""Regions of the fused preprocessor on the GPU: PySurfacePreprocessor.RunRoi* / RunRoiBatch*.

The definition (include/vali_hip.h, vali_nv12_preproc_roi): inside the placement, bit-identical to vali_nv12_preproc on
the view of the crop and the view of the placement; outside it the pad colour through the same normalisation, or the
bytes are not written.  Checked against that definition on view descriptors (shim.nv12_preproc), against the CPU
oracle, in batches (sources of several sizes, a mosaic, device-supplied rectangles, a captured graph), and with
malformed device rectangles inside one sentinel-filled arena (what the kernel's sanitising must contain)."""
import numpy as np
import pytest

from conftest import make_nv12

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
NORMS = {"imagenet": (255.0, MEAN, STD), "identity": (1.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))}
SENT = 0x5A
PAD = (10, 200, 77)        # not grey: catches a channel-order slip
# bytes per pixel of a destination view, planes, element type, host layout
DST = {"RGB_32F_PLANAR": (4, 3, np.float32, "CHW"), "RGB_32F": (12, 1, np.float32, "HWC"),
       "RGB": (3, 1, np.uint8, "HWC"), "BGR": (3, 1, np.uint8, "HWC"), "RGB_PLANAR": (1, 3, np.uint8, "CHW")}

# (src_w, src_h, crop, canvas_w, canvas_h, place)
GEOMS = {
    "crop_2x2_up": (64, 48, (10, 6, 2, 2), 32, 32, (6, 8, 8, 6)),
    "crop_right_bottom_edges": (130, 70, (66, 30, 64, 40), 96, 64, (4, 2, 60, 50)),
    "x_2_mod_4": (200, 120, (22, 10, 90, 60), 160, 100, (34, 6, 94, 70)),
    "upscale": (100, 80, (2, 2, 30, 20), 300, 200, (10, 20, 270, 170)),
    "downscale_tall": (640, 360, (102, 50, 400, 300), 224, 224, (2, 2, 218, 198)),
    "same_size": (320, 240, (50, 42, 130, 90), 300, 200, (38, 90, 130, 90)),
    "same_size_whole": (256, 128, (0, 0, 256, 128), 256, 128, (0, 0, 256, 128)),
    "wide_x_2_mod_4": (1280, 720, (2, 2, 1276, 716), 1300, 740, (6, 10, 1282, 718)),
    "letterbox_1080p": (1920, 1080, (0, 0, 1920, 1080), 640, 640, (0, 140, 640, 360)),
}


def upload(vali, gpu, host, w, h):
    s = vali.Surface.Make(vali.NV12, w, h, gpu)
    assert vali.PyFrameUploader(gpu).Run(np.ascontiguousarray(host).reshape(-1), s)[0]
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


def src_view(shim, s, x, y, w, h):
    p = s.Pitch
    return shim.SurfaceDesc([s.PixelPtr(0) + y * p + x, s.PixelPtr(1) + (y // 2) * p + x], [p, p], w, h, int(s.Format))


def dst_view(shim, d, fmt, x, y, w, h):
    bpp, planes, _, _ = DST[fmt]
    p = d.Pitch
    return shim.SurfaceDesc([d.PixelPtr(c) + y * p + x * bpp for c in range(planes)], [p] * planes, w, h,
                            int(d.Format))


def pad_pixel(fmt, norm, pad):
    """the pad colour as it lands in memory, per channel slot of the host layout"""
    if DST[fmt][2] == np.uint8:
        return np.array(pad[::-1] if fmt == "BGR" else pad, np.uint8)
    div, mean, std = norm
    q = np.asarray(pad, np.float32)
    return (((q / np.float32(255.0)) / np.float32(div) - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
            ).astype(np.float32)


def expected_canvas(view_raw, fmt, cw, ch, place, norm, pad):
    """the definition: the view result inside `place`; outside it the pad colour, or the sentinel (pad off)"""
    want = as_image(view_raw.copy(), fmt, cw, ch)
    if pad is not None:
        x, y, w, h = place
        outside = np.ones((ch, cw), bool)
        outside[y:y + h, x:x + w] = False
        pv = pad_pixel(fmt, norm, pad)
        if DST[fmt][3] == "CHW":
            for c in range(3):
                want[c][outside] = pv[c]
        else:
            want[outside] = pv
    return want


def configs():
    for g in GEOMS:
        for fmt in DST:
            for norm in (("imagenet", "identity") if DST[fmt][2] == np.float32 else ("identity",)):
                for pad in (True, False):
                    yield pytest.param(g, fmt, norm, pad, id=f"{g}-{fmt}-{norm}-{'pad' if pad else 'nopad'}")


@pytest.mark.parametrize("geom, fmt, norm, pad", list(configs()))
def test_roi_equals_preproc_on_views(vali, gpu, geom, fmt, norm, pad):
    from vali_amd._native import shim

    sw, sh, crop, cw, ch, place = GEOMS[geom]
    div, mean, std = NORMS[norm]
    host = make_nv12(sw, sh, seed=sw + ch)
    src = upload(vali, gpu, host, sw, sh)
    cc = vali.ColorspaceConversionContext(vali.ColorSpace.BT_709, vali.ColorRange.MPEG)
    pp = vali.PySurfacePreprocessor(gpu, mean=mean, std=std, div=div)
    got = canvas(vali, gpu, fmt, cw, ch)
    padc = PAD if pad else None
    assert pp.RunRoi(src, got, crop, place, padc, cc) == (True, vali.TaskExecInfo.SUCCESS)
    ref = canvas(vali, gpu, fmt, cw, ch)
    rc = shim.nv12_preproc(src_view(shim, src, *crop), dst_view(shim, ref, fmt, *place), pp._params(cc), pp.Stream)
    assert rc == 0, shim.last_error()
    shim.stream_sync(gpu, pp.Stream)
    want = expected_canvas(download(vali, gpu, ref), fmt, cw, ch, place, NORMS[norm], padc)
    g = as_image(download(vali, gpu, got), fmt, cw, ch)
    assert np.array_equal(g.view(np.uint8), want.view(np.uint8))


def torch_part(x, div, mean, std):
    x = x.astype(np.float32) / np.float32(div)
    return ((x - np.asarray(mean, np.float32)[:, None, None]) / np.asarray(std, np.float32)[:, None, None]).astype(
        np.float32)


def crop_host(host, sw, sh, crop):
    """the crop of a host NV12 image as a contiguous NV12 image of its own"""
    x, y, w, h = crop
    return np.concatenate([host[y:y + h, x:x + w], host[sh + y // 2:sh + (y + h) // 2, x:x + w]])


def oracle_chain(oracle, nv12, sw, sh, dw, dh, coeffs, div, mean, std):
    small = nv12 if (sw, sh) == (dw, dh) else oracle.resize_surface(
        np.ascontiguousarray(nv12).reshape(-1), "NV12", sw, sh, dw, dh).reshape(dh * 3 // 2, dw)
    rgb = oracle.nv12_to_rgb(np.ascontiguousarray(small), dw, dh, oracle.csc_from_tuple(coeffs), "RGB")
    x = (rgb.reshape(dh, dw, 3).astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)
    return torch_part(x, div, mean, std)


@pytest.mark.parametrize("geom", ["crop_2x2_up", "x_2_mod_4", "downscale_tall", "same_size", "letterbox_1080p"])
def test_roi_against_oracle(vali, gpu, oracle, geom):
    from vali_amd.tasks import CSC_NPP_709CSC

    sw, sh, crop, cw, ch, place = GEOMS[geom]
    host = make_nv12(sw, sh, seed=3 * sw + 1)
    src = upload(vali, gpu, host, sw, sh)
    cc = vali.ColorspaceConversionContext(vali.ColorSpace.BT_709, vali.ColorRange.MPEG)
    pp = vali.PySurfacePreprocessor(gpu, mean=MEAN, std=STD, div=255.0)
    dst = canvas(vali, gpu, "RGB_32F_PLANAR", cw, ch)
    assert pp.RunRoi(src, dst, crop, place, (114, 114, 114), cc)[0]
    got = as_image(download(vali, gpu, dst), "RGB_32F_PLANAR", cw, ch)
    x, y, w, h = place
    want = oracle_chain(oracle, crop_host(host, sw, sh, crop), crop[2], crop[3], w, h, CSC_NPP_709CSC, 255.0, MEAN, STD)
    assert np.array_equal(got[:, y:y + h, x:x + w].view(np.uint32), want.view(np.uint32))
    pv = pad_pixel("RGB_32F_PLANAR", NORMS["imagenet"], (114, 114, 114))
    assert np.array_equal(got[:, :y, :].reshape(3, -1).view(np.uint32),
                          np.broadcast_to(pv[:, None], (3, y * cw)).view(np.uint32))


def test_roi_errors(vali, gpu):
    I = vali.TaskExecInfo
    pp = vali.PySurfacePreprocessor(gpu)
    nv = vali.Surface.Make(vali.NV12, 64, 48, gpu)
    dst = vali.Surface.Make(vali.RGB_32F_PLANAR, 32, 32, gpu)
    for crop in ((1, 0, 4, 4), (0, 0, 66, 4), (-2, 0, 4, 4), (0, 0, 0, 4)):
        assert pp.RunRoi(nv, dst, crop) == (False, I.INVALID_INPUT)
    assert pp.RunRoi(nv, dst, None, (30, 30, 4, 4)) == (False, I.INVALID_INPUT)
    assert pp.RunRoi(nv, dst, None, None, (1, 2)) == (False, I.INVALID_INPUT)
    assert pp.RunRoi(nv, vali.Surface.Make(vali.YUV444, 32, 32, gpu)) == (False, I.NOT_SUPPORTED)
    assert pp.RunRoi(vali.Surface.Make(vali.YUV420, 64, 48, gpu), dst) == (False, I.NOT_SUPPORTED)
    norm = vali.PySurfacePreprocessor(gpu, mean=MEAN, std=STD, div=255.0)
    assert norm.RunRoi(nv, vali.Surface.Make(vali.RGB, 32, 32, gpu)) == (False, I.NOT_SUPPORTED)
    assert pp.RunRoi(nv, dst, (2, 2, 8, 8), (0, 0, 32, 32), (0, 0, 0)) == (True, I.SUCCESS)


def _batch_vs_single(vali, gpu, pp, srcs, crops, cw, ch, fmt, place, pad, cc):
    dsts = [canvas(vali, gpu, fmt, cw, ch) for _ in srcs]
    batch = pp.PrepareRoiBatch(srcs, dsts, crops, [place] * len(srcs))
    assert pp.RunRoiBatch(batch, pad, cc) == (True, vali.TaskExecInfo.SUCCESS)
    for s, c, d in zip(srcs, crops, dsts):
        one = canvas(vali, gpu, fmt, cw, ch)
        assert pp.RunRoi(s, one, c, place, pad, cc)[0]
        assert np.array_equal(download(vali, gpu, d), download(vali, gpu, one))
    return batch, dsts


def test_batch_mixed_sources_equals_single_calls(vali, gpu):
    sizes = [(1920, 1080), (640, 360), (1280, 720)]
    frames = [upload(vali, gpu, make_nv12(w, h, seed=w), w, h) for w, h in sizes]
    big = frames[0]
    boxes = [(0, 0, 32, 32), (1888, 1048, 32, 32), (100, 200, 512, 300), (998, 2, 2, 2), (6, 1000, 400, 80),
             (1000, 500, 918, 578), (640, 360, 224, 224), (2, 2, 1916, 1076)]
    srcs = frames + [big] * len(boxes)
    crops = [None, (10, 20, 300, 200), (2, 2, 1276, 716)] + boxes
    cc = vali.ColorspaceConversionContext(vali.ColorSpace.BT_601, vali.ColorRange.JPEG)
    pp = vali.PySurfacePreprocessor(gpu, mean=MEAN, std=STD, div=255.0)
    _batch_vs_single(vali, gpu, pp, srcs, crops, 224, 224, "RGB_32F_PLANAR", (0, 20, 224, 184), (114, 114, 114), cc)
    pp8 = vali.PySurfacePreprocessor(gpu)
    _batch_vs_single(vali, gpu, pp8, srcs, crops, 640, 640, "BGR", vali.letterbox_rect(1920, 1080, 640, 640), PAD, None)


def test_batch_mosaic_without_padding(vali, gpu):
    sizes = [(640, 360), (320, 240), (1280, 720), (200, 200)]
    srcs = [upload(vali, gpu, make_nv12(w, h, seed=7 + w), w, h) for w, h in sizes]
    pp = vali.PySurfacePreprocessor(gpu, mean=MEAN, std=STD, div=255.0)
    cells = [(0, 0, 320, 320), (322, 0, 318, 320), (0, 322, 320, 318), (322, 322, 318, 318)]
    mosaic = canvas(vali, gpu, "RGB_32F", 640, 640)
    batch = pp.PrepareRoiBatch(srcs, [mosaic] * 4, None, cells)
    assert pp.RunRoiBatch(batch) == (True, vali.TaskExecInfo.SUCCESS)
    want = canvas(vali, gpu, "RGB_32F", 640, 640)
    for s, cell in zip(srcs, cells):
        assert pp.RunRoi(s, want, None, cell)[0]
    got = download(vali, gpu, mosaic)
    assert np.array_equal(got, download(vali, gpu, want))
    img = as_image(got, "RGB_32F", 640, 640).view(np.uint8).reshape(640, 640, 12)
    assert (img[320:322] == SENT).all() and (img[:, 320:322] == SENT).all()     # the gaps were never written

    # n = 0 is a no-op
    from vali_amd._native import shim

    fill(gpu, mosaic)
    rc = shim.nv12_preproc_roi_batch(batch.d_src, batch.d_dst, batch.d_roi, 0, 640, 640, int(vali.RGB_32F),
                                     pp._params(None), True, (1, 2, 3), pp.Stream)
    assert rc == 0
    shim.stream_sync(gpu, pp.Stream)
    assert (download(vali, gpu, mosaic) == SENT).all()


def _torch_rects(rects):
    import torch

    t = torch.tensor(rects, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    return t


def test_device_rects_equal_uploaded_rects(vali, gpu):
    host = make_nv12(1920, 1080, seed=5)
    frame = upload(vali, gpu, host, 1920, 1080)
    boxes = [(0, 0, 64, 128), (500, 300, 300, 300), (1856, 1016, 64, 64), (100, 900, 800, 180)]
    place = (0, 0, 224, 224)
    pp = vali.PySurfacePreprocessor(gpu, mean=MEAN, std=STD, div=255.0)
    d1 = [canvas(vali, gpu, "RGB_32F_PLANAR", 224, 224) for _ in boxes]
    b1 = pp.PrepareRoiBatch([frame] * 4, d1, boxes)
    assert pp.RunRoiBatch(b1, (114, 114, 114))[0]
    d2 = [canvas(vali, gpu, "RGB_32F_PLANAR", 224, 224) for _ in boxes]
    b2 = pp.PrepareRoiBatch([frame] * 4, d2, [None] * 4)          # uploaded rects: whole frame
    t = _torch_rects([list(b) + list(place) for b in boxes])
    assert pp.RunRoiBatch(b2, (114, 114, 114), rects=t) == (True, vali.TaskExecInfo.SUCCESS)
    for a, b in zip(d1, d2):
        assert np.array_equal(download(vali, gpu, a), download(vali, gpu, b))

    class DlpackOnly:                       # the DLPack path of the same tensor
        def __init__(self, t):
            self._t = t

        def __dlpack__(self, stream=None):
            return self._t.__dlpack__()

    d3 = [canvas(vali, gpu, "RGB_32F_PLANAR", 224, 224) for _ in boxes]
    b3 = pp.PrepareRoiBatch([frame] * 4, d3)
    assert pp.RunRoiBatch(b3, (114, 114, 114), rects=DlpackOnly(t))[0]
    for a, b in zip(d1, d3):
        assert np.array_equal(download(vali, gpu, a), download(vali, gpu, b))
    import torch
    with pytest.raises(ValueError):
        pp.RunRoiBatch(b3, rects=t[:3])
    with pytest.raises(ValueError):
        pp.RunRoiBatch(b3, rects=t.to(torch.int64))
    with pytest.raises(ValueError):
        pp.RunRoiBatch(b3, rects=torch.zeros((8, 4), dtype=torch.int32, device="cuda:0").t())
    with pytest.raises(ValueError):
        pp.RunRoiBatch(b3, rects=t.cpu())


class Arena:
    """one device buffer filled with the sentinel; every surface of the test is carved out of it"""

    def __init__(self, gpu, size):
        from vali_amd._native import shim

        self.shim, self.gpu, self.size = shim, gpu, size
        self.ptr = shim.mem_alloc(gpu, size)
        shim.memset2d_async(gpu, self.ptr, size, SENT, size, 1, 0)
        shim.stream_sync(gpu, 0)
        self.cursor, self.regions = 0, []

    def carve(self, row_bytes, rows, pitch=None):
        off = ((self.cursor + 255) // 256) * 256
        pitch = pitch or row_bytes
        self.cursor = off + pitch * rows + 256          # a gap after every region, checked for the sentinel
        assert self.cursor <= self.size
        self.regions.append((off, pitch, row_bytes, rows))
        return off, pitch

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
    """the kernel's rule for one axis (include/vali_hip.h)"""
    x, w = v
    size = max(size, 0)
    x = min(max(x, 0), size) & ~1
    w = min(max(w, 0), size - x) & ~1
    return x, w


def test_device_rects_are_sanitised_and_contained(vali, gpu):
    from vali_amd._native import shim

    SW, SH, CW, CH = 130, 70, 64, 48
    big = 2 ** 31 - 1
    rects = [
        (100, 10, 60, 40, 0, 0, 64, 48),           # crop runs past the right edge
        (-10, 4, 50, 30, -4, -6, 40, 40),          # negative x / placement
        (5, 7, 33, 21, 3, 3, 31, 31),              # odd everything
        (10, 10, 1, 40, 0, 0, 64, 48),             # empty crop
        (0, 0, big, big, 60, 44, 100, 100),        # huge sizes, placement in the corner
        (0, 0, 64, 64, 70, 0, 10, 10),             # placement beyond the canvas: empty
        (-big - 1, -big - 1, big, big, 2, 2, -8, 20),   # negative width: empty
    ]
    n = len(rects)
    host = make_nv12(SW, SH, seed=99)
    arena = Arena(gpu, 1 << 20)
    soff, sp = arena.carve(SW, SH * 3 // 2, pitch=SW + 6)
    arena.upload(soff, sp, host)
    src = shim.SurfaceDesc([arena.ptr + soff, arena.ptr + soff + SH * sp], [sp, sp], SW, SH, int(vali.NV12))
    dsts, dregions = [], []
    for _ in range(n):
        off, dp = arena.carve(CW * 4, CH * 3, pitch=CW * 4 + 20)
        dregions.append((off, dp))
        dsts.append(shim.SurfaceDesc([arena.ptr + off + c * CH * dp for c in range(3)], [dp] * 3, CW, CH,
                                     int(vali.RGB_32F_PLANAR)))
    pp = vali.PySurfacePreprocessor(gpu, mean=MEAN, std=STD, div=255.0)
    p = pp._params(None)
    d_src = shim.descs_upload(gpu, [src] * n, pp.Stream)
    d_dst = shim.descs_upload(gpu, dsts, pp.Stream)
    t = _torch_rects([list(r) for r in rects])
    try:
        rc = shim.nv12_preproc_roi_batch(d_src, d_dst, t.data_ptr(), n, CW, CH, int(vali.RGB_32F_PLANAR), p, True,
                                         (114, 114, 114), pp.Stream)
        assert rc == 0, shim.last_error()
        shim.stream_sync(gpu, pp.Stream)
        buf = arena.download()
    finally:
        shim.mem_free(gpu, d_src)
        shim.mem_free(gpu, d_dst)
    nv = upload(vali, gpu, host, SW, SH)
    pv = pad_pixel("RGB_32F_PLANAR", NORMS["imagenet"], (114, 114, 114))
    for r, (off, dp) in zip(rects, dregions):
        sx, sw = _sanitise((r[0], r[2]), SW)
        sy, sh = _sanitise((r[1], r[3]), SH)
        dx, dw = _sanitise((r[4], r[6]), CW)
        dy, dh = _sanitise((r[5], r[7]), CH)
        got = buf[off:off + 3 * CH * dp].reshape(3 * CH, dp)[:, :CW * 4].reshape(3, CH, CW * 4)
        if min(sw, sh, dw, dh) < 2:
            want = np.broadcast_to(pv[:, None, None], (3, CH, CW)).astype(np.float32)
        else:
            one = canvas(vali, gpu, "RGB_32F_PLANAR", CW, CH)
            assert pp.RunRoi(nv, one, (sx, sy, sw, sh), (dx, dy, dw, dh), (114, 114, 114))[0]
            want = as_image(download(vali, gpu, one), "RGB_32F_PLANAR", CW, CH)
        assert np.array_equal(got, np.ascontiguousarray(want).view(np.uint8).reshape(3, CH, CW * 4)), r
    # containment: every byte outside the destination rows (pitch padding, gaps, the rest of the arena) is the
    # sentinel, and the source is unchanged
    mask = np.ones(arena.size, bool)
    for off, dp in dregions:
        for row in range(3 * CH):
            mask[off + row * dp: off + row * dp + CW * 4] = False
    for row in range(SH * 3 // 2):
        mask[soff + row * sp: soff + row * sp + SW] = False
    assert (buf[mask] == SENT).all()
    assert np.array_equal(buf[soff:soff + sp * SH * 3 // 2].reshape(-1, sp)[:, :SW], host)
    arena.free()


def test_capture_reads_rects_from_a_device_tensor(vali, gpu):
    from vali_amd._native import shim

    stream = shim.stream_create(gpu)
    pp = vali.PySurfacePreprocessor(gpu, stream, mean=MEAN, std=STD, div=255.0)
    frame = upload(vali, gpu, make_nv12(1280, 720, seed=11), 1280, 720)
    n = 6
    dsts = [canvas(vali, gpu, "RGB_32F_PLANAR", 224, 224) for _ in range(n)]
    batch = pp.PrepareRoiBatch([frame] * n, dsts)
    first = [[40 * i, 20 * i, 200, 100, 0, 62, 224, 100] for i in range(n)]
    second = [[1280 - 64 * (i + 1), 720 - 96, 64 * (i + 1), 96, 10, 2, 200, 220] for i in range(n)]
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
