"""Regions of surfaces as JPEG, without a GPU: the host-only planner vali_jpeg_plan_rois through ctypes (every rule with
its message, the layout it promises), what vali_jpeg_encode_rois refuses before it touches a device, the ValueErrors of
PyNvJpegEncoder.RunRoi up to the point where a surface is needed, and the crop model (tests/jpeg_roi_model.py)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import jpeg_model as jm
import jpeg_roi_model as rm

ROOT = Path(__file__).resolve().parent.parent
I32 = ctypes.c_int32


class Params(ctypes.Structure):
    _fields_ = [("quality", I32), ("format", I32), ("h_samp", I32), ("v_samp", I32), ("restart_interval", I32),
                ("optimize", I32), ("reserved", I32 * 2), ("qtable", (ctypes.c_uint8 * 64) * 2)]


class Roi(ctypes.Structure):
    _fields_ = [("x", I32), ("y", I32), ("width", I32), ("height", I32)]


class Item(ctypes.Structure):
    _fields_ = [("x", I32), ("y", I32), ("width", I32), ("height", I32), ("mcux", I32), ("mcuy", I32), ("nblocks", I32),
                ("nseg", I32), ("cw", I32 * 3), ("ch", I32 * 3), ("bw", I32 * 3), ("bh", I32 * 3),
                ("wg_fdct", ctypes.c_uint32), ("wg_hist", ctypes.c_uint32), ("wg_seg", ctypes.c_uint32),
                ("check", ctypes.c_uint32), ("block_first", ctypes.c_uint64), ("seg_first", ctypes.c_uint64),
                ("out_offset", ctypes.c_uint64), ("reserved", ctypes.c_uint64)]


SAMPLINGS = {"444": (1, 1), "422": (2, 1), "420": (2, 2)}
# (format, sampling of the files)
SOURCES = [(jm.RGB, "444"), (jm.BGR, "422"), (jm.RGB_PLANAR, "420"), (jm.YUV444, "444"), (jm.YUV422, "422"),
           (jm.YUV420, "420")]


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(str(ROOT / "vali_amd" / "libvali_hip.so"))
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    lib.vali_last_error.restype = ctypes.c_char_p
    lib.vali_jpeg_plan_rois.argtypes = [vp, vp, vp, ctypes.c_int, vp, vp, vp, vp]
    lib.vali_jpeg_encode_rois.argtypes = [vp, vp, vp, ctypes.c_int, vp, vp, sz, vp, sz, vp, vp]
    lib.vali_jpeg_workspace_size.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp]
    lib.vali_jpeg_stream_capacity.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp]
    return lib


def params(lib, fmt, samp, q=90, optimize=0):
    p = Params()
    H, V = SAMPLINGS[samp]
    assert lib.vali_jpeg_params_init_sampled(q, fmt, H, V, ctypes.byref(p)) == 0
    p.optimize = optimize
    return p


def plan(lib, p, rects, sizes):
    """(rc, items, ws_bytes, out_bytes) of vali_jpeg_plan_rois for rects[i] on a surface of sizes[i]"""
    n = len(rects)
    rois = (Roi * max(n, 1))(*[Roi(*r) for r in rects])
    sw = (I32 * max(n, 1))(*[s[0] for s in sizes])
    sh = (I32 * max(n, 1))(*[s[1] for s in sizes])
    items = (Item * max(n, 1))()
    ws, out = ctypes.c_size_t(12345), ctypes.c_size_t(12345)
    rc = lib.vali_jpeg_plan_rois(rois, sw, sh, n, ctypes.byref(p), items, ctypes.byref(ws), ctypes.byref(out))
    return rc, items, ws.value, out.value


def capacity(lib, p, w, h):
    cap = ctypes.c_size_t(0)
    assert lib.vali_jpeg_stream_capacity(w, h, ctypes.byref(p), ctypes.byref(cap)) == 0
    return cap.value


def align256(v):
    return -(-v // 256) * 256


def test_struct_sizes_are_those_of_the_header():
    text = (ROOT / "include" / "vali_hip.h").read_text()
    assert ctypes.sizeof(Roi) == 16 and re.search(r"\} vali_jpeg_roi;\s*/\* 16 bytes \*/", text)
    assert ctypes.sizeof(Item) == 128 and re.search(r"\} vali_jpeg_item;\s*/\* 128 bytes \*/", text)
    assert Item.wg_fdct.offset == 80 and Item.block_first.offset == 96 and Item.out_offset.offset == 112
    from vali_amd._native import shim
    from vali_amd.codecs import _JPEG_ITEM

    assert shim.JPEG_ITEM_SIZE == 128 and _JPEG_ITEM.itemsize == 128
    for name in ("wg_fdct", "block_first", "seg_first", "out_offset"):
        assert _JPEG_ITEM.fields[name][1] == getattr(Item, name).offset, name


@pytest.mark.parametrize("fmt, samp", SOURCES)
def test_every_rule_is_refused_with_its_message(lib, fmt, samp):
    p = params(lib, fmt, samp)
    size = (64, 48)
    bad = [((0, 0, 0, 8), "1..65535"), ((0, 0, 8, 0), "1..65535"), ((0, 0, 65536, 8), "1..65535"),
           ((0, 0, 8, -2), "1..65535"),
           ((-2, 0, 8, 8), "does not lie inside"), ((0, -2, 8, 8), "does not lie inside"),
           ((58, 0, 8, 8), "does not lie inside"), ((0, 42, 8, 8), "does not lie inside"),
           ((2**31 - 2, 0, 8, 8), "does not lie inside"), ((0, 2**31 - 2, 8, 8), "does not lie inside")]
    if fmt == jm.YUV420:
        bad += [((1, 0, 8, 8), "even"), ((0, 1, 8, 8), "even"), ((0, 0, 7, 8), "even"), ((0, 0, 8, 7), "even")]
    if fmt == jm.YUV422:
        bad += [((1, 0, 8, 8), "even"), ((0, 0, 7, 8), "even")]
    for r, what in bad:
        # the bad item is the second of three: the message names it
        rc, _, ws, out = plan(lib, p, [(0, 0, 8, 8), r, (8, 8, 8, 8)], [size] * 3)
        msg = lib.vali_last_error().decode()
        assert rc == -1 and "vali_jpeg_plan_rois" in msg and "item 1" in msg and what in msg, (r, msg)
    good = [(0, 0, 64, 48), (56, 40, 8, 8)]
    if fmt == jm.YUV422:
        good += [(2, 1, 6, 7)]                      # odd rows are fine at 4:2:2
    if fmt in rm.RGB_FORMATS + (jm.YUV444,):
        good += [(1, 3, 7, 5), (63, 47, 1, 1)]      # any integers, at every sampling
    rc, _, _, _ = plan(lib, p, good, [size] * len(good))
    assert rc == 0, lib.vali_last_error()


def test_batch_size_params_and_null_arguments(lib):
    p = params(lib, jm.RGB, "420")
    one = [(0, 0, 8, 8)]
    rois, sw, sh, items = (Roi * 1)(Roi(0, 0, 8, 8)), (I32 * 1)(8), (I32 * 1)(8), (Item * 1)()
    ws, out = ctypes.c_size_t(0), ctypes.c_size_t(0)
    for n in (-1, 65536):
        assert lib.vali_jpeg_plan_rois(rois, sw, sh, n, ctypes.byref(p), items, ctypes.byref(ws), ctypes.byref(out)) == -1
        assert "batch size" in lib.vali_last_error().decode()
    for args in ((None, sw, sh, 1, ctypes.byref(p), items, ctypes.byref(ws), ctypes.byref(out)),
                 (rois, None, sh, 1, ctypes.byref(p), items, ctypes.byref(ws), ctypes.byref(out)),
                 (rois, sw, None, 1, ctypes.byref(p), items, ctypes.byref(ws), ctypes.byref(out)),
                 (rois, sw, sh, 1, None, items, ctypes.byref(ws), ctypes.byref(out)),
                 (rois, sw, sh, 1, ctypes.byref(p), None, ctypes.byref(ws), ctypes.byref(out)),
                 (rois, sw, sh, 1, ctypes.byref(p), items, None, ctypes.byref(out)),
                 (rois, sw, sh, 1, ctypes.byref(p), items, ctypes.byref(ws), None)):
        assert lib.vali_jpeg_plan_rois(*args) == -1
        assert "null" in lib.vali_last_error().decode()
    # what jpeg_geom refuses in params
    for field, value, what in (("optimize", 2, "optimize"), ("restart_interval", 0, "restart interval"),
                               ("restart_interval", 11, "restart interval"), ("h_samp", 3, "sampling")):
        q = params(lib, jm.RGB, "420")
        setattr(q, field, value)
        assert plan(lib, q, one, [(8, 8)])[0] == -1
        assert what in lib.vali_last_error().decode()
    q = params(lib, jm.RGB, "420")
    q.qtable[1][5] = 0
    assert plan(lib, q, one, [(8, 8)])[0] == -1 and "quantisation table" in lib.vali_last_error().decode()
    q = params(lib, jm.RGB, "420")
    q.format = 3                                     # NV12 stays refused
    assert plan(lib, q, one, [(8, 8)])[0] == -2 and "cannot be encoded" in lib.vali_last_error().decode()
    # one image's output slot stays addressable with 32 bits
    rc, _, _, _ = plan(lib, params(lib, jm.RGB, "444"), [(0, 0, 65535, 65535)], [(65535, 65535)])
    assert rc == -1 and "too large" in lib.vali_last_error().decode()


def test_no_items(lib):
    p = params(lib, jm.RGB, "420")
    ws, out = ctypes.c_size_t(7), ctypes.c_size_t(7)
    assert lib.vali_jpeg_plan_rois(None, None, None, 0, ctypes.byref(p), None, ctypes.byref(ws), ctypes.byref(out)) == 0
    assert (ws.value, out.value) == (0, 0)


@pytest.mark.parametrize("optimize", [0, 1])
@pytest.mark.parametrize("fmt, samp", SOURCES)
def test_layout_of_a_mixed_batch(lib, fmt, samp, optimize):
    p = params(lib, fmt, samp, optimize=optimize)
    H, V = SAMPLINGS[samp]
    bpm, R = H * V + 2, p.restart_interval
    sizes = [(1920, 1080), (64, 48), (1920, 1080), (640, 360)]
    rects = [(0, 0, 1920, 1080), (2, 2, 2, 2), (100, 200, 250, 136), (0, 0, 640, 360), (2, 2, 2, 2), (40, 20, 64, 64)]
    on = [0, 1, 2, 3, 1, 0]
    rc, items, ws, out = plan(lib, p, rects, [sizes[k] for k in on])
    assert rc == 0, lib.vali_last_error()
    per_wg = 256 // bpm * bpm if fmt in rm.RGB_FORMATS and samp != "444" else 256
    blocks = segs = outs = wg_f = wg_h = 0
    for it, (x, y, w, h) in zip(items, rects):
        assert (it.x, it.y, it.width, it.height) == (x, y, w, h)
        mcux, mcuy = -(-w // (8 * H)), -(-h // (8 * V))
        assert (it.mcux, it.mcuy, it.nblocks, it.nseg) == (mcux, mcuy, mcux * mcuy * bpm, -(-mcux * mcuy // R))
        assert list(it.cw) == [w, -(-w // H), -(-w // H)] and list(it.ch) == [h, -(-h // V), -(-h // V)]
        assert list(it.bw) == [-(-c // 8) for c in it.cw] and list(it.bh) == [-(-c // 8) for c in it.ch]
        # monotone, each image after the whole of the one before
        assert (it.block_first, it.seg_first, it.out_offset) == (blocks, segs, outs)
        assert (it.wg_fdct, it.wg_hist, it.wg_seg) == (wg_f, wg_h, segs)
        blocks, segs = blocks + it.nblocks, segs + it.nseg
        outs += capacity(lib, p, w, h)
        wg_f, wg_h = wg_f + -(-it.nblocks // per_wg), wg_h + -(-it.nseg // 16)
    assert out == outs
    slot = 2 * R * bpm * 208
    parts = blocks * 128 + 2 * segs * 4 + segs * slot
    if optimize:
        parts += len(rects) * (2 * 4 * 256 * 4 + 4 * 288 + 4 * 4)
    assert parts <= ws <= parts + 8 * 256


@pytest.mark.parametrize("optimize", [0, 1])
def test_whole_surfaces_of_one_size_take_the_uniform_workspace(lib, optimize):
    for (fmt, samp), (w, h), n in zip(SOURCES, [(1920, 1080), (424, 232), (33, 31), (64, 48), (130, 70), (2, 2)],
                                      [8, 3, 5, 1, 64, 2]):
        if fmt in (jm.YUV422, jm.YUV420):
            w, h = w + (w & 1), h + (h & 1)
        p = params(lib, fmt, samp, optimize=optimize)
        rc, items, ws, out = plan(lib, p, [(0, 0, w, h)] * n, [(w, h)] * n)
        assert rc == 0, lib.vali_last_error()
        uniform = ctypes.c_size_t(0)
        assert lib.vali_jpeg_workspace_size(n, w, h, ctypes.byref(p), ctypes.byref(uniform)) == 0
        assert abs(ws - uniform.value) <= 4 * 256, (fmt, samp, ws, uniform.value)
        assert out == n * capacity(lib, p, w, h)
        assert [it.out_offset for it in items] == [k * capacity(lib, p, w, h) for k in range(n)]


def test_encode_refuses_before_any_device_is_touched(lib):
    p = params(lib, jm.RGB, "420")
    rects, sizes = [(0, 0, 64, 48), (3, 5, 17, 9)], [(64, 48), (64, 48)]
    rc, items, ws, out = plan(lib, p, rects, sizes)
    assert rc == 0
    fake = ctypes.c_void_p(1 << 20)                  # aligned, never read: the arguments are judged first

    def call(d_src=fake, it=items, d_it=fake, n=2, pp=p, w=fake, wsb=ws, o=fake, ob=out, sz=fake):
        return lib.vali_jpeg_encode_rois(d_src, it, d_it, n, ctypes.byref(pp) if pp is not None else None, w, wsb, o,
                                         ob, sz, None)

    for kw in (dict(d_src=None), dict(it=None), dict(d_it=None), dict(pp=None), dict(w=None), dict(o=None),
               dict(sz=None)):
        assert call(**kw) == -1 and "null" in lib.vali_last_error().decode(), kw
    assert call(w=ctypes.c_void_p((1 << 20) + 128)) == -1 and "aligned" in lib.vali_last_error().decode()
    assert call(wsb=ws - 1) == -1 and "workspace" in lib.vali_last_error().decode()
    assert call(ob=out - 1) == -1 and "output" in lib.vali_last_error().decode()
    assert call(n=65536) == -1 and "batch size" in lib.vali_last_error().decode()
    # items the planner did not make for these params
    for other in (params(lib, jm.RGB, "444"), params(lib, jm.RGB, "420", optimize=1), params(lib, jm.BGR, "420")):
        assert call(pp=other) == -1 and "vali_jpeg_plan_rois" in lib.vali_last_error().decode()
    shorter = params(lib, jm.RGB, "420")
    shorter.restart_interval = 5
    assert call(pp=shorter) == -1 and "vali_jpeg_plan_rois" in lib.vali_last_error().decode()
    for field, value in (("width", 18), ("nblocks", 13), ("wg_fdct", 0), ("out_offset", 8), ("seg_first", 1),
                         ("block_first", 0), ("reserved", 1)):
        rc, tampered, _, _ = plan(lib, p, rects, sizes)
        setattr(tampered[1], field, value)
        assert call(it=tampered) == -1 and "item 1" in lib.vali_last_error().decode(), field
    swapped = (Item * 2)(items[1], items[0])
    assert call(it=swapped) == -1 and "item 0" in lib.vali_last_error().decode()


# ---- PyNvJpegEncoder.RunRoi, up to the point where a surface is needed ---------------------------------------------------
def _encoder(vali):
    """an encoder without its device-side parts: everything below is refused before one is needed"""
    enc = object.__new__(vali.PyNvJpegEncoder)
    enc._backend, enc._gpu_id, enc._stream = "hip", 0, 0
    return enc


def test_run_roi_value_errors_without_a_surface(vali):
    enc = _encoder(vali)
    ctx = vali.PyNvJpegEncoder.Context(enc, 90, vali.RGB, subsampling="420")
    with pytest.raises(ValueError, match="2 rectangles for 1 surfaces"):
        enc.RunRoi(ctx, [None], [None, None])
    for rect, what in (((0, 0, 8), "four integers"), ((0, 0, 8, 8, 8), "four integers"), ((0, 0, 8.5, 8), "four integers"),
                       ("abcd", "four integers"), (7, "four integers"), ((0, 0, 0, 8), "1..65535"),
                       ((0, 0, 8, 65536), "1..65535"), ((-1, 0, 8, 8), "outside"), ((0, -4, 8, 8), "outside")):
        with pytest.raises(ValueError, match="item 1.*" + what):
            enc.RunRoi(ctx, [None, None], [None, rect])
    # a missing surface is a failed call, not an exception; nothing is no work
    assert enc.RunRoi(ctx, [None], [(0, 0, 8, 8)]) == ([], vali.TaskExecInfo.FAIL)
    assert enc.RunRoi(ctx, [None]) == ([], vali.TaskExecInfo.FAIL)
    assert enc.RunRoi(ctx, []) == ([], vali.TaskExecInfo.SUCCESS)
    assert enc.RunRoi(ctx, [], []) == ([], vali.TaskExecInfo.SUCCESS)


def test_python_vali_reexports_run_roi(vali):
    import python_vali

    assert python_vali.PyNvJpegEncoder.RunRoi is vali.PyNvJpegEncoder.RunRoi
    assert "GPU memory" in vali.PyNvJpegEncoder.RunRoi.__doc__


# ---- the model is "crop, then the whole-surface model" ------------------------------------------------------------------
@pytest.mark.parametrize("fmt", jm.FORMATS)
def test_model_crops_every_layout(fmt):
    sw, sh = 40, 24
    host = jm.make_host(fmt, sw, sh, "noise", seed=3)
    rect = (6, 4, 18, 10)
    x, y, w, h = rect
    got = rm.crop(fmt, host, sw, sh, rect)
    assert got.size == jm.make_host(fmt, w, h, "noise").size
    planes, whole = jm.planes_of(fmt, got, w, h), jm.planes_of(fmt, host, sw, sh)
    if fmt in rm.RGB_FORMATS:
        for a, b in zip(planes, whole):
            assert np.array_equal(a, b[y:y + h, x:x + w])
    else:
        dx, dy = whole[0].shape[1] // whole[1].shape[1], whole[0].shape[0] // whole[1].shape[0]
        assert np.array_equal(planes[0], whole[0][y:y + h, x:x + w])
        for a, b in zip(planes[1:], whole[1:]):
            assert np.array_equal(a, b[y // dy:(y + h) // dy, x // dx:(x + w) // dx])
    # the library's own host crop (the cpu backend) is the same function of the same bytes
    from vali_amd.codecs import _crop_host
    from vali_amd.enums import PixelFormat

    assert np.array_equal(_crop_host(PixelFormat(fmt), sw, sh, host, *rect), got)
    assert rm.encode(fmt, host, sw, sh, None, 90) == rm.encode_crop(fmt, host, sw, sh, 90)
    for opt in (False, True):
        samp = "420" if fmt in rm.RGB_FORMATS else None
        assert rm.encode(fmt, host, sw, sh, rect, 75, samp, opt) == rm.encode_crop(fmt, got, w, h, 75, samp, opt)
