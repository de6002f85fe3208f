"""MARK_STAMP / vali_annotate_batch_atlas without a GPU: the identities of the model (tests/annotate_stamp_model.py),
pack_uv, the host-marks checker with an atlas, render_labels, and every refusal of the C entry point."""
import ctypes
import types
from pathlib import Path

import numpy as np
import pytest

import annotate_model as am
import annotate_stamp_model as sm

ROOT = Path(__file__).resolve().parent.parent
ROWS = ((0.299, 0.587, 0.114, 0.0), (-0.147, -0.289, 0.436, 128.0), (0.615, -0.515, -0.100, 128.0))


def one(fmt, w, h, marks, atlas, seed=1):
    flat = am.noise_frame(fmt, w, h, seed)
    before = flat.copy()
    drawn = sm.apply([flat], fmt, [(w, h)], marks, ROWS, atlas)
    return before, flat, drawn


def noise_atlas(aw, ah, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (ah, aw), dtype=np.uint8)


# ---- the model's identities ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", am.FORMATS)
def test_full_coverage_is_fill(fmt):
    w, h = 24, 16
    full = np.full((12, 20), 255, np.uint8)
    for a in (255, 128, 1):
        c = am.pack_colour(9, 200, 77, a)
        _, stamp, drawn = one(fmt, w, h, [(0, 4, 2, 10, 8, sm.STAMP, sm.pack_uv(3, 1), c)], full)   # even x, y, w, h
        _, fill, _ = one(fmt, w, h, [(0, 4, 2, 10, 8, am.FILL, 0, c)], None)
        assert drawn == [0] and np.array_equal(stamp, fill)


@pytest.mark.parametrize("fmt", am.FORMATS)
def test_zero_coverage_changes_nothing(fmt):
    before, after, drawn = one(fmt, 24, 16, [(0, 3, 1, 11, 9, sm.STAMP, 0, am.pack_colour(9, 200, 77))],
                               np.zeros((12, 20), np.uint8))
    assert drawn == [0] and np.array_equal(before, after)


@pytest.mark.parametrize("fmt", am.FORMATS)
def test_off_the_atlas_reads_zero(fmt):
    atlas = noise_atlas(9, 7)
    padded = np.zeros((40, 40), np.uint8)
    padded[:7, :9] = atlas
    row = (0, 3, 1, 15, 12, sm.STAMP, sm.pack_uv(4, 2), am.pack_colour(250, 10, 90, 200))     # u + 15 > 9, v + 12 > 7
    _, a, drawn = one(fmt, 24, 16, [row], atlas)
    _, b, _ = one(fmt, 24, 16, [row], padded)
    assert drawn == [0] and np.array_equal(a, b)
    # ... and changes nothing beyond the 5 x 5 pixels the atlas has for it
    before, after, _ = one(fmt, 24, 16, [row], atlas)
    for (v, sh, _), (v0, _, _) in zip(am.channels(fmt, after, 24, 16), am.channels(fmt, before, 24, 16)):
        touched = np.zeros(v.shape, bool)
        touched[1 >> sh:(6 + sh) >> sh, 3 >> sh:(8 + sh) >> sh] = True
        assert np.array_equal(v[~touched], v0[~touched])


@pytest.mark.parametrize("fmt", am.S420)
def test_chroma_weights_of_a_stamp_at_odd_coordinates(fmt):
    """[3, 7) x [5, 7) of coverage 255, opaque: luma is painted on exactly that rectangle (it is NOT snapped) and a
    chroma sample gets k = (255 * covered + 2) >> 2 for the `covered` of its four luma pixels inside: 1 -> 64, 2 -> 128.
    A rectangle gives a block 1, 2 or 4 pixels, so three (k = 191) takes a hole of one pixel in the coverage."""
    w, h = 16, 12
    colour = am.pack_colour(255, 255, 255, 255)
    cy, cu, cv = am.yuv_of(255, 255, 255, ROWS)
    atlas = np.full((8, 8), 255, np.uint8)
    before, after, _ = one(fmt, w, h, [(0, 3, 5, 4, 2, sm.STAMP, 0, colour)], atlas)
    ch, ch0 = am.channels(fmt, after, w, h), am.channels(fmt, before, w, h)
    painted = np.zeros((h, w), bool)
    painted[5:7, 3:7] = True
    assert (ch[0][0][painted] == cy).all() and np.array_equal(ch[0][0][~painted], ch0[0][0][~painted])
    # chroma rows 2 (luma 4, 5) and 3 (luma 6, 7) have one luma row inside; columns 1 (luma 2, 3) and 3 (luma 6, 7) one
    # luma column, column 2 (luma 4, 5) both
    want_k = {(2, 1): 64, (2, 2): 128, (2, 3): 64, (3, 1): 64, (3, 2): 128, (3, 3): 64}
    for (v, _, ci), (v0, _, _) in zip(ch[1:], ch0[1:]):
        c = (cu, cv)[ci - 1]
        for y in range(h // 2):
            for x in range(w // 2):
                k = want_k.get((y, x), 0)
                ae = (k * 255 + 127) // 255
                assert ae == k
                assert v[y, x] == (int(v0[y, x]) * (255 - ae) + c * ae + 127) // 255, (y, x)
    # three of four: the stamp covers the block of chroma (2, 2) = luma [4, 6) x [4, 6) but for a hole at its origin
    atlas[0, 0] = 0
    before, after, _ = one(fmt, w, h, [(0, 4, 4, 2, 2, sm.STAMP, 0, colour)], atlas)
    for (v, _, ci), (v0, _, _) in zip(am.channels(fmt, after, w, h)[1:], am.channels(fmt, before, w, h)[1:]):
        c = (cu, cv)[ci - 1]
        assert (3 * 255 + 2) >> 2 == 191
        assert v[2, 2] == (int(v0[2, 2]) * (255 - 191) + c * 191 + 127) // 255
        v0 = v0.copy()
        v0[2, 2] = v[2, 2]
        assert np.array_equal(v, v0)


def test_a_stamp_at_odd_x_does_not_grow_a_column():
    atlas = np.full((4, 4), 255, np.uint8)
    before, after, _ = one("NV12", 16, 8, [(0, 5, 1, 3, 3, sm.STAMP, 0, am.pack_colour(1, 2, 3))], atlas)
    y0, y1 = before[:16 * 8].reshape(8, 16), after[:16 * 8].reshape(8, 16)
    changed = np.argwhere(y0 != y1)
    assert changed[:, 1].min() >= 5 and changed[:, 1].max() <= 7 and changed[:, 0].min() >= 1 and changed[:, 0].max() <= 3


@pytest.mark.parametrize("fmt", am.FORMATS)
def test_overlapping_rows_depend_on_the_order(fmt):
    atlas = noise_atlas(16, 16) | 0x80
    s = (0, 2, 2, 10, 8, sm.STAMP, sm.pack_uv(1, 3), am.pack_colour(255, 0, 0, 200))
    f = (0, 4, 4, 12, 8, am.FILL, 0, am.pack_colour(0, 0, 255, 120))
    _, sf, d1 = one(fmt, 24, 16, [s, f], atlas)
    _, fs, d2 = one(fmt, 24, 16, [f, s], atlas)
    assert d1 == d2 == [0, 1] and not np.array_equal(sf, fs)
    _, first, _ = one(fmt, 24, 16, [s], atlas)
    sm.apply([first], fmt, [(24, 16)], [f], ROWS, atlas)
    assert np.array_equal(first, sf)


def test_skipped_rows_in_the_model():
    atlas = np.full((6, 9), 255, np.uint8)
    c = am.pack_colour(1, 1, 1)
    rows = [(0, 0, 0, 4, 4, sm.STAMP, sm.pack_uv(9, 0), c), (0, 0, 0, 4, 4, sm.STAMP, sm.pack_uv(0, 6), c),
            (0, 0, 0, 0, 4, sm.STAMP, 0, c), (0, 0, 0, 4, -1, sm.STAMP, 0, c), (1, 0, 0, 4, 4, sm.STAMP, 0, c),
            (-1, 0, 0, 4, 4, sm.STAMP, 0, c), (0, 8, 0, 4, 4, sm.STAMP, 0, c), (0, -4, 0, 4, 4, sm.STAMP, 0, c),
            (0, -2**31, 0, 2**31 - 1, 4, sm.STAMP, 0, c), (0, 0, 0, 4, 4, 5, 0, c)]
    before, after, drawn = one("RGB", 8, 8, rows, atlas)
    assert drawn == [] and np.array_equal(before, after)
    # no atlas: kind 4 is unknown
    before, after, drawn = one("RGB", 8, 8, [(0, 0, 0, 4, 4, sm.STAMP, 0, c)], None)
    assert drawn == [] and np.array_equal(before, after)
    # x = -2**31 + 3 with w = 2**31 - 1 reaches pixel 1; its coverage lies 2**31 - 3 columns into the atlas: zero
    before, after, drawn = one("RGB", 8, 8, [(0, -2**31 + 3, 0, 2**31 - 1, 4, sm.STAMP, 0, c)], atlas)
    assert drawn == [0] and np.array_equal(before, after)


# ---- pack_uv --------------------------------------------------------------------------------------------------------------
def test_pack_uv(vali):
    assert vali.MARK_STAMP == 4 == sm.STAMP
    assert vali.pack_uv(0, 0) == 0 and vali.pack_uv(5, 0) == 5 and vali.pack_uv(0, 1) == 65536
    assert vali.pack_uv(65535, 65535) == -1 and vali.pack_uv(0, 32768) == -(1 << 31)
    for u, v in ((0, 0), (1, 2), (65535, 0), (0, 65535), (65535, 65535), (1234, 40000)):
        a = vali.pack_uv(u, v)
        assert -(1 << 31) <= a < (1 << 31) and int(np.int32(a)) == a and a == sm.pack_uv(u, v)
        assert sm.unpack_uv(a) == (u, v)
    for bad in ((-1, 0), (0, -1), (65536, 0), (0, 65536)):
        with pytest.raises(ValueError, match="0..65535"):
            vali.pack_uv(*bad)
    with pytest.raises(TypeError):
        vali.pack_uv(1.5, 0)


# ---- the host-marks checker -------------------------------------------------------------------------------------------------
class _FakeAtlas:
    """what RunBatchAsync reads of an atlas Surface before it touches a device"""

    def __init__(self, fmt, w, h, empty=False, device=0):
        self.Format, self.Width, self.Height, self.IsEmpty, self.DeviceId = fmt, w, h, empty, device

    def desc(self):
        raise AssertionError("the marks are judged before the descriptor is needed")


def _task(vali):
    ann = object.__new__(vali.PySurfaceAnnotator)
    ann._gpu_id, ann._stream = 0, 0
    return ann


def _batch(vali, fmt, sizes):
    ab = object.__new__(vali.AnnotateBatch)
    ab.gpu_id, ab.n, ab.format, ab.sizes, ab.d_marks, ab._marks_keep = 0, len(sizes), fmt, list(sizes), 0, None
    return ab


def test_host_stamp_rows_are_checked_when_there_is_an_atlas(vali):
    from vali_amd import tasks

    sizes = [(64, 48), (32, 32)]
    c = vali.pack_colour(1, 2, 3)
    good = (0, 1, 1, 10, 10, vali.MARK_STAMP, vali.pack_uv(3, 4), c)
    assert tasks._host_marks([good], sizes, False, (97, 45)) == [good]
    for row, what in (((0, 1, 1, 10, 10, vali.MARK_STAMP, vali.pack_uv(97, 0), c), "row 1: the stamp's origin \\(97, 0\\) is outside the atlas \\(97x45\\)"),
                      ((0, 1, 1, 10, 10, vali.MARK_STAMP, vali.pack_uv(0, 45), c), "row 1: the stamp's origin \\(0, 45\\) is outside the atlas"),
                      ((0, 1, 1, 0, 10, vali.MARK_STAMP, 0, c), "row 1: the rectangle is 0x10"),
                      ((0, 1, 1, 10, -1, vali.MARK_STAMP, 0, c), "row 1: the rectangle is 10x-1"),
                      ((2, 1, 1, 10, 10, vali.MARK_STAMP, 0, c), "row 1: frame 2 is outside 0..1"),
                      ((0, 64, 1, 10, 10, vali.MARK_STAMP, 0, c), "row 1: the rectangle .* does not meet frame 0 \\(64x48\\)"),
                      ((1, 3, -10, 10, 10, vali.MARK_STAMP, 0, c), "row 1: the rectangle .* does not meet frame 1")):
        for is420 in (False, True):
            with pytest.raises(ValueError, match=what):
                tasks._host_marks([good, row], sizes, is420, (97, 45))
        # without an atlas the row passes as any unknown kind does
        assert tasks._host_marks([good, row], sizes, False) == [good, row]
    # a stamp is not snapped: on a 4:2:0 frame one that ends at pixel 0 misses, one that covers pixel 0 meets
    with pytest.raises(ValueError, match="does not meet"):
        tasks._host_marks([(0, -3, 0, 3, 4, vali.MARK_STAMP, 0, c)], sizes, True, (97, 45))
    assert len(tasks._host_marks([(0, -3, 0, 4, 4, vali.MARK_STAMP, 0, c)], sizes, True, (97, 45))) == 1


def test_run_refuses_a_bad_atlas_and_checks_stamp_rows(vali):
    ann = _task(vali)
    ab = _batch(vali, vali.RGB, [(64, 48)])
    c = vali.pack_colour(1, 2, 3)
    rows = [(0, 1, 1, 10, 10, vali.MARK_STAMP, 0, c)]
    for atlas, what in ((_FakeAtlas(vali.RGB, 8, 8), "atlas: the surface has format .*RGB.*format Y"),
                        (_FakeAtlas(vali.NV12, 8, 8), "atlas: the surface has format .*NV12"),
                        (_FakeAtlas(vali.Y, 0, 0, empty=True), "atlas: the surface is empty"),
                        (_FakeAtlas(vali.Y, 8, 8, device=1), "atlas: the surface is on device 1, the task on 0"),
                        (np.zeros((4, 4), np.uint8), "atlas: need a Surface of format Y, got ndarray")):
        with pytest.raises(ValueError, match=what):
            ann.RunBatchAsync(ab, rows, atlas=atlas)
        with pytest.raises(ValueError, match=what):
            ann.RunBatch(ab, rows, None, atlas)
    with pytest.raises(ValueError, match="row 0: the stamp's origin \\(8, 0\\) is outside the atlas \\(8x8\\)"):
        ann.RunBatchAsync(ab, [(0, 1, 1, 10, 10, vali.MARK_STAMP, vali.pack_uv(8, 0), c)], atlas=_FakeAtlas(vali.Y, 8, 8))
    # no rows: success before any device part of the batch or the atlas is needed
    assert ann.RunBatchAsync(ab, [], atlas=_FakeAtlas(vali.Y, 8, 8)) == (True, vali.TaskExecInfo.SUCCESS)


def test_public_names(vali):
    import python_vali

    for name in ("MARK_STAMP", "pack_uv", "render_labels", "LabelAtlas"):
        assert getattr(python_vali, name) is getattr(vali, name), name


# ---- render_labels ------------------------------------------------------------------------------------------------------------
LABELS = ["person", "bicycle 0.93", "Q", "traffic light", "i"]


def test_render_labels_rectangles_and_coverage(vali):
    pytest.importorskip("PIL")
    atlas, rects = vali.render_labels(LABELS)
    assert atlas.dtype == np.uint8 and atlas.ndim == 2 and rects.dtype == np.int32 and rects.shape == (len(LABELS), 4)
    ah, aw = atlas.shape
    assert 1 <= aw <= 65535 and 1 <= ah <= 65535
    owner = np.zeros(atlas.shape, np.int32)
    for i, (u, v, w, h) in enumerate(rects):
        assert w >= 1 and h >= 1 and u >= 0 and v >= 0 and u + w <= aw and v + h <= ah
        owner[v:v + h, u:u + w] += 1
        strip = atlas[v:v + h, u:u + w]
        assert strip.max() > 128, LABELS[i]            # the text is there, and solid somewhere
        assert ((strip > 0) & (strip < 255)).any()        # ... and antialiased
    assert owner.max() == 1                               # disjoint
    assert list(rects[:, 1]) == sorted(rects[:, 1]) and (rects[1:, 1] == rects[:-1, 1] + rects[:-1, 3]).all()   # stacked
    assert rects[1, 2] > rects[2, 2]                      # a longer text is a wider strip
    assert (atlas[owner == 0] == 0).all()


def test_render_labels_pad_and_determinism(vali):
    pytest.importorskip("PIL")
    a0, r0 = vali.render_labels(LABELS, pad=0)
    a1, r1 = vali.render_labels(LABELS)                   # pad = 1
    a3, r3 = vali.render_labels(LABELS, pad=3)
    for p, (a, r) in ((1, (a1, r1)), (3, (a3, r3))):
        assert (r[:, 2] == r0[:, 2] + 2 * p).all() and (r[:, 3] == r0[:, 3] + 2 * p).all()
        for (u, v, w, h), (u0, v0, w0, h0) in zip(r, r0):
            strip = a[v:v + h, u:u + w]
            assert np.array_equal(strip[p:h - p, p:w - p], a0[v0:v0 + h0, u0:u0 + w0])
            border = np.ones(strip.shape, bool)
            border[p:h - p, p:w - p] = False
            assert (strip[border] == 0).all()
    again, rects = vali.render_labels(LABELS)
    assert np.array_equal(again, a1) and np.array_equal(rects, r1)
    with pytest.raises(ValueError):
        vali.render_labels(LABELS, pad=-1)
    with pytest.raises(ValueError):
        vali.render_labels([])


# ---- C ABI --------------------------------------------------------------------------------------------------------------------
class _Surface(ctypes.Structure):
    """include/vali_hip.h: vali_surface"""
    _fields_ = [("plane", ctypes.c_void_p * 3), ("pitch", ctypes.c_int32 * 3), ("width", ctypes.c_int32),
                ("height", ctypes.c_int32), ("format", ctypes.c_int32)]


def test_library_refuses_a_bad_atlas_without_a_gpu(vali):
    """Every refusal is decided before any HIP call: the pointers below are dummies that are never read on a device."""
    lib = ctypes.CDLL(str(ROOT / "vali_amd" / "libvali_hip.so"))
    assert hasattr(lib, "vali_annotate_batch_atlas")
    lib.vali_last_error.restype = ctypes.c_char_p
    lib.vali_annotate_batch_atlas.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                              ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_size_t, ctypes.c_void_p]
    lib.vali_annotate_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                        ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    buf = ctypes.create_string_buffer(256)
    base = (ctypes.addressof(buf) + 15) & ~15
    params = (ctypes.c_float * 20)()
    sizes = [(64, 48), (2, 2)]

    def frames(fmt):
        arr = (_Surface * len(sizes))()
        for s, (w, h) in zip(arr, sizes):
            for p in range(3):
                s.plane[p], s.pitch[p] = base, 3 * w
            s.width, s.height, s.format = w, h, int(getattr(vali, fmt))
        return arr

    def atlas(**kw):
        a = _Surface()
        a.plane[0], a.pitch[0], a.width, a.height, a.format = base, 97, 97, 45, int(vali.Y)
        for k, v in kw.items():
            if k == "plane":
                a.plane[0] = v
            elif k == "pitch":
                a.pitch[0] = v
            else:
                setattr(a, k, v)
        return a

    def run(arr, fmt, at, m=4, marks=base, ws_bytes=1 << 30, n=2):
        return lib.vali_annotate_batch_atlas(arr, base, n, int(getattr(vali, fmt)), marks, m, ctypes.byref(at) if at else None,
                                             params, base, ws_bytes, None)

    for fmt in ("NV12", "RGB"):
        good = frames(fmt)
        for kw, what in ((dict(format=int(vali.NV12)), b"VALI_FMT_Y"), (dict(format=int(vali.RGB)), b"VALI_FMT_Y"),
                         (dict(format=0), b"VALI_FMT_Y"), (dict(plane=None), b"null plane"),
                         (dict(width=0), b"1..65535"), (dict(height=0), b"1..65535"), (dict(width=65536, pitch=65536), b"1..65535"),
                         (dict(height=65536), b"1..65535"), (dict(width=-3), b"1..65535"), (dict(pitch=96), b"pitch"),
                         (dict(pitch=0), b"pitch")):
            assert run(good, fmt, atlas(**kw)) == -1, kw
            err = lib.vali_last_error()
            assert b"vali_annotate_batch_atlas" in err and what in err and b"atlas" in err, (kw, err)
            assert run(good, fmt, atlas(**kw), m=0) == -1, kw               # ... also when there is nothing to draw
        # the largest atlas, and one whose rows are exactly a pitch long, pass the checks (m = 0: nothing is launched)
        assert run(good, fmt, atlas(width=65535, height=65535, pitch=65535), m=0) == 0
        assert run(good, fmt, atlas(width=1, height=1, pitch=1), m=0) == 0
        # the other refusals of vali_annotate_batch hold with an atlas
        assert run(good, fmt, atlas(), m=4097) == -1 and b"4096" in lib.vali_last_error()
        assert run(good, fmt, atlas(), ws_bytes=8) == -1 and b"workspace" in lib.vali_last_error()
        assert run(good, fmt, atlas(), marks=None) == -1
        # a NULL atlas: what vali_annotate_batch accepts and refuses
        for kw in (dict(m=0), dict(m=0, marks=None), dict(m=4097), dict(ws_bytes=8), dict(marks=None), dict(n=-1)):
            a = run(good, fmt, None, **kw)
            b = lib.vali_annotate_batch(good, base, kw.get("n", 2), int(getattr(vali, fmt)), kw.get("marks", base), kw.get("m", 4),
                                        params, base, kw.get("ws_bytes", 1 << 30), None)
            assert a == b and a == (0 if kw.get("m") == 0 else -1), kw
    assert run(None, "RGB", None, m=0, n=0) == 0
