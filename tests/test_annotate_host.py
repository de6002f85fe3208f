"""PySurfaceAnnotator / vali_annotate_batch without a GPU: the model's own properties (tests/annotate_model.py), the
colour packing, every ValueError of the Python layer and every refusal of the C ABI."""
import ctypes
import shutil
import subprocess
import types
from pathlib import Path

import numpy as np
import pytest

import annotate_model as am
import postproc_model as pm

ROOT = Path(__file__).resolve().parent.parent
ROWS = ((0.299, 0.587, 0.114, 0.0), (-0.147, -0.289, 0.436, 128.0), (0.615, -0.515, -0.100, 128.0))


def one(fmt, w, h, marks, seed=1, rows=ROWS):
    flat = am.noise_frame(fmt, w, h, seed)
    before = flat.copy()
    drawn = am.apply([flat], fmt, [(w, h)], marks, rows)
    return before, flat, drawn


# ---- the model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", am.FORMATS)
def test_alpha_0_is_the_identity_and_255_replaces(fmt):
    w, h = 20, 12
    for kind, arg in ((am.FILL, 0), (am.BOX, 2)):
        before, after, drawn = one(fmt, w, h, [(0, 2, 2, 10, 8, kind, arg, am.pack_colour(9, 200, 77, 0))])
        assert drawn == [0] and np.array_equal(before, after)
    before, after, _ = one(fmt, w, h, [(0, 2, 2, 10, 8, am.FILL, 0, am.pack_colour(9, 200, 77, 255))])
    want = am.yuv_of(9, 200, 77, ROWS) if fmt in am.YUV else (9, 200, 77)
    for (v, sh, ci), (v0, _, _) in zip(am.channels(fmt, after, w, h), am.channels(fmt, before, w, h)):
        inside = np.zeros(v.shape, bool)
        inside[2 >> sh:10 >> sh, 2 >> sh:12 >> sh] = True
        assert (v[inside] == want[ci]).all() and np.array_equal(v[~inside], v0[~inside])


def test_blend_formula_and_bgr_channel_order():
    before, after, _ = one("BGR", 4, 4, [(0, 1, 1, 2, 2, am.FILL, 0, am.pack_colour(250, 100, 10, 77))])
    b0, a0 = before.reshape(4, 4, 3), after.reshape(4, 4, 3)
    for k, c in enumerate((10, 100, 250)):                       # a BGR surface stores b first
        v = int(b0[1, 1, k])
        assert a0[1, 1, k] == (v * (255 - 77) + c * 77 + 127) // 255
    assert np.array_equal(a0[0], b0[0]) and np.array_equal(a0[3], b0[3])


def test_overlapping_translucent_fills_depend_on_the_order():
    m1 = (0, 0, 0, 8, 8, am.FILL, 0, am.pack_colour(255, 0, 0, 100))
    m2 = (0, 4, 4, 8, 8, am.FILL, 0, am.pack_colour(0, 0, 255, 180))
    _, ab, _ = one("RGB", 12, 12, [m1, m2])
    _, ba, _ = one("RGB", 12, 12, [m2, m1])
    assert not np.array_equal(ab, ba)
    # each equals the sequential definition: the second mark on the result of the first
    _, first, _ = one("RGB", 12, 12, [m1])
    am.apply([first], "RGB", [(12, 12)], [m2])
    assert np.array_equal(first, ab)
    _, first, _ = one("RGB", 12, 12, [m2])
    am.apply([first], "RGB", [(12, 12)], [m1])
    assert np.array_equal(first, ba)


@pytest.mark.parametrize("fmt", am.S420)
def test_snapping_on_420(fmt):
    w, h = 16, 12
    c = am.pack_colour(1, 2, 3)
    _, odd, _ = one(fmt, w, h, [(0, 3, 5, 4, 2, am.FILL, 0, c)])          # [3, 7) x [5, 7) -> [2, 8) x [4, 8)
    _, even, _ = one(fmt, w, h, [(0, 2, 4, 6, 4, am.FILL, 0, c)])
    assert np.array_equal(odd, even)
    # a chroma sample is painted exactly when its four luma pixels are
    before, after, _ = one(fmt, w, h, [(0, 3, 5, 4, 2, am.FILL, 0, c)])
    chans, chans0 = am.channels(fmt, after, w, h), am.channels(fmt, before, w, h)
    luma = chans[0][0] != chans0[0][0]
    painted = np.zeros((h, w), bool)
    painted[4:8, 2:8] = True
    assert not (luma & ~painted).any()
    for (v, sh, _), (v0, _, _) in zip(chans[1:], chans0[1:]):
        changed = np.argwhere(v != v0)
        assert all(painted[2 * y:2 * y + 2, 2 * x:2 * x + 2].all() for y, x in changed)
    # thickness 1 is rounded up to 2
    _, t1, _ = one(fmt, w, h, [(0, 2, 2, 10, 8, am.BOX, 1, c)])
    _, t2, _ = one(fmt, w, h, [(0, 2, 2, 10, 8, am.BOX, 2, c)])
    assert np.array_equal(t1, t2)


@pytest.mark.parametrize("fmt", am.FORMATS)
def test_a_thick_box_is_a_fill(fmt):
    c = am.pack_colour(200, 100, 50, 90)
    for rw, rh, t in ((10, 6, 3), (6, 10, 3), (10, 6, 40), (8, 8, 4)):
        _, box, _ = one(fmt, 24, 16, [(0, 4, 4, rw, rh, am.BOX, t, c)])
        _, fill, _ = one(fmt, 24, 16, [(0, 4, 4, rw, rh, am.FILL, 0, c)])
        assert np.array_equal(box, fill)
    _, box, _ = one(fmt, 24, 16, [(0, 4, 4, 10, 8, am.BOX, 2, c)])
    _, fill, _ = one(fmt, 24, 16, [(0, 4, 4, 10, 8, am.FILL, 0, c)])
    assert not np.array_equal(box, fill)


def test_a_clipped_box_keeps_only_its_inner_edges():
    w, h = 16, 16
    before, after, _ = one("RGB_PLANAR", w, h, [(0, -6, 4, 12, 30, am.BOX, 2, am.pack_colour(7, 7, 7))])
    changed = (after.reshape(3, h, w) != before.reshape(3, h, w)).any(0)
    want = np.zeros((h, w), bool)
    want[4:6, 0:6] = True          # the top edge, as far as it is inside
    want[4:, 4:6] = True           # the right edge; the left edge (x -6 .. -5) and the bottom (y 32 .. 33) are outside
    assert not (changed & ~want).any()                 # x 0 .. 3 below the top edge is the interior: as it was
    assert (after.reshape(3, h, w)[:, want] == 7).all()


def test_pixelate_is_the_rounded_mean_of_cell_and_frame():
    w, h = 22, 13                                                  # not multiples of the cell
    before, after, _ = one("YUV444", w, h, [(0, 8, 8, 8, 8, am.PIXELATE, 8, 0)])
    b, a = before.reshape(3, h, w), after.reshape(3, h, w)
    for c in range(3):
        full = b[c, 8:13, 8:16].astype(np.int64)                    # the cell at (8, 8) is cut by the bottom edge: 8 x 5
        assert (a[c, 8:13, 8:16] == (full.sum() + 20) // 40).all()
        assert np.array_equal(a[c, :8], b[c, :8]) and np.array_equal(a[c, :, :8], b[c, :, :8]) and np.array_equal(a[c, :, 16:], b[c, :, 16:])
    # a rectangle that is not aligned grows to the grid; the right-hand cells are 6 wide and use their own count
    before, after, _ = one("YUV444", w, h, [(0, 13, 1, 5, 2, am.PIXELATE, 8, 0)])
    b, a = before.reshape(3, h, w), after.reshape(3, h, w)
    assert (a[0, 0:8, 8:16] == (int(b[0, 0:8, 8:16].sum()) + 32) // 64).all()
    assert (a[0, 0:8, 16:22] == (int(b[0, 0:8, 16:22].sum()) + 24) // 48).all()
    assert np.array_equal(a[0, 8:], b[0, 8:]) and np.array_equal(a[0, :, :8], b[0, :, :8])


@pytest.mark.parametrize("fmt", am.S420)
def test_pixelate_420_uses_half_cells_for_chroma(fmt):
    w, h = 24, 16
    before, after, _ = one(fmt, w, h, [(0, 9, 1, 3, 3, am.PIXELATE, 8, 0)])      # -> the cell [8, 16) x [0, 8)
    for (v, sh, _), (v0, _, _) in zip(am.channels(fmt, after, w, h), am.channels(fmt, before, w, h)):
        s = 8 >> sh
        cell = v0[0:s, s:2 * s].astype(np.int64)
        assert (v[0:s, s:2 * s] == (cell.sum() + s * s // 2) // (s * s)).all()
        rest = np.ones(v.shape, bool)
        rest[0:s, s:2 * s] = False
        assert np.array_equal(v[rest], v0[rest])


@pytest.mark.parametrize("fmt", ["NV12", "RGB"])
def test_int32_overflow_rows(fmt):
    big = 2**31 - 1
    c = am.pack_colour(5, 6, 7)
    # x + w = 2**32 - 9: wholly to the right, skipped
    before, after, drawn = one(fmt, 16, 8, [(0, 2**31 - 8, 0, big, big, am.FILL, 0, c)])
    assert drawn == [] and np.array_equal(before, after)
    # x + w = -1: wholly to the left
    before, after, drawn = one(fmt, 16, 8, [(0, -2**31, -2**31, big, big, am.FILL, 0, c)])
    assert drawn == [] and np.array_equal(before, after)
    # from beyond the left / top to the far right / bottom: the whole frame
    _, whole, _ = one(fmt, 16, 8, [(0, 0, 0, 16, 8, am.FILL, 0, c)])
    _, huge, drawn = one(fmt, 16, 8, [(0, -5, -5, big, big, am.FILL, 0, c)])
    assert drawn == [0] and np.array_equal(huge, whole)
    # a box whose thickness overflows with x: the whole rectangle
    _, box, _ = one(fmt, 16, 8, [(0, 2, 2, big, big, am.BOX, big, c)])
    _, fill, _ = one(fmt, 16, 8, [(0, 2, 2, 14, 6, am.FILL, 0, c)])
    assert np.array_equal(box, fill)


def test_skipped_rows_in_the_model():
    c = am.pack_colour(1, 1, 1)
    rows = [(0, 0, 0, 4, 4, 0, 0, c), (0, 0, 0, 4, 4, 7, 0, c), (-1, 0, 0, 4, 4, am.FILL, 0, c), (1, 0, 0, 4, 4, am.FILL, 0, c),
            (0, 0, 0, 0, 4, am.FILL, 0, c), (0, 0, 0, 4, 0, am.FILL, 0, c), (0, 0, 0, 4, 4, am.PIXELATE, 5, c),
            (0, 0, 0, 4, 4, am.BOX, 0, c), (0, 8, 0, 4, 4, am.FILL, 0, c), (0, -4, 0, 4, 4, am.FILL, 0, c)]
    before, after, drawn = one("RGB", 8, 8, rows)
    assert drawn == [] and np.array_equal(before, after)


def test_model_colour_is_the_postprocessor_model(oracle):
    for name, rows in pm.matrices().items():
        p = pm.lattice(16, 8)
        want = pm.numpy_yuv(p, rows, "YUV444").reshape(3, 8, 16)
        for y in range(8):
            for x in range(0, 16, 5):
                r, g, b = (int(v) for v in p[y, x])
                assert am.yuv_of(r, g, b, rows) == tuple(int(want[k, y, x]) for k in range(3)), name


# ---- pack_colour ----------------------------------------------------------------------------------------------------------
def test_pack_colour(vali):
    assert vali.pack_colour(1, 2, 3, 0) == 0x010203
    assert vali.pack_colour(0x12, 0x34, 0x56, 0x7F) == 0x7F123456
    assert vali.pack_colour(0x12, 0x34, 0x56, 0x80) == 0x80123456 - (1 << 32)
    assert vali.pack_colour(255, 255, 255) == -1                                  # a defaults to 255
    assert vali.pack_colour(0, 0, 0, 128) == -(1 << 31)
    for args in ((1, 2, 3, 4), (255, 0, 255, 200), (0, 0, 0, 255)):
        v = vali.pack_colour(*args)
        assert -(1 << 31) <= v < (1 << 31) and v == am.pack_colour(*args)
        assert am.unpack_colour(v) == args
        assert int(np.int32(v)) == v
    for bad in ((256, 0, 0), (0, -1, 0), (0, 0, 0, 256)):
        with pytest.raises(ValueError):
            vali.pack_colour(*bad)
    assert (vali.MARK_NONE, vali.MARK_BOX, vali.MARK_FILL, vali.MARK_PIXELATE) == (0, 1, 2, 3)


# ---- Python refusals ------------------------------------------------------------------------------------------------------
class _FakeSurface:
    """what AnnotateBatch reads of a Surface before it touches a device"""

    def __init__(self, fmt, w, h, empty=False, device=0):
        self.Format, self.Width, self.Height, self.IsEmpty, self.DeviceId = fmt, w, h, empty, device


class _DeviceArray:
    """an int32 device array on GPU 0 seen through __cuda_array_interface__ (never dereferenced)"""
    device = types.SimpleNamespace(type="cuda", index=0)

    def __init__(self, shape=(4, 8), typestr="<i4", strides=None):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (4096, False), "version": 3,
                                         "strides": strides}


def _task(vali):
    ann = object.__new__(vali.PySurfaceAnnotator)
    ann._gpu_id, ann._stream = 0, 0
    return ann


def _batch(vali, fmt, sizes):
    """an AnnotateBatch without its device parts: the marks are judged before any is needed"""
    ab = object.__new__(vali.AnnotateBatch)
    ab.gpu_id, ab.n, ab.format, ab.sizes, ab.d_marks, ab._marks_keep = 0, len(sizes), fmt, list(sizes), 0, None
    return ab


def test_prepare_refuses_frames_that_do_not_fit(vali):
    ann = _task(vali)
    S = _FakeSurface
    for frames, what in (([S(vali.NV12, 10, 8), S(vali.YUV420, 10, 8)], "surface 1 has format.*one format per batch"),
                         ([S(vali.RGB, 10, 8), S(vali.BGR, 10, 8)], "one format per batch"),
                         ([S(vali.NV12, 11, 8)], "surface 0: NV12 is 4:2:0 and needs an even"),
                         ([S(vali.YUV420, 10, 8), S(vali.YUV420, 10, 7)], "surface 1: YUV420 is 4:2:0"),
                         ([S(vali.RGB, 10, 8), S(vali.RGB, 10, 8, empty=True)], "surface 1 is empty"),
                         ([None], "surface 0 is empty"),
                         ([S(vali.Y, 10, 8)], "surface 0 has format.*supported"),
                         ([S(vali.RGB_32F, 10, 8)], "supported"),
                         ([S(vali.RGB, 10, 8, device=1)], "device 1")):
        with pytest.raises(ValueError, match=what):
            ann.PrepareBatch(frames)


def test_run_refuses_bad_marks(vali):
    import torch

    ann = _task(vali)
    ab = _batch(vali, vali.RGB, [(64, 48), (32, 32)])
    with pytest.raises(ValueError, match="AnnotateBatch"):
        ann.RunBatchAsync(object(), [])
    c = vali.pack_colour(1, 2, 3)
    good = (0, 1, 1, 10, 10, vali.MARK_FILL, 0, c)
    # more than 4096
    with pytest.raises(ValueError, match="4097 rows; at most 4096"):
        ann.RunBatchAsync(ab, [good] * 4097)
    with pytest.raises(ValueError, match="4097 rows; at most 4096"):
        ann.RunBatchAsync(ab, _DeviceArray((4097, 8)))
    # a bad host row: the row and the rule
    for row, what in (((2, 1, 1, 10, 10, vali.MARK_FILL, 0, c), "row 1: frame 2 is outside 0..1"),
                      ((-1, 1, 1, 10, 10, vali.MARK_BOX, 1, c), "row 1: frame -1"),
                      ((0, 1, 1, 0, 10, vali.MARK_FILL, 0, c), "row 1: the rectangle is 0x10"),
                      ((0, 1, 1, 10, -2, vali.MARK_FILL, 0, c), "row 1: the rectangle is 10x-2"),
                      ((0, 1, 1, 10, 10, vali.MARK_BOX, 0, c), "row 1: MARK_BOX needs a thickness"),
                      ((0, 1, 1, 10, 10, vali.MARK_PIXELATE, 5, c), "row 1: MARK_PIXELATE needs a cell of 4, 8, 16 or 32, got 5"),
                      ((0, 64, 1, 10, 10, vali.MARK_FILL, 0, c), "row 1: the rectangle .* does not meet frame 0 \\(64x48\\)"),
                      ((1, 0, -10, 10, 10, vali.MARK_FILL, 0, c), "row 1: the rectangle .* does not meet frame 1"),
                      ((0, 1, 1, 10, 10, vali.MARK_FILL, 0), "row 1 has 7 values"),
                      ((0, 1, 1, 10, 10, vali.MARK_FILL, 0, 1 << 31), "row 1: every value must fit an int32"),
                      ((0, 1.5, 1, 10, 10, vali.MARK_FILL, 0, c), "row 1 must be 8 integers"),
                      (5, "row 1 must be 8 integers")):
        with pytest.raises(ValueError, match=what):
            ann.RunBatchAsync(ab, [good, row])
    # 4:2:0 frames: the meeting test is on the snapped rectangle, and it never changes the answer
    ab420 = _batch(vali, vali.NV12, [(64, 48)])
    with pytest.raises(ValueError, match="does not meet"):
        ann.RunBatchAsync(ab420, [(0, -1, 0, 1, 4, vali.MARK_FILL, 0, c)])
    # what is no int32 (M, 8) contiguous tensor of this GPU
    other = _DeviceArray()
    other.device = types.SimpleNamespace(type="cuda", index=1)
    for marks, what in ((torch.zeros((4, 8), dtype=torch.int32), "GPU"),                       # a CPU tensor
                        (_DeviceArray((4, 7)), "shape \\(M, 8\\)"),
                        (_DeviceArray((32,)), "shape \\(M, 8\\)"),
                        (_DeviceArray((4, 8, 1)), "shape \\(M, 8\\)"),
                        (_DeviceArray((4, 8), "<i8"), "int32"),
                        (_DeviceArray((4, 8), "<f4"), "int32"),
                        (_DeviceArray((4, 8), strides=(64, 4)), "contiguous"),
                        (_DeviceArray((4, 8), strides=(32, 8)), "contiguous"),
                        (torch.zeros((8, 4), dtype=torch.int32).t(), "contiguous|GPU"),
                        (other, "device 1"),
                        (object(), "sequence of 8-tuples")):
        with pytest.raises(ValueError, match=what):
            ann.RunBatchAsync(ab, marks)
    # an unsupported colour context: the postprocessor's status, nothing is launched (the batch has no device parts)
    C, S, R = vali.ColorspaceConversionContext, vali.ColorSpace, vali.ColorRange
    for cc in (C(S.BT_709, R.UDEF), C(S.UNSPEC, R.JPEG)):
        assert ann.RunBatchAsync(ab420, [(0, 1, 1, 4, 4, vali.MARK_FILL, 0, c)], cc) == \
            (False, vali.TaskExecInfo.UNSUPPORTED_FMT_CONV_PARAMS)
    # no marks, or no frames: success without a device
    assert ann.RunBatchAsync(ab, []) == (True, vali.TaskExecInfo.SUCCESS)
    assert ann.RunBatchAsync(_batch(vali, None, []), _DeviceArray((3, 8))) == (True, vali.TaskExecInfo.SUCCESS)


def test_public_surface(vali):
    import python_vali

    assert vali.PySurfaceAnnotator.SupportedFormats() == [vali.NV12, vali.YUV420, vali.YUV444, vali.RGB, vali.BGR,
                                                          vali.RGB_PLANAR]
    for name in ("PySurfaceAnnotator", "AnnotateBatch", "pack_colour", "MARK_NONE", "MARK_BOX", "MARK_FILL", "MARK_PIXELATE"):
        assert getattr(python_vali, name) is getattr(vali, name), name
    for name in ("PrepareBatch", "RunBatch", "RunBatchAsync", "SupportedFormats"):
        assert callable(getattr(python_vali.PySurfaceAnnotator, name))
    # the other tasks' tables are what they were
    assert vali.PySurfacePostprocessor.SupportedFormats() == [vali.NV12, vali.YUV420, vali.YUV444, vali.RGB, vali.RGB_PLANAR]
    assert len(vali.PySurfacePreprocessor.SupportedFormats()) == 20


# ---- C ABI ----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_header_compiles_with_gcc_and_the_mark_is_32_bytes(tmp_path):
    tu = tmp_path / "tu.c"
    tu.write_text(
        '#include <stddef.h>\n#include "vali_hip.h"\n'
        "int main(void) {\n"
        "  int (*size)(int, const vali_surface*, size_t*) = vali_annotate_workspace_size;\n"
        "  int (*run)(const vali_surface*, const vali_surface*, int, int, const vali_mark*, int, const vali_cvt_params*,\n"
        "             void*, size_t, vali_stream_t) = vali_annotate_batch;\n"
        "  vali_mark m = {0, 1, 2, 3, 4, VALI_MARK_PIXELATE, 16, 0};\n"
        "  (void)size; (void)run; (void)m;\n"
        "  return sizeof(vali_mark) == 32 && offsetof(vali_mark, colour) == 28 && VALI_MAX_MARKS == 4096 ? 0 : 1;\n"
        "}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", "-c",
                    str(tu), "-o", str(tmp_path / "tu.o")], check=True)
    lib = ROOT / "vali_amd" / "libvali_hip.so"
    subprocess.run(["gcc", str(tmp_path / "tu.o"), "-o", str(tmp_path / "tu"), f"-L{lib.parent}", "-lvali_hip",
                    f"-Wl,-rpath,{lib.parent}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], check=True)
    assert subprocess.run([str(tmp_path / "tu")]).returncode == 0


class _Surface(ctypes.Structure):
    """include/vali_hip.h: vali_surface"""
    _fields_ = [("plane", ctypes.c_void_p * 3), ("pitch", ctypes.c_int32 * 3), ("width", ctypes.c_int32),
                ("height", ctypes.c_int32), ("format", ctypes.c_int32)]


def test_library_refuses_without_a_gpu(vali):
    """Every refusal is decided before any HIP call: the pointers below are dummies that are never read on a device."""
    lib = ctypes.CDLL(str(ROOT / "vali_amd" / "libvali_hip.so"))
    lib.vali_last_error.restype = ctypes.c_char_p
    lib.vali_annotate_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                        ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vali_annotate_workspace_size.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    assert ctypes.sizeof(_Surface) == 48
    buf = ctypes.create_string_buffer(256)
    base = (ctypes.addressof(buf) + 15) & ~15
    params = (ctypes.c_float * 20)()
    fmt_of = {f: int(getattr(vali, f)) for f in am.FORMATS}

    def frames(fmt, sizes, **kw):
        arr = (_Surface * len(sizes))()
        for s, (w, h) in zip(arr, sizes):
            for p in range(3):
                s.plane[p] = base
                s.pitch[p] = 3 * w
            s.width, s.height, s.format = w, h, fmt_of[fmt]
        for k, v in kw.items():          # a fault in the LAST frame
            if k == "plane":
                arr[len(sizes) - 1].plane[v] = None
            elif k == "pitch":
                arr[len(sizes) - 1].pitch[0] = v
            else:
                setattr(arr[len(sizes) - 1], k, v)
        return arr

    def size(n, arr, out=True):
        b = ctypes.c_size_t(12345)
        rc = lib.vali_annotate_workspace_size(n, arr, ctypes.byref(b) if out else None)
        return rc, b.value

    def run(arr, n, fmt, d_frames=base, marks=base, m=4, prm=params, ws=base, ws_bytes=1 << 30):
        return lib.vali_annotate_batch(arr, d_frames, n, fmt_of.get(fmt, fmt), marks, m, prm, ws, ws_bytes, None)

    def refused(rc, code=-1, who=b"vali_annotate"):
        assert rc == code, (rc, lib.vali_last_error())
        assert len(lib.vali_last_error()) > 10 and who in lib.vali_last_error()

    two = [(64, 48), (2, 2)]
    # the workspace size, and that it is a whole number of 16 bytes per frame
    rc, per2 = size(2, frames("NV12", two))
    assert rc == 0 and per2 > 0 and per2 % 32 == 0
    assert size(0, None) == (0, 0)
    assert size(1, frames("RGB", [(1, 1)])) == (0, per2 // 2)
    # null arguments, n
    refused(size(2, frames("NV12", two), out=False)[0])
    refused(size(2, None)[0])
    refused(size(-1, frames("NV12", two))[0])
    refused(size(65536, frames("NV12", two))[0])
    good = frames("NV12", two)
    refused(run(None, 2, "NV12"))
    refused(run(good, 2, "NV12", d_frames=None))
    refused(run(good, 2, "NV12", marks=None))
    refused(run(good, 2, "NV12", ws=None))
    refused(run(good, -1, "NV12"))
    refused(run(good, 65536, "NV12"))
    for fmt in am.YUV:
        refused(run(frames(fmt, two), 2, fmt, prm=None))
        assert b"params" in lib.vali_last_error()
    # m outside 0..4096
    for m in (-1, 4097, 1 << 30):
        refused(run(good, 2, "NV12", m=m))
        assert b"4096" in lib.vali_last_error()
    # the workspace: unaligned, too small
    refused(run(good, 2, "NV12", ws=base + 8))
    assert b"aligned" in lib.vali_last_error()
    refused(run(good, 2, "NV12", ws_bytes=per2 - 1))
    assert b"workspace" in lib.vali_last_error()
    refused(run(good, 2, "NV12", marks=base + 2))
    # frames: an odd 4:2:0 size, sizes out of range, a null plane, a short pitch, another format than the batch's
    for fmt in am.S420:
        for kw in (dict(width=63), dict(height=47)):
            bad = frames(fmt, two, **kw)
            refused(run(bad, 2, fmt))
            assert b"even" in lib.vali_last_error() and b"frame 1" in lib.vali_last_error()
            refused(size(2, bad)[0])
    for kw in (dict(width=0), dict(height=0), dict(width=65536), dict(height=-4), dict(plane=0), dict(pitch=1),
               dict(format=fmt_of["YUV444"])):
        bad = frames("RGB", two, **kw)
        refused(run(bad, 2, "RGB"))
        assert b"frame 1" in lib.vali_last_error()
        refused(size(2, bad)[0])
    refused(run(frames("NV12", two, plane=1), 2, "NV12"))
    refused(run(frames("YUV420", two, plane=2), 2, "YUV420"))
    refused(run(frames("RGB", two), 2, "BGR"))                                   # the frames are not of `format`
    # formats outside the list
    for name in ("UNDEFINED", "Y", "RGB_32F", "RGB_32F_PLANAR", "YUV422", "P10", "P12", "YUV444_10bit", "YUV420_10bit",
                 "GRAY12"):
        f = int(getattr(vali, name))
        bad = frames("RGB", two)
        for s in bad:
            s.format = f
        refused(run(bad, 2, f), code=-2)
        refused(size(2, bad)[0], code=-2)
    refused(run(good, 2, 99), code=-2)
    # nothing to do: success, and nothing is launched (there is no device here to launch on)
    assert run(good, 2, "NV12", m=0) == 0
    assert run(good, 2, "NV12", m=0, marks=None) == 0
    assert run(None, 0, "RGB", d_frames=None, ws=None, ws_bytes=0, prm=None) == 0


def test_symbols_are_exported():
    lib = ctypes.CDLL(str(ROOT / "vali_amd" / "libvali_hip.so"))
    assert hasattr(lib, "vali_annotate_batch") and hasattr(lib, "vali_annotate_workspace_size")
