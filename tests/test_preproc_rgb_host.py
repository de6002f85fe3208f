"""RGB, BGR and RGB_PLANAR sources of the fused preprocessor, host side (no GPU): RoiBatch's checks as a pure
function, the relaxed rectangle rule, SupportedFormats, and the C declarations / argument checks of
vali_rgb_preproc_roi[_batch]."""
import ctypes
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


class _FakeSurface:
    """what the host checks read of a Surface before a device is touched"""

    def __init__(self, fmt, w, h):
        self.Format, self.Width, self.Height, self.IsEmpty = fmt, w, h, False


@pytest.mark.parametrize("fmt", ["RGB", "BGR", "RGB_PLANAR"])
def test_roi_batch_records_accept_odd_rgb_geometry(vali, fmt):
    from vali_amd import tasks

    f = getattr(vali, fmt)
    srcs = [_FakeSurface(f, 63, 47), _FakeSurface(f, 1, 1)]
    dsts = [_FakeSurface(vali.RGB_32F_PLANAR, 299, 299) for _ in srcs]
    got = tasks._roi_batch_records(srcs, dsts, [(1, 3, 5, 7), None], [(7, 9, 201, 1), None])
    assert got == (f, [(1, 3, 5, 7, 7, 9, 201, 1), (0, 0, 1, 1, 0, 0, 299, 299)])
    # the last pixel of the source, alone
    assert tasks._roi_batch_records(srcs[:1], dsts[:1], [(62, 46, 1, 1)])[1] == [(62, 46, 1, 1, 0, 0, 299, 299)]


def test_roi_batch_records_refuse_malformed_rgb_input(vali):
    from vali_amd import tasks

    rgb = [_FakeSurface(vali.RGB, 63, 47), _FakeSurface(vali.RGB, 63, 47)]
    dst = [_FakeSurface(vali.RGB_32F_PLANAR, 299, 299) for _ in range(2)]
    with pytest.raises(ValueError, match="one format"):        # mixed source formats
        tasks._roi_batch_records([rgb[0], _FakeSurface(vali.NV12, 64, 48)], dst)
    with pytest.raises(ValueError, match="one format"):
        tasks._roi_batch_records([rgb[0], _FakeSurface(vali.BGR, 63, 47)], dst)
    with pytest.raises(ValueError):                            # crop past the edge
        tasks._roi_batch_records(rgb, dst, [(1, 3, 5, 7), (60, 0, 4, 4)])
    with pytest.raises(ValueError):
        tasks._roi_batch_records(rgb, dst, [(1, 3, 5, 7), (0, 41, 4, 7)])
    with pytest.raises(ValueError):                            # 0-wide / 0-high rectangles
        tasks._roi_batch_records(rgb, dst, [(1, 3, 0, 7), None])
    with pytest.raises(ValueError):
        tasks._roi_batch_records(rgb, dst, None, [None, (0, 0, 5, 0)])
    with pytest.raises(ValueError):                            # negative origin
        tasks._roi_batch_records(rgb, dst, [(-1, 0, 4, 4), None])
    with pytest.raises(ValueError):                            # placement outside the canvas
        tasks._roi_batch_records(rgb, dst, None, [None, (1, 0, 299, 299)])
    with pytest.raises(ValueError):                            # destinations of two sizes
        tasks._roi_batch_records(rgb, [dst[0], _FakeSurface(vali.RGB_32F_PLANAR, 299, 298)])
    with pytest.raises(ValueError):                            # list lengths
        tasks._roi_batch_records(rgb, dst[:1])
    with pytest.raises(ValueError):
        tasks._roi_batch_records([], [])


def test_roi_batch_records_keep_the_nv12_rules(vali):
    from vali_amd import tasks

    nv = [_FakeSurface(vali.NV12, 64, 48), _FakeSurface(vali.NV12, 128, 96)]
    dst = [_FakeSurface(vali.RGB_32F_PLANAR, 32, 32) for _ in range(2)]
    assert tasks._roi_batch_records(nv, dst, [(2, 4, 6, 8), None]) == (
        vali.NV12, [(2, 4, 6, 8, 0, 0, 32, 32), (0, 0, 128, 96, 0, 0, 32, 32)])
    with pytest.raises(ValueError):        # odd crop
        tasks._roi_batch_records(nv, dst, [(1, 3, 5, 7), None])
    with pytest.raises(ValueError):        # 1 x 1 is too small for 4:2:0
        tasks._roi_batch_records(nv, dst, [(0, 0, 1, 1), None])
    with pytest.raises(ValueError):        # odd source size
        tasks._roi_batch_records([_FakeSurface(vali.NV12, 63, 48)], dst[:1])
    with pytest.raises(ValueError):        # odd destination size
        tasks._roi_batch_records(nv[:1], [_FakeSurface(vali.RGB_32F_PLANAR, 299, 299)])
    with pytest.raises(ValueError):        # odd placement
        tasks._roi_batch_records(nv, dst, None, [(1, 0, 4, 4), None])


def test_roi_batch_calls_the_host_checks_before_a_device(vali):
    from vali_amd.tasks import RoiBatch

    dst = [_FakeSurface(vali.RGB_32F_PLANAR, 299, 299) for _ in range(2)]
    with pytest.raises(ValueError, match="one format"):
        RoiBatch(0, 0, [_FakeSurface(vali.RGB, 63, 47), _FakeSurface(vali.NV12, 64, 48)], dst)
    with pytest.raises(ValueError):
        RoiBatch(0, 0, [_FakeSurface(vali.RGB, 63, 47)], dst[:1], [(60, 0, 4, 4)])


def test_rect_keeps_its_three_argument_rule_and_relaxes_on_request():
    from vali_amd import tasks

    with pytest.raises(ValueError):
        tasks._rect((1, 3, 5, 7), (63, 47), "r")
    assert tasks._rect((1, 3, 5, 7), (63, 47), "r", even=False) == (1, 3, 5, 7)
    assert tasks._rect(None, (63, 47), "r", even=False) == (0, 0, 63, 47)
    for bad in ((0, 0, 0, 1), (0, 0, 64, 1), (-1, 0, 1, 1), (0, 47, 1, 1), (0, 0, 1.0, 1)):
        with pytest.raises(ValueError):
            tasks._rect(bad, (63, 47), "r", even=False)


def test_supported_formats(vali):
    import python_vali

    pairs = vali.PySurfacePreprocessor.SupportedFormats()
    srcs = (vali.NV12, vali.RGB, vali.BGR, vali.RGB_PLANAR)
    dsts = (vali.RGB_32F_PLANAR, vali.RGB_32F, vali.RGB, vali.BGR, vali.RGB_PLANAR)
    assert sorted((int(s), int(d)) for s, d in pairs) == sorted((int(s), int(d)) for s in srcs for d in dsts)
    assert python_vali.PySurfacePreprocessor.SupportedFormats() == pairs


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_header_declares_rgb_entry_points(tmp_path):
    tu = tmp_path / "tu.c"
    tu.write_text(
        '#include "vali_hip.h"\n'
        "int main(void) {\n"
        "  int (*single)(const vali_surface*, const vali_surface*, const vali_roi*, const vali_preproc_params*, int,\n"
        "                const uint8_t*, vali_stream_t) = vali_rgb_preproc_roi;\n"
        "  int (*batch)(const vali_surface*, const vali_surface*, const vali_roi*, int, int, int, int, int,\n"
        "               const vali_preproc_params*, int, const uint8_t*, vali_stream_t) = vali_rgb_preproc_roi_batch;\n"
        "  (void)single; (void)batch;\n"
        "  return 0;\n"
        "}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", "-c",
                    str(tu), "-o", str(tmp_path / "tu.o")], check=True)


class _Surface(ctypes.Structure):
    """include/vali_hip.h: vali_surface"""
    _fields_ = [("plane", ctypes.c_void_p * 3), ("pitch", ctypes.c_int32 * 3), ("width", ctypes.c_int32),
                ("height", ctypes.c_int32), ("format", ctypes.c_int32)]


def test_library_checks_rgb_arguments_without_a_gpu(vali):
    """Null arguments, formats and host rectangles are judged before any HIP call."""
    lib = ctypes.CDLL(str(ROOT / "vali_amd" / "libvali_hip.so"))
    lib.vali_last_error.restype = ctypes.c_char_p
    assert lib.vali_rgb_preproc_roi(None, None, None, None, 0, None, None) == -1
    assert b"null" in lib.vali_last_error()
    assert lib.vali_rgb_preproc_roi_batch(None, None, None, 0, int(vali.RGB), 64, 64, int(vali.RGB_32F), None, 0,
                                          None, None) == -1
    assert ctypes.sizeof(_Surface) == 48
    params = (ctypes.c_float * 16)()
    buf = ctypes.create_string_buffer(64)       # never read: every call below is refused first

    def desc(fmt, w, h):
        s = _Surface()
        for c in range(3):
            s.plane[c] = ctypes.addressof(buf)
            s.pitch[c] = 1 << 12
        s.width, s.height, s.format = w, h, int(fmt)
        return s

    dst = desc(vali.RGB_32F_PLANAR, 32, 32)
    for bad in (vali.NV12, vali.YUV420, vali.Y):
        src = desc(bad, 64, 48)
        assert lib.vali_rgb_preproc_roi(ctypes.byref(src), ctypes.byref(dst), None, params, 0, None, None) == -2
    src = desc(vali.RGB, 63, 47)
    yuv = desc(vali.YUV444, 32, 32)
    assert lib.vali_rgb_preproc_roi(ctypes.byref(src), ctypes.byref(yuv), None, params, 0, None, None) == -2
    roi = (ctypes.c_int32 * 8)
    for r in ((60, 0, 4, 4, 0, 0, 32, 32), (0, 0, 0, 4, 0, 0, 32, 32), (-1, 0, 4, 4, 0, 0, 32, 32),
              (0, 0, 4, 4, 0, 30, 4, 3), (0, 0, 4, 4, 0, 0, 4, 0)):
        assert lib.vali_rgb_preproc_roi(ctypes.byref(src), ctypes.byref(dst), roi(*r), params, 0, None, None) == -1, r
    # a pad colour is needed when padding is on
    assert lib.vali_rgb_preproc_roi(ctypes.byref(src), ctypes.byref(dst), None, params, 1, None, None) == -1
    d_any = ctypes.c_void_p(ctypes.addressof(buf))
    for bad in (vali.NV12, vali.YUV420):
        assert lib.vali_rgb_preproc_roi_batch(d_any, d_any, d_any, 1, int(bad), 32, 32, int(vali.RGB_32F), params, 0,
                                              None, None) == -2
    assert lib.vali_rgb_preproc_roi_batch(d_any, d_any, d_any, 1, int(vali.RGB), 32, 32, int(vali.NV12), params, 0,
                                          None, None) == -2
    assert lib.vali_rgb_preproc_roi_batch(d_any, d_any, d_any, 1, int(vali.RGB), 0, 32, int(vali.RGB_32F), params, 0,
                                          None, None) == -1
    assert lib.vali_rgb_preproc_roi_batch(d_any, d_any, d_any, 0, int(vali.RGB), 299, 299, int(vali.RGB_32F), params,
                                          0, None, None) == 0       # n = 0: nothing to do
