"""Regions of the fused preprocessor, host side (no GPU): letterbox_rect, rectangle validation of RunRoi* /
PrepareRoiBatch, and the C declarations of vali_roi / vali_nv12_preproc_roi[_batch]."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("args, want", [
    ((1920, 1080, 640, 640), (0, 140, 640, 360)),      # landscape: bands above and below
    ((1080, 1920, 640, 640), (140, 0, 360, 640)),      # portrait: bands left and right
    ((1280, 720, 640, 360), (0, 0, 640, 360)),         # equal aspect: the whole canvas
    ((1000, 750, 416, 416), (0, 52, 416, 312)),        # 312 exactly; centred at an even row
    ((640, 480, 300, 300), (0, 38, 300, 224)),         # 225 rounds to the even 224 (2 * round(112.5) = 224)
    ((100, 50, 640, 640), (0, 160, 640, 320)),         # a source smaller than the canvas grows
    ((1920, 1080, 224, 224), (0, 48, 224, 126)),       # 126 = 2 * round(63.0)
])
def test_letterbox_rect(vali, args, want):
    assert vali.letterbox_rect(*args) == want
    x, y, w, h = want
    assert (x | y | w | h) & 1 == 0


def test_letterbox_rect_is_exported_by_both_names(vali):
    import python_vali

    assert python_vali.letterbox_rect is vali.letterbox_rect
    assert python_vali.RoiBatch is vali.RoiBatch
    with pytest.raises(ValueError):
        vali.letterbox_rect(0, 10, 10, 10)


@pytest.mark.parametrize("rect, size", [
    ((1, 0, 4, 4), (64, 48)), ((0, 0, 5, 4), (64, 48)),        # odd
    ((-2, 0, 4, 4), (64, 48)), ((0, -2, 4, 4), (64, 48)),      # negative
    ((62, 0, 4, 4), (64, 48)), ((0, 46, 4, 4), (64, 48)),      # past the edge
    ((0, 0, 0, 4), (64, 48)), ((0, 0, 4, 0), (64, 48)),        # empty
    ((0, 0, 64), (64, 48)), ((0, 0, 4.0, 4), (64, 48)),        # not four integers
])
def test_rect_validation(rect, size):
    from vali_amd import tasks

    with pytest.raises(ValueError):
        tasks._rect(rect, size, "r")


def test_valid_rects_and_pad_pass_unchanged():
    from vali_amd import tasks

    assert tasks._rect(None, (64, 48), "r") == (0, 0, 64, 48)
    assert tasks._rect((62, 46, 2, 2), (64, 48), "r") == (62, 46, 2, 2)
    assert tasks._roi_record((2, 4, 6, 8), None, (64, 48), (10, 12)) == (2, 4, 6, 8, 0, 0, 10, 12)
    assert tasks._pad_colour(None) == (False, (0, 0, 0))
    assert tasks._pad_colour((114, 114, 114)) == (True, (114, 114, 114))
    for bad in ((1, 2), (0, 0, 256), (-1, 0, 0), "abc", (1.5, 0, 0)):
        with pytest.raises(ValueError):
            tasks._pad_colour(bad)


class _FakeSurface:
    """what RoiBatch reads of a Surface before it touches a device"""

    def __init__(self, fmt, w, h):
        self.Format, self.Width, self.Height, self.IsEmpty = fmt, w, h, False


def test_prepare_roi_batch_refuses_malformed_input(vali):
    from vali_amd.tasks import RoiBatch

    nv = [_FakeSurface(vali.NV12, 64, 48), _FakeSurface(vali.NV12, 128, 96)]
    dst = [_FakeSurface(vali.RGB_32F_PLANAR, 32, 32) for _ in range(2)]
    with pytest.raises(ValueError):        # list lengths
        RoiBatch(0, 0, nv, dst[:1])
    with pytest.raises(ValueError):
        RoiBatch(0, 0, nv, dst, [None])
    with pytest.raises(ValueError):
        RoiBatch(0, 0, nv, dst, None, [None, None, None])
    with pytest.raises(ValueError):        # empty
        RoiBatch(0, 0, [], [])
    with pytest.raises(ValueError):        # mixed destination sizes
        RoiBatch(0, 0, nv, [dst[0], _FakeSurface(vali.RGB_32F_PLANAR, 32, 34)])
    with pytest.raises(ValueError):        # mixed destination formats
        RoiBatch(0, 0, nv, [dst[0], _FakeSurface(vali.RGB_32F, 32, 32)])
    with pytest.raises(ValueError):        # crop past the second (larger) source is fine, past the first is not
        RoiBatch(0, 0, nv, dst, [(0, 0, 128, 96), (0, 0, 128, 96)])
    with pytest.raises(ValueError):        # odd crop
        RoiBatch(0, 0, nv, dst, [(0, 0, 10, 10), (0, 1, 10, 10)])
    with pytest.raises(ValueError):        # placement outside the canvas
        RoiBatch(0, 0, nv, dst, None, [(0, 0, 32, 32), (2, 0, 32, 32)])
    with pytest.raises(ValueError):        # odd source size
        RoiBatch(0, 0, [_FakeSurface(vali.NV12, 63, 48)], dst[:1])


def test_shim_roi_record_size(vali):
    from vali_amd._native import shim

    assert shim.ROI_SIZE == 32


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_header_declares_roi_entry_points(tmp_path):
    tu = tmp_path / "tu.c"
    tu.write_text(
        '#include <stddef.h>\n#include "vali_hip.h"\n'
        "int main(void) {\n"
        "  int (*single)(const vali_surface*, const vali_surface*, const vali_roi*, const vali_preproc_params*, int,\n"
        "                const uint8_t*, vali_stream_t) = vali_nv12_preproc_roi;\n"
        "  int (*batch)(const vali_surface*, const vali_surface*, const vali_roi*, int, int, int, int,\n"
        "               const vali_preproc_params*, int, const uint8_t*, vali_stream_t) = vali_nv12_preproc_roi_batch;\n"
        "  (void)single; (void)batch;\n"
        "  return sizeof(vali_roi) == 32 && offsetof(vali_roi, dst_x) == 16 && offsetof(vali_roi, dst_h) == 28 ? 0 : 1;\n"
        "}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", "-c",
                    str(tu), "-o", str(tmp_path / "tu.o")], check=True)
    # compile-only above (no library needed); the size check itself runs as a host program
    subprocess.run(["gcc", "-std=c99", f"-I{ROOT / 'include'}", str(tu), "-o", str(tmp_path / "tu"),
                    "-Wl,--unresolved-symbols=ignore-all"], check=True)
    assert subprocess.run([str(tmp_path / "tu")]).returncode == 0


def test_library_rejects_bad_roi_arguments_without_a_gpu():
    """Strict host validation of the single form happens before any HIP call."""
    import ctypes

    lib = ctypes.CDLL(str(ROOT / "vali_amd" / "libvali_hip.so"))
    lib.vali_last_error.restype = ctypes.c_char_p
    assert lib.vali_nv12_preproc_roi(None, None, None, None, 0, None, None) == -1
    assert b"null" in lib.vali_last_error()
    assert lib.vali_nv12_preproc_roi_batch(None, None, None, 0, 64, 64, 9, None, 0, None, None) == -1
