"""PyInstanceMasker: a segmentation head's prototypes and coefficients -> instance masks blended onto frames, on the GPU
(vali_mask_paint).

The mask of a detection is coeffs[k] . protos, upsampled bilinearly to the frame and thresholded at 0; the masks of the
selector's detections are blended in place, in row order, in two launches whatever the data: no box, no class id and no
mask is ever on the host.  The definition, sample for sample, is in include/vali_hip.h; tests/mask_model.py restates it
in numpy.
"""
from __future__ import annotations

from typing import Sequence, Tuple

from ._batch import PAINT_FORMATS, PreparedBatch, frames_of_one_format
from ._native import shim
from ._runargs import alpha_arg, batch_size, host_colours, max_det_arg, net_size_arg, run_colours, run_rects
from .enums import TaskExecInfo
from .surface import Surface
from .tasks import _UNSUPP_CC_PAIR, _SurfaceTask, _rgb2yuv_params, _status
from .tensors import HEAD_CAI, device_float, device_i32, strided_layout

MAX_PROTOS, MAX_SIDE, MAX_HEAD, MAX_DET = 64, 1024, 1 << 20, 1024


def protos_layout(shape, strides, code, bits):
    """The rules for `protos`, without a device: (N, M, Hp, Wp) with an x stride of 1.  Returns (dtype code, shape,
    strides); ValueError, naming what is wrong, otherwise."""
    code, shape, strides = strided_layout("protos", ("N", "M", "Hp", "Wp"), shape, strides, code, bits)
    n, m, hp, wp = shape
    batch_size(n, "protos")
    if not 1 <= m <= MAX_PROTOS:
        raise ValueError(f"protos: M = {m} is outside 1..{MAX_PROTOS}")
    if not (1 <= hp <= MAX_SIDE and 1 <= wp <= MAX_SIDE):
        raise ValueError(f"protos: Hp x Wp = {hp} x {wp} is outside 1..{MAX_SIDE}")
    if wp > 1 and strides[3] != 1:
        raise ValueError(f"protos: the x stride must be 1, got {strides[3]}")
    return code, shape, strides


def coeffs_layout(shape, strides, code, bits):
    """The rules for `coeffs`, without a device: (N, K, M) with any element strides >= 0"""
    code, shape, strides = strided_layout("coeffs", ("N", "K", "M"), shape, strides, code, bits)
    n, k, m = shape
    batch_size(n, "coeffs")
    if not 1 <= k <= MAX_HEAD:
        raise ValueError(f"coeffs: K = {k} is outside 1..2^20")
    if not 1 <= m <= MAX_PROTOS:
        raise ValueError(f"coeffs: M = {m} is outside 1..{MAX_PROTOS}")
    return code, shape, strides


def mask_spec(n_frames, protos_view, coeffs_view, max_det=100, net_size=(640, 640)):
    """What Prepare checks once the tensors are seen, without a device: views are (dtype code, shape, strides) as
    protos_layout / coeffs_layout return them.  Returns (n, m, hp, wp, k, D, net_w, net_h)."""
    (_, (n, m, hp, wp), _), (_, (n2, k, m2), _) = protos_view, coeffs_view
    if n != n2 or m != m2:
        raise ValueError(f"protos and coeffs disagree: protos are ({n}, {m}, {hp}, {wp}), coeffs ({n2}, {k}, {m2})")
    if n_frames != n:
        raise ValueError(f"frames: {n_frames} surfaces for tensors of N = {n}")
    D = max_det_arg(max_det, n, MAX_DET)
    return (n, m, hp, wp, k, D) + net_size_arg(net_size)


def paint_spec(colours, alpha):
    """What Run checks of its host arguments: (host colours or None for a device tensor, alpha as the C ABI takes it)"""
    a = alpha_arg(alpha)
    return host_colours("colours", colours), a


class MaskBatch(PreparedBatch):
    """What PyInstanceMasker.Run works on: the frames, the head's two tensors, the selector's dets and the workspace,
    checked and set up once (PyInstanceMasker.Prepare).  Keeps the surfaces and tensors alive."""

    _owned = ("d_frames", "d_ws", "d_rects", "d_colours")

    def __init__(self, gpu_id: int, stream: int, frames: Sequence[Surface], protos, coeffs, dets, max_det=100,
                 net_size=(640, 640)):
        frames = list(frames)
        fmt = frames_of_one_format("MaskBatch", frames, PAINT_FORMATS, gpu_id)
        pseen, (pcode, pshape, pstr) = device_float("protos", protos, protos_layout, gpu_id, *HEAD_CAI)
        cseen, (ccode, cshape, cstr) = device_float("coeffs", coeffs, coeffs_layout, gpu_id, *HEAD_CAI)
        n, m, hp, wp, k, D, net_w, net_h = mask_spec(len(frames), (pcode, pshape, pstr), (ccode, cshape, cstr), max_det,
                                                     net_size)
        if dets is None:
            raise ValueError(f"dets: an int32 ({n * D}, 8) device tensor is required")
        self.d_dets, _, dh = device_i32("dets", dets, (n * D, 8), gpu_id)
        self._begin(gpu_id, stream, "Prepare()", frames, rects=n, colours=True)
        self.n, self.m, self.hp, self.wp, self.k, self.D = n, m, hp, wp, k, D
        self.net_w, self.net_h = net_w, net_h
        self.format = fmt
        self.protos = (pseen.ptr, pcode, pstr[0], pstr[1], pstr[2])
        self.coeffs = (cseen.ptr, ccode, *cstr)
        self._keep = [frames, pseen.holder, cseen.holder, dh]
        self.ws_bytes = shim.mask_workspace_size(n, D, hp, wp)
        self.d_ws = shim.mem_alloc(gpu_id, self.ws_bytes)


class PyInstanceMasker(_SurfaceTask):
    """The instance masks of a segmentation network (YOLOv8-seg, YOLACT and their descendants) blended IN PLACE onto a
    batch of NV12, YUV420, YUV444, RGB, BGR or RGB_PLANAR frames of any sizes, in two launches whatever the data, with
    nothing allocated and no synchronisation, so the call can be captured and replayed after its tensors and frames were
    rewritten in place (vali_mask_paint).

    mb = Prepare(frames, protos, coeffs, dets, max_det=100, net_size=(640, 640)): `protos` (N, M, Hp, Wp) and `coeffs`
    (N, K, M) are float32, float16 or bfloat16 GPU tensors (`__dlpack__`, or `__cuda_array_interface__` for float32 and
    float16); protos has an x stride of 1 and any n, m, y strides >= 0 (a (1, M, Hp, Wp) tensor expanded over N), coeffs
    any element strides >= 0 -- a YOLOv8-seg head (N, 4 + C + M, K) goes in as pred[:, 4 + C:].transpose(1, 2), without a
    copy.  `dets` is PyDetectionSelector's (N * max_det, 8) int32 tensor, read on the device only: row i * max_det + r
    belongs to frame i and its `k` picks the coefficients.  N 1..1024, M 1..64, Hp and Wp 1..1024, K 1..2^20, max_det
    1..1024, N * max_det <= 65535, net_size (the network input's width and height) 1..65535.

    Run(mb, rects, colours, alpha=128, cc_ctx=None): `rects` is the (N, 8) int32 record array the frames were placed with,
    handled as PyDetectionSelector.Run handles it; `colours` packed colours (pack_colour) as a host sequence, uploaded
    when it changes, or an int32 device tensor: a detection is painted in colours[class % len(colours)] at `alpha`
    (None: the colour's own).  `cc_ctx` picks the RGB -> YUV matrix as PySurfaceAnnotator.RunBatch does.  The mask of a
    detection exists inside its box only; masks are applied in row order.
    """

    def Prepare(self, frames: Sequence[Surface], protos, coeffs, dets, max_det=100, net_size=(640, 640)) -> MaskBatch:
        return MaskBatch(self._gpu_id, self._stream, frames, protos, coeffs, dets, max_det, net_size)

    def RunAsync(self, mb: MaskBatch, rects, colours, alpha=128, cc_ctx=None) -> Tuple[bool, TaskExecInfo]:
        if not isinstance(mb, MaskBatch):
            raise ValueError("Run: pass a MaskBatch (Prepare)")
        host, a = paint_spec(colours, alpha)
        supported, params = _rgb2yuv_params(mb.format, cc_ctx)
        if not supported:
            return _UNSUPP_CC_PAIR
        dc, nc = run_colours("PyInstanceMasker", mb, "colours", colours, host, self._gpu_id, self._stream)
        d_rects = run_rects(mb, rects, self._gpu_id, self._stream)
        d = _status(shim.mask_paint(mb.descs, mb.d_frames, int(mb.format), mb.protos, mb.coeffs, mb.m, mb.hp, mb.wp, mb.k,
                                    mb.D, mb.net_w, mb.net_h, mb.d_dets, d_rects, dc, nc, a, params, mb.d_ws, mb.ws_bytes,
                                    self._stream))
        return d.success, d.info

    def Run(self, mb: MaskBatch, rects, colours, alpha=128, cc_ctx=None) -> Tuple[bool, TaskExecInfo]:
        r = self.RunAsync(mb, rects, colours, alpha, cc_ctx)
        self._sync()
        return r
