"""PyKeypointDecoder: the heatmaps or SimCC vectors of a second-stage (top-down) pose or landmark network -> points in
frame pixels, on the GPU (vali_kpt_decode).

The peak of every (slot, keypoint) map is found with an exact tie rule, refined by a quarter of a cell, placed on the
canvas the crops were cut to and mapped back to the frame through the very rows the crops were cut with -- PySurfaceWarper's
matrices or PyDetectionSelector's rois -- in ONE launch: no map, matrix or point is ever on the host.  The rows it writes
are the rows PyPoseDrawer.RunPoints draws.  The definition, step for step, is in include/vali_hip.h;
tests/kpt_decode_model.py restates it in numpy.
"""
from __future__ import annotations

import operator
from typing import Sequence, Tuple

from ._batch import PreparedBatch, surfaces_on_device
from ._native import shim
from ._runargs import batch_size, kpt_thr_arg, max_det_arg
from .enums import TaskExecInfo
from .pose import MAX_DET, MAX_POINTS
from .surface import Surface
from .tasks import _SurfaceTask, _status
from .tensors import HEAD_CAI, device_float, device_i32, strided_layout

MAX_SLOTS, MAX_SIDE, MAX_ELEMS, MAX_CANVAS = 65535, 4096, 1 << 20, 65535
REFINES = {"none": 0, "quarter": 1}
ALIGNS = {"centre": 0, "index": 1}


def _unit_last(who, shape, strides):
    if shape[-1] > 1 and strides[-1] != 1:
        raise ValueError(f"{who}: the last dimension must have stride 1, got strides {strides}")


def heat_layout(shape, strides, code, bits):
    """The rules for `heat`, without a device: (M, P, Hh, Wh) float32, float16 or bfloat16, x stride 1, the other element
    strides >= 0.  Returns (dtype code, shape, strides); ValueError, naming what is wrong, otherwise."""
    code, shape, strides = strided_layout("heat", ("M", "P", "Hh", "Wh"), shape, strides, code, bits)
    m, p, hh, wh = shape
    if not 1 <= m <= MAX_SLOTS:
        raise ValueError(f"heat: M = {m} is outside 1..{MAX_SLOTS}")
    if not 1 <= p <= MAX_POINTS:
        raise ValueError(f"heat: P = {p} is outside 1..{MAX_POINTS}")
    if not (1 <= hh <= MAX_SIDE and 1 <= wh <= MAX_SIDE):
        raise ValueError(f"heat: Hh x Wh = {hh} x {wh} is outside 1..{MAX_SIDE} a side")
    if hh * wh > MAX_ELEMS:
        raise ValueError(f"heat: Hh * Wh = {hh * wh} exceeds 2^20")
    _unit_last("heat", shape, strides)
    return code, shape, strides


def simcc_layout(who):
    """... for a SimCC vector tensor (M, P, W) named `who`: last stride 1, the others >= 0"""
    def layout(shape, strides, code, bits):
        code, shape, strides = strided_layout(who, ("M", "P", "W"), shape, strides, code, bits)
        m, p, w = shape
        if not 1 <= m <= MAX_SLOTS:
            raise ValueError(f"{who}: M = {m} is outside 1..{MAX_SLOTS}")
        if not 1 <= p <= MAX_POINTS:
            raise ValueError(f"{who}: P = {p} is outside 1..{MAX_POINTS}")
        if not 1 <= w <= MAX_SIDE:
            raise ValueError(f"{who}: W = {w} is outside 1..{MAX_SIDE}")
        _unit_last(who, shape, strides)
        return code, shape, strides
    return layout


def simcc_pair(xview, yview):
    """the two vector tensors belong together: one dtype, one (M, P)"""
    if xview[0] != yview[0]:
        raise ValueError("simcc_x and simcc_y must have one dtype")
    if xview[1][:2] != yview[1][:2]:
        raise ValueError(f"simcc_x is (M, P) = {xview[1][:2]}, simcc_y {yview[1][:2]}")


def mapping_spec(n_frames, m, canvas, matrices, rois, max_det):
    """What Prepare checks of the mapping, without a device; `matrices` and `rois` are the tensors or None.  Returns
    (canvas w, canvas h, D or 0)."""
    batch_size(n_frames)
    try:
        w, h = (operator.index(v) for v in canvas)
    except (TypeError, ValueError):
        raise ValueError("canvas: the (w, h) the crops were cut to") from None
    if not (1 <= w <= MAX_CANVAS and 1 <= h <= MAX_CANVAS):
        raise ValueError(f"canvas: {w} x {h} is outside 1..{MAX_CANVAS} a side")
    if (matrices is None) == (rois is None):
        raise ValueError("give exactly one of matrices and rois: " + ("both" if rois is not None else "neither") + " given")
    if matrices is not None:
        if max_det is not None:
            raise ValueError("max_det goes with rois; matrices name their frame themselves")
        return w, h, 0
    if max_det is None:
        raise ValueError("rois: max_det is required (slot i * max_det + r belongs to frame i)")
    # (no cap on N * max_det: M, which it must equal, has its own in the layouts)
    return w, h, max_det_arg(max_det, n_frames, MAX_DET, cap=None, slots=("rois", m, ""))


def run_spec(kpt_thr, refine, align, simcc):
    """What Run checks of its arguments: (kpt_thr, refine code, align code)"""
    thr = kpt_thr_arg(kpt_thr)
    if refine not in REFINES:
        raise ValueError(f"refine = {refine!r}; one of {', '.join(repr(v) for v in REFINES)}")
    if align not in ALIGNS:
        raise ValueError(f"align = {align!r}; one of {', '.join(repr(v) for v in ALIGNS)}")
    if simcc and refine != "none":
        raise ValueError(f"refine = {refine!r}: SimCC vectors take no refinement (refine=\"none\")")
    return thr, REFINES[refine], ALIGNS[align]


class KeypointBatch(PreparedBatch):
    """What PyKeypointDecoder.Run works on: the frames, the maps, the mapping rows and the outputs, checked and set up
    once (PrepareHeatmaps / PrepareSimcc).  Keeps the surfaces and tensors alive."""

    _owned = ("d_frames",)

    def __init__(self, gpu_id: int, stream: int, frames: Sequence[Surface], heat, simcc, points, canvas, matrices, rois,
                 max_det, kpts):
        frames = list(frames)
        surfaces_on_device("frames", frames, gpu_id)
        self.simcc = heat is None
        self.heat, self.vectors, keep = (0, 0, 0, 0), (0, 0, 0, 0, 0, 0), []
        if self.simcc:
            sx, sy = simcc
            xs, xv = device_float("simcc_x", sx, simcc_layout("simcc_x"), gpu_id, *HEAD_CAI)
            ys, yv = device_float("simcc_y", sy, simcc_layout("simcc_y"), gpu_id, *HEAD_CAI)
            simcc_pair(xv, yv)
            self.dtype, (m, p, wh) = xv[0], xv[1]
            hh = yv[1][2]
            self.vectors = (xs.ptr, xv[2][0], xv[2][1], ys.ptr, yv[2][0], yv[2][1])
            keep += [xs.holder, ys.holder]
        else:
            hs, (self.dtype, (m, p, hh, wh), hstr) = device_float("heat", heat, heat_layout, gpu_id, *HEAD_CAI)
            self.heat = (hs.ptr, hstr[0], hstr[1], hstr[2])
            keep.append(hs.holder)
        w, h, self.D = mapping_spec(len(frames), m, canvas, matrices, rois, max_det)
        self.d_matrices = self.d_rois = self.d_kpts = 0
        if matrices is not None:
            self.d_matrices, _, mh = device_i32("matrices", matrices, (m, 8), gpu_id)
        else:
            self.d_rois, _, mh = device_i32("rois", rois, (m, 8), gpu_id)
        if points is None:
            raise ValueError(f"points: an int32 ({m}, {p}, 4) device tensor is required")
        self.d_points, _, ph = device_i32("points", points, (m, p, 4), gpu_id)
        if self.d_points % 16:
            raise ValueError("points: the tensor must be 16-byte aligned")
        kh = None
        if kpts is not None:
            def kpts_layout(shape, strides, code, bits):
                if (int(code), int(bits)) != (2, 32) or tuple(shape) != (m, p, 3):
                    raise ValueError(f"kpts: need a float32 tensor of shape ({m}, {p}, 3), got {tuple(shape)}")
                if strides is not None and any(s > 1 and st != e for s, st, e in zip(shape, strides, (3 * p, 3, 1))):
                    raise ValueError("kpts: the tensor must be contiguous")
                return None
            ks, _ = device_float("kpts", kpts, kpts_layout, gpu_id, ("<f4",))
            self.d_kpts, kh = ks.ptr, ks.holder
        self._begin(gpu_id, stream, "Prepare", frames)
        self.n, self.m, self.p, self.hh, self.wh, self.canvas = len(frames), m, p, hh, wh, (w, h)
        self._keep = [frames, keep, mh, ph, kh]

    def __len__(self):
        return self.m


class PyKeypointDecoder(_SurfaceTask):
    """Heatmaps (M, P, Hh, Wh), or SimCC vectors (M, P, Wx) and (M, P, Wy), of a network that ran on crops -> one point
    per map in the pixels of the frame its crop was cut from, in ONE launch with nothing allocated and no
    synchronisation, so the call can be captured and replayed after its tensors were rewritten in place
    (vali_kpt_decode).

    kb = PrepareHeatmaps(frames, heat, points, canvas=(w, h), matrices=None, rois=None, max_det=None, kpts=None): `heat`
    is a float32, float16 or bfloat16 GPU tensor (`__dlpack__`, or `__cuda_array_interface__` for float32 and float16)
    with x stride 1 and any other element strides >= 0 (a slice, pitched rows, an expanded tensor).  `canvas` is the size
    the crops were cut to.  Exactly one of `matrices` -- PySurfaceWarper's (M, 8) int32 rows -- and `rois` --
    PyDetectionSelector's (M, 8) int32 records with `max_det` = D and M = N * D, slot i * D + r belonging to frame i -- is
    the way back; `frames` are read for their sizes only.  `points` is a contiguous, 16-byte aligned (M, P, 4) int32 GPU
    tensor -- X, Y, the confidence's float32 bits, flag (0 invisible, 1 visible, 3 visible and inside the frame): the rows
    PyPoseDrawer.RunPoints draws; `kpts`, optional, a contiguous (M, P, 3) float32 one: fx, fy, confidence.  Every row of
    both is rewritten by every call; a skipped slot's rows (a matrix whose frame is outside 0..N-1, an empty roi) are zero.
    kb = PrepareSimcc(frames, simcc_x, simcc_y, points, ...) likewise; the confidence is the smaller of the two peaks and
    Run takes refine="none" only.
    M 1..65535, P 1..64, Hh, Wh, Wx, Wy 1..4096, Hh * Wh <= 2^20.

    Run(kb, kpt_thr=0.3, refine="quarter", align="centre"): the peak is the first of the greatest elements (a NaN never
    is); `refine` "quarter" moves it a quarter of a cell towards the greater neighbour along each axis (heatmaps only),
    "none" leaves it; `align` "centre" places cell x at (x + 0.5) * w / Wh, "index" at x * w / Wh + 0.5 (codecs that label
    in pixel-index coordinates, mmpose's among them).  A point is visible when its confidence is above `kpt_thr`.
    """

    def PrepareHeatmaps(self, frames: Sequence[Surface], heat, points, canvas, matrices=None, rois=None, max_det=None,
                        kpts=None) -> KeypointBatch:
        if heat is None:
            raise ValueError("heat: a float32, float16 or bfloat16 (M, P, Hh, Wh) device tensor is required")
        return KeypointBatch(self._gpu_id, self._stream, frames, heat, None, points, canvas, matrices, rois, max_det, kpts)

    def PrepareSimcc(self, frames: Sequence[Surface], simcc_x, simcc_y, points, canvas, matrices=None, rois=None,
                     max_det=None, kpts=None) -> KeypointBatch:
        if simcc_x is None or simcc_y is None:
            raise ValueError("simcc_x, simcc_y: float32, float16 or bfloat16 (M, P, W) device tensors are required")
        return KeypointBatch(self._gpu_id, self._stream, frames, None, (simcc_x, simcc_y), points, canvas, matrices, rois,
                             max_det, kpts)

    def RunAsync(self, kb: KeypointBatch, kpt_thr=0.3, refine="quarter", align="centre") -> Tuple[bool, TaskExecInfo]:
        if not isinstance(kb, KeypointBatch):
            raise ValueError("Run: pass a KeypointBatch (PrepareHeatmaps / PrepareSimcc)")
        thr, rf, al = run_spec(kpt_thr, refine, align, kb.simcc)
        d = _status(shim.kpt_decode(kb.d_frames, kb.n, kb.dtype, kb.heat, kb.vectors, (kb.m, kb.p, kb.hh, kb.wh),
                                    kb.canvas[0], kb.canvas[1], rf, al, thr, kb.D, kb.d_matrices, kb.d_rois, kb.d_points,
                                    kb.d_kpts, self._stream))
        return d.success, d.info

    def Run(self, kb: KeypointBatch, kpt_thr=0.3, refine="quarter", align="centre") -> Tuple[bool, TaskExecInfo]:
        r = self.RunAsync(kb, kpt_thr, refine, align)
        self._sync()
        return r
