"""PyDetectionSelector: a detector's raw head -> GPU-held detections in frame pixels (vali_detect_select).

Threshold and class arg-max, exact top-T, greedy NMS, the way back through the letterbox and the rows the other tasks
read (annotator marks, crop records), in four launches whatever the data: no box and no class id is ever on the host.
The definition, sample for sample, is in include/vali_hip.h; tests/detect_model.py restates it in numpy.
"""
from __future__ import annotations

import math
import operator
from functools import partial
from typing import Optional, Tuple

from ._batch import PreparedBatch
from ._native import shim
from ._runargs import batch_size, host_rects as _host_rects, max_det_arg, run_rects
from .enums import TaskExecInfo
from .runtime import is_capturing
from .tasks import MAX_MARKS, _SurfaceTask, _status, pack_colour
from .tensors import HEAD_CAI, declared_shape, device_float, device_i32, is_device, strided_layout, upload_i32

MAX_HEAD, MAX_CLASSES, MAX_CANDIDATES = 1 << 20, 4096, 1024

_FORMATS = {"xyxy": 0, "cxcywh": 1}


def head_layout(who, shape, strides, code, bits, last=None):
    """The rules for `boxes` and `scores`, without a device: a 3-D (N, K, last) float32, float16 or bfloat16 view with
    element strides >= 0.  Returns (dtype code, (n, k, c), strides); ValueError, naming what is wrong, otherwise."""
    def limits(shape):
        n, k, c = shape
        if last is not None and c != last:
            raise ValueError(f"{who}: the last dimension must be {last}, got {shape}")
        batch_size(n, who)
        if not 1 <= k <= MAX_HEAD:
            raise ValueError(f"{who}: K = {k} is outside 1..2^20")
        if not 1 <= c <= MAX_CLASSES:
            raise ValueError(f"{who}: C = {c} is outside 1..{MAX_CLASSES}")

    return strided_layout(who, ("N", "K", str(last or "C")), shape, strides, code, bits, limits)


class DetectionStyle:
    """How PyDetectionSelector writes `marks`: an outline of `thickness` in colours[class % len(colours)] per detection
    and, with `label_rects` (LabelAtlas.rects, (L, 4) rows u, v, w, h), the label's background in that colour at alpha
    `label_alpha` and its text in `text_colour` on top of the box's upper edge.  `colours` and `label_rects` are int32
    device tensors, or host values that are uploaded once, at the first Run that uses the style."""

    def __init__(self, thickness: int = 2, colours=(pack_colour(40, 255, 80),), label_rects=None, label_alpha: int = 200,
                 text_colour: int = pack_colour(0, 0, 0)):
        self.thickness = operator.index(thickness)
        if self.thickness < 1:
            raise ValueError("DetectionStyle: thickness must be at least 1")
        self.label_alpha = operator.index(label_alpha)
        if not 0 <= self.label_alpha <= 255:
            raise ValueError("DetectionStyle: label_alpha in 0..255")
        self.text_colour = operator.index(text_colour)
        if not -(1 << 31) <= self.text_colour < (1 << 31):
            raise ValueError("DetectionStyle: text_colour must fit an int32 (pack_colour)")
        self.colours, self.label_rects = colours, label_rects
        if not is_device(colours):
            self.colours = [operator.index(v) for v in colours]
            if not self.colours:
                raise ValueError("DetectionStyle: at least one colour")
            if any(not -(1 << 31) <= v < (1 << 31) for v in self.colours):
                raise ValueError("DetectionStyle: every colour must fit an int32 (pack_colour)")
        if label_rects is not None and not is_device(label_rects):
            rows = [tuple(operator.index(v) for v in r) for r in label_rects]
            if not rows or any(len(r) != 4 for r in rows):
                raise ValueError("DetectionStyle: label_rects must be (L, 4) rows (u, v, w, h), L >= 1")
            self.label_rects = rows
        self._dev = {}       # gpu_id -> (d_colours, n_colours, d_labels, n_labels, holders, owned)

    def device(self, gpu_id, stream):
        """(d_colours, n_colours, d_label_rects, n_labels) on `gpu_id`"""
        got = self._dev.get(gpu_id)
        if got is None:
            holders, owned = [], []
            host = not is_device(self.colours) or (self.label_rects is not None and not is_device(self.label_rects))
            if host and is_capturing(gpu_id, stream):
                raise RuntimeError("DetectionStyle: host colours / label_rects cannot be uploaded while the stream is "
                                   "capturing -- Run once before the capture, or pass device tensors")

            def rows(who, values, shape, want):
                """(device pointer, rows) of a device tensor, or of host values uploaded here"""
                if is_device(values):
                    d, seen, h = device_i32(who, values, shape, gpu_id, want=want)
                    holders.append(h)
                    return d, seen[0]
                d = upload_i32(gpu_id, stream, values if len(shape) == 1 else [v for r in values for v in r])
                owned.append(d)
                return d, len(values)

            dc, nc = rows("style.colours", self.colours, (None,), "(n,)")
            dl, nl = (0, 0) if self.label_rects is None else rows("style.label_rects", self.label_rects, (None, 4), "(L, 4)")
            got = self._dev[gpu_id] = (dc, nc, dl, nl, holders, owned, stream)
        return got[:4]

    def __del__(self):
        for gpu_id, got in getattr(self, "_dev", {}).items():
            if got[5]:
                try:
                    shim.stream_sync(gpu_id, got[6])
                except Exception:
                    pass
            for p in got[5]:
                try:
                    shim.mem_free(gpu_id, p)
                except Exception:
                    pass


def select_spec(boxes_view, scores_view, box_format="xyxy", max_candidates=1024, max_det=100, rows=(False, False, 0)):
    """What Prepare checks once the tensors are seen, without a device: views are (dtype code, (n, k, c), strides).
    `rows`: (has rois, has marks, rows of marks).  Returns (n, k, c, T, D, format code, R)."""
    (_, (n, k, _), _), (_, (n2, k2, c), _) = boxes_view, scores_view
    if (n, k) != (n2, k2):
        raise ValueError(f"boxes and scores disagree: boxes are ({n}, {k}, 4), scores ({n2}, {k2}, {c})")
    if box_format not in _FORMATS:
        raise ValueError(f"box_format: 'xyxy' or 'cxcywh', got {box_format!r}")
    T, D = operator.index(max_candidates), operator.index(max_det)
    if not 1 <= T <= MAX_CANDIDATES:
        raise ValueError(f"max_candidates = {T} is outside 1..{MAX_CANDIDATES}")
    max_det_arg(D, n, T, f"max_candidates ({T})")
    R = 0
    if rows[1]:
        m = rows[2]
        if m not in (n * D, 3 * n * D):
            raise ValueError(f"marks: need ({n * D}, 8) rows (outlines) or ({3 * n * D}, 8) (outlines and labels), got {m}")
        if m > MAX_MARKS:
            raise ValueError(f"marks: {m} rows; the annotator takes at most {MAX_MARKS} per call")
        R = m // (n * D)
    return n, k, c, T, D, _FORMATS[box_format], R


def run_spec(R, has_rois, score_thr, iou_thr, crop_placement, style):
    """What Run checks before it looks at `rects`: (score_thr, iou_thr, crop)"""
    score_thr, iou_thr = float(score_thr), float(iou_thr)
    if not math.isfinite(score_thr):
        raise ValueError(f"score_thr must be finite, got {score_thr}")
    if not math.isfinite(iou_thr):
        raise ValueError(f"iou_thr must be finite, got {iou_thr}")
    crop = (0, 0, 0, 0)
    if has_rois:
        if crop_placement is None:
            raise ValueError("crop_placement: four integers (px, py, pw, ph) are required when the batch has rois")
        crop = tuple(operator.index(v) for v in crop_placement)
        if len(crop) != 4 or any(not -(1 << 31) <= v < (1 << 31) for v in crop):
            raise ValueError("crop_placement: four int32 values (px, py, pw, ph)")
    if R:
        if not isinstance(style, DetectionStyle):
            raise ValueError("style: a DetectionStyle is required when the batch has marks")
        if (R == 3) != (style.label_rects is not None):
            raise ValueError("style: marks of 3 * N * max_det rows need a style with label_rects, N * max_det rows one "
                             "without")
    return score_thr, iou_thr, crop


class SelectBatch(PreparedBatch):
    """What PyDetectionSelector.Run works on: the head's two tensors, the output tensors and the workspace, checked and
    set up once (PyDetectionSelector.Prepare).  Keeps the tensors alive."""

    _owned = ("d_ws", "d_rects")

    def __init__(self, gpu_id: int, stream: int, boxes, scores, dets, counts=None, rois=None, marks=None,
                 box_format="xyxy", max_candidates=1024, max_det=100):
        bseen, (bcode, bshape, bstr) = device_float("boxes", boxes, partial(head_layout, "boxes", last=4), gpu_id, *HEAD_CAI)
        sseen, (scode, sshape, sstr) = device_float("scores", scores, partial(head_layout, "scores"), gpu_id, *HEAD_CAI)
        mrows = 0
        if marks is not None:
            mshape = declared_shape(marks)
            mrows = mshape[0] if len(mshape) == 2 else -1
        n, k, c, T, D, fmt, R = select_spec((bcode, bshape, bstr), (scode, sshape, sstr), box_format, max_candidates,
                                            max_det, (rois is not None, marks is not None, mrows))
        if dets is None:
            raise ValueError(f"dets: an int32 ({n * D}, 8) device tensor is required")
        keep = [bseen.holder, sseen.holder]
        self.d_dets = self.d_counts = self.d_rois = self.d_marks = 0
        for name, t, shape in (("dets", dets, (n * D, 8)), ("counts", counts, (n,)), ("rois", rois, (n * D, 8)),
                               ("marks", marks, (R * n * D, 8))):
            if t is not None:
                ptr, _, h = device_i32(name, t, shape, gpu_id)
                setattr(self, "d_" + name, ptr)
                keep.append(h)
        self._begin(gpu_id, stream, "Prepare()", rects=n)
        self.n, self.k, self.c, self.T, self.D, self.R = n, k, c, T, D, R
        self.box_format = fmt
        self.boxes = (bseen.ptr, bcode, *bstr)
        self.scores = (sseen.ptr, scode, *sstr)
        self._keep = keep
        self._style_keep = None
        self.ws_bytes = shim.detect_workspace_size(n, k, T)
        self.d_ws = shim.mem_alloc(gpu_id, self.ws_bytes)


class PyDetectionSelector(_SurfaceTask):
    """The step between a network and everything that consumes its detections, on the GPU: score threshold and class
    arg-max, exact top-`max_candidates`, greedy NMS, the way back through the letterbox, and the rows the other tasks
    read -- in four launches whatever the data, with nothing allocated and no synchronisation, so the call can be
    captured and replayed after its input tensors were rewritten in place (vali_detect_select).

    sb = Prepare(boxes, scores, dets, counts=None, rois=None, marks=None, box_format="xyxy", max_candidates=1024,
    max_det=100): `boxes` (N, K, 4) and `scores` (N, K, C) are float32, float16 or bfloat16 GPU tensors with any
    element strides >= 0 (`__dlpack__`, or `__cuda_array_interface__` for float32 and float16) -- a YOLOv8 head
    (N, 4 + C, K) goes in as pred[:, :4].transpose(1, 2) and pred[:, 4:].transpose(1, 2), without a copy.  N 1..1024,
    K 1..2^20, C 1..4096, max_candidates T 1..1024, max_det D 1..T, N * D <= 65535.  The outputs are contiguous int32
    GPU tensors, every row rewritten by every call: dets (N * D, 8) rows (frame, x, y, w, h, class, score bits, k),
    unused (-1, 0, ...); counts (N,); rois (N * D, 8) rows (x, y, w, h, *crop_placement), the `rects=` of a RoiBatch /
    TensorBatch whose item i * D + r has frame i as its source, unused all zero; marks (R * N * D, 8) annotator rows,
    R = 3 with style.label_rects and 1 without, R * N * D <= 4096.

    Run(sb, rects, score_thr=0.25, iou_thr=0.45, class_agnostic=False, crop_placement=None, style=None): `rects` is the
    (N, 8) int32 record array the frames were placed with (PrepareTensorBatch), a device tensor whose values are
    sanitised on the device, or a host sequence of 8-tuples that is uploaded with one blocking copy.
    """

    def Prepare(self, boxes, scores, dets, counts=None, rois=None, marks=None, box_format="xyxy",
                max_candidates=1024, max_det=100) -> SelectBatch:
        return SelectBatch(self._gpu_id, self._stream, boxes, scores, dets, counts, rois, marks, box_format,
                           max_candidates, max_det)

    def RunAsync(self, sb: SelectBatch, rects, score_thr=0.25, iou_thr=0.45, class_agnostic=False, crop_placement=None,
                 style: Optional[DetectionStyle] = None) -> Tuple[bool, TaskExecInfo]:
        if not isinstance(sb, SelectBatch):
            raise ValueError("Run: pass a SelectBatch (Prepare)")
        score_thr, iou_thr, crop = run_spec(sb.R, bool(sb.d_rois), score_thr, iou_thr, crop_placement, style)
        d_rects = run_rects(sb, rects, self._gpu_id, self._stream)
        dc = nc = dl = nl = 0
        thickness, label_alpha, text_colour = 1, 0, 0
        if sb.R:
            dc, nc, dl, nl = style.device(self._gpu_id, self._stream)
            thickness, label_alpha, text_colour = style.thickness, style.label_alpha, style.text_colour
            sb._style_keep = style
        d = _status(shim.detect_select(sb.boxes, sb.scores, sb.n, sb.k, sb.c, sb.T, sb.D, score_thr, iou_thr,
                                       1 if class_agnostic else 0, sb.box_format, crop, thickness, label_alpha,
                                       text_colour, nc, nl, d_rects, sb.d_dets, sb.d_counts, sb.d_rois, sb.d_marks,
                                       dc, dl, sb.d_ws, sb.ws_bytes, self._stream))
        return d.success, d.info

    def Run(self, sb: SelectBatch, rects, score_thr=0.25, iou_thr=0.45, class_agnostic=False, crop_placement=None,
            style: Optional[DetectionStyle] = None) -> Tuple[bool, TaskExecInfo]:
        r = self.RunAsync(sb, rects, score_thr, iou_thr, class_agnostic, crop_placement, style)
        self._sync()
        return r
