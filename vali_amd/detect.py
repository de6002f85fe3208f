"""PyDetectionSelector: a detector's raw head -> GPU-held detections in frame pixels (vali_detect_select).

Threshold and class arg-max, exact top-T, greedy NMS, the way back through the letterbox and the rows the other tasks
read (annotator marks, crop records), in four launches whatever the data: no box and no class id is ever on the host.
The definition, sample for sample, is in include/vali_hip.h; tests/detect_model.py restates it in numpy.
"""
from __future__ import annotations

import math
import operator
from typing import Optional, Tuple

from ._native import shim
from .enums import DLDeviceType, TaskExecInfo
from .runtime import is_capturing
from .tasks import MAX_MARKS, _SurfaceTask, _device_rects, _release, _status, pack_colour

MAX_FRAMES, MAX_HEAD, MAX_CLASSES, MAX_CANDIDATES = 1024, 1 << 20, 4096, 1024

# DLPack (code, bits) -> (name, enum vali_dtype)
_DTYPES = {(2, 32): ("float32", 0), (2, 16): ("float16", 1), (4, 16): ("bfloat16", 2)}
_CAI = {"<f4": (2, 32), "<f2": (2, 16)}
_FORMATS = {"xyxy": 0, "cxcywh": 1}


def head_layout(who, shape, strides, code, bits, last=None):
    """The rules for `boxes` and `scores`, without a device: a 3-D (N, K, last) float32, float16 or bfloat16 view with
    element strides >= 0.  Returns (dtype code, (n, k, c), strides); ValueError, naming what is wrong, otherwise."""
    dtype = _DTYPES.get((int(code), int(bits)))
    if dtype is None:
        raise ValueError(f"{who}: the dtype must be float32, float16 or bfloat16 (DLPack code {code}, {bits} bits)")
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3:
        raise ValueError(f"{who}: need a 3-D tensor (N, K, {last or 'C'}), got {len(shape)}-D {shape}")
    n, k, c = shape
    if last is not None and c != last:
        raise ValueError(f"{who}: the last dimension must be {last}, got {shape}")
    if not 1 <= n <= MAX_FRAMES:
        raise ValueError(f"{who}: N = {n} is outside 1..{MAX_FRAMES}")
    if not 1 <= k <= MAX_HEAD:
        raise ValueError(f"{who}: K = {k} is outside 1..2^20")
    if not 1 <= c <= MAX_CLASSES:
        raise ValueError(f"{who}: C = {c} is outside 1..{MAX_CLASSES}")
    if strides is None:
        strides = (k * c, c, 1)
    strides = tuple(int(v) for v in strides)
    if len(strides) != 3:
        raise ValueError(f"{who}: {len(strides)} strides for a 3-D tensor")
    if any(v < 0 for v in strides):
        raise ValueError(f"{who}: negative strides {strides} (a flipped view) are not supported")
    if any(v > 1 << 40 for v in strides):
        raise ValueError(f"{who}: strides {strides} beyond 2^40 elements")
    return dtype[1], shape, strides


def _head_view(who, t, gpu_id, last=None):
    """(ptr, dtype code, (n, k, c), strides, holder) of a device tensor on `gpu_id`"""
    if hasattr(t, "__dlpack__"):
        info, holder = shim.dlpack_import(t.__dlpack__())
        if info["lanes"] != 1:
            raise ValueError(f"{who}: vector dtypes are not supported")
        code, shape, strides = head_layout(who, info["shape"], info["strides"], info["code"], info["bits"], last)
        if info["device_type"] not in (int(DLDeviceType.kDLROCM), int(DLDeviceType.kDLCUDA)):
            raise ValueError(f"{who}: the tensor must live on the GPU")
        ptr, device = int(info["ptr"]), int(info["device_id"])
    elif hasattr(t, "__cuda_array_interface__"):
        cai = t.__cuda_array_interface__
        if cai["typestr"] not in _CAI:
            raise ValueError(f"{who}: the dtype must be float32 or float16 through __cuda_array_interface__ (bfloat16: "
                             f"__dlpack__), got {cai['typestr']}")
        dl_code, bits = _CAI[cai["typestr"]]
        strides = cai.get("strides")
        if strides is not None:
            if any(int(v) % (bits // 8) for v in strides):
                raise ValueError(f"{who}: strides that are no multiple of the element size")
            strides = tuple(int(v) // (bits // 8) for v in strides)
        code, shape, strides = head_layout(who, cai["shape"], strides, dl_code, bits, last)
        ptr, holder = int(cai["data"][0]), t
        dev = getattr(t, "device", None)
        if getattr(dev, "type", "cuda") != "cuda":
            raise ValueError(f"{who}: the tensor must live on the GPU")
        device = dev.index if dev is not None and dev.index is not None else shim.ptr_device(ptr)
    else:
        raise ValueError(f"{who}: a device tensor with __dlpack__ or __cuda_array_interface__")
    if device != gpu_id:
        raise ValueError(f"{who}: the tensor is on device {device}, the task on {gpu_id}")
    return ptr, code, shape, strides, holder


def _device_i32(who, t, shape, gpu_id):
    """(device pointer, holder) of a contiguous int32 device tensor of exactly `shape`: _device_marks' checks"""
    want = "x".join(str(v) for v in shape)
    if hasattr(t, "__cuda_array_interface__"):
        cai = t.__cuda_array_interface__
        got = tuple(int(v) for v in cai["shape"])
        if cai["typestr"] not in ("<i4", "|i4") or got != tuple(shape):
            raise ValueError(f"{who}: need an int32 tensor of shape ({want}), got {cai['typestr']} {got}")
        strides = cai.get("strides")
        if strides is not None:
            expect = 4
            for size, st in zip(reversed(got), reversed([int(v) for v in strides])):
                if size != 1 and st != expect:
                    raise ValueError(f"{who}: the tensor must be contiguous")
                expect *= size
        ptr, holder = int(cai["data"][0]), t
        dev = getattr(t, "device", None)
        if getattr(dev, "type", "cuda") != "cuda":
            raise ValueError(f"{who}: the tensor must live on the GPU")
        device = dev.index if dev is not None and dev.index is not None else shim.ptr_device(ptr)
    elif hasattr(t, "__dlpack__"):
        info, holder = shim.dlpack_import(t.__dlpack__())
        got, strides = tuple(info["shape"]), tuple(info["strides"])
        if info["code"] != 0 or info["bits"] != 32 or info["lanes"] != 1 or got != tuple(shape):
            raise ValueError(f"{who}: need an int32 tensor of shape ({want}), got shape {got}")
        expect = 1
        for size, st in zip(reversed(got), reversed(strides)):
            if size != 1 and st != expect:
                raise ValueError(f"{who}: the tensor must be contiguous")
            expect *= size
        if info["device_type"] not in (int(DLDeviceType.kDLROCM), int(DLDeviceType.kDLCUDA)):
            raise ValueError(f"{who}: the tensor must live on the GPU")
        ptr, device = int(info["ptr"]), int(info["device_id"])
    else:
        raise ValueError(f"{who}: a device tensor with __cuda_array_interface__ or __dlpack__")
    if device != gpu_id:
        raise ValueError(f"{who}: the tensor is on device {device}, the task on {gpu_id}")
    return ptr, holder


def _is_device(t):
    """a device tensor, as opposed to host values (numpy arrays speak DLPack too: theirs is the CPU's)"""
    if hasattr(t, "__cuda_array_interface__"):
        return True
    if hasattr(t, "__dlpack__"):
        where = getattr(t, "__dlpack_device__", None)
        return where is None or int(where()[0]) != int(DLDeviceType.kDLCPU)
    return False


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
        if not _is_device(colours):
            self.colours = [operator.index(v) for v in colours]
            if not self.colours:
                raise ValueError("DetectionStyle: at least one colour")
            if any(not -(1 << 31) <= v < (1 << 31) for v in self.colours):
                raise ValueError("DetectionStyle: every colour must fit an int32 (pack_colour)")
        if label_rects is not None and not _is_device(label_rects):
            rows = [tuple(operator.index(v) for v in r) for r in label_rects]
            if not rows or any(len(r) != 4 for r in rows):
                raise ValueError("DetectionStyle: label_rects must be (L, 4) rows (u, v, w, h), L >= 1")
            self.label_rects = rows
        self._dev = {}       # gpu_id -> (d_colours, n_colours, d_labels, n_labels, holders, owned)

    @staticmethod
    def _rows_of(who, t, width):
        shape = (t.__cuda_array_interface__["shape"] if hasattr(t, "__cuda_array_interface__") else t.shape)
        shape = tuple(int(v) for v in shape)
        if len(shape) != (2 if width else 1) or shape[0] < 1 or (width and shape[1] != width):
            raise ValueError(f"{who}: need an int32 tensor of shape " + (f"(L, {width})" if width else "(n,)") + f", got {shape}")
        return shape

    def _upload(self, gpu_id, stream, values):
        import array

        buf = array.array("i", values)
        nbytes = 4 * len(values)
        d = shim.mem_alloc(gpu_id, nbytes)
        shim.memcpy2d_async(gpu_id, d, nbytes, buf.buffer_info()[0], nbytes, nbytes, 1, 0, stream)
        shim.stream_sync(gpu_id, stream)
        return d

    def device(self, gpu_id, stream):
        """(d_colours, n_colours, d_label_rects, n_labels) on `gpu_id`"""
        got = self._dev.get(gpu_id)
        if got is None:
            holders, owned = [], []
            host = not _is_device(self.colours) or (self.label_rects is not None and not _is_device(self.label_rects))
            if host and is_capturing(gpu_id, stream):
                raise RuntimeError("DetectionStyle: host colours / label_rects cannot be uploaded while the stream is "
                                   "capturing -- Run once before the capture, or pass device tensors")
            if _is_device(self.colours):
                shape = self._rows_of("style.colours", self.colours, 0)
                dc, h = _device_i32("style.colours", self.colours, shape, gpu_id)
                nc = shape[0]
                holders.append(h)
            else:
                dc, nc = self._upload(gpu_id, stream, self.colours), len(self.colours)
                owned.append(dc)
            dl, nl = 0, 0
            if self.label_rects is not None:
                if _is_device(self.label_rects):
                    shape = self._rows_of("style.label_rects", self.label_rects, 4)
                    dl, h = _device_i32("style.label_rects", self.label_rects, shape, gpu_id)
                    nl = shape[0]
                    holders.append(h)
                else:
                    dl, nl = self._upload(gpu_id, stream, [v for r in self.label_rects for v in r]), len(self.label_rects)
                    owned.append(dl)
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
    if not 1 <= D <= T:
        raise ValueError(f"max_det = {D} is outside 1..max_candidates ({T})")
    if n * D > 65535:
        raise ValueError(f"N * max_det = {n * D} exceeds 65535")
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


def _host_rects(rects, n):
    try:
        rows = [tuple(operator.index(v) for v in r) for r in rects]
    except TypeError:
        raise ValueError("rects: a device tensor with __cuda_array_interface__ or __dlpack__, or a sequence of "
                         "8-tuples") from None
    if len(rows) != n or any(len(r) != 8 for r in rows):
        raise ValueError(f"rects: need {n} rows of 8 integers (src_x, src_y, src_w, src_h, dst_x, dst_y, dst_w, dst_h)")
    if any(not -(1 << 31) <= v < (1 << 31) for r in rows for v in r):
        raise ValueError("rects: every value must fit an int32")
    return rows


class SelectBatch:
    """What PyDetectionSelector.Run works on: the head's two tensors, the output tensors and the workspace, checked and
    set up once (PyDetectionSelector.Prepare).  Keeps the tensors alive."""

    def __init__(self, gpu_id: int, stream: int, boxes, scores, dets, counts=None, rois=None, marks=None,
                 box_format="xyxy", max_candidates=1024, max_det=100):
        bp, bcode, bshape, bstr, bh = _head_view("boxes", boxes, gpu_id, 4)
        sp, scode, sshape, sstr, sh = _head_view("scores", scores, gpu_id)
        mrows = 0
        if marks is not None:
            mshape = (marks.__cuda_array_interface__["shape"] if hasattr(marks, "__cuda_array_interface__")
                      else getattr(marks, "shape", ()))
            mrows = int(mshape[0]) if len(mshape) == 2 else -1
        n, k, c, T, D, fmt, R = select_spec((bcode, bshape, bstr), (scode, sshape, sstr), box_format, max_candidates,
                                            max_det, (rois is not None, marks is not None, mrows))
        if dets is None:
            raise ValueError(f"dets: an int32 ({n * D}, 8) device tensor is required")
        keep = [bh, sh]
        self.d_dets, h = _device_i32("dets", dets, (n * D, 8), gpu_id)
        keep.append(h)
        self.d_counts = self.d_rois = self.d_marks = 0
        if counts is not None:
            self.d_counts, h = _device_i32("counts", counts, (n,), gpu_id)
            keep.append(h)
        if rois is not None:
            self.d_rois, h = _device_i32("rois", rois, (n * D, 8), gpu_id)
            keep.append(h)
        if marks is not None:
            self.d_marks, h = _device_i32("marks", marks, (R * n * D, 8), gpu_id)
            keep.append(h)
        if is_capturing(gpu_id, stream):
            raise RuntimeError("SelectBatch: cannot be created while the stream is capturing -- Prepare() before the "
                               "StreamCapture block and Keep() the batch with the capture")
        self.gpu_id, self._stream = gpu_id, stream
        self.n, self.k, self.c, self.T, self.D, self.R = n, k, c, T, D, R
        self.box_format = fmt
        self.boxes = (bp, bcode, *bstr)
        self.scores = (sp, scode, *sstr)
        self._keep = keep
        self._rects_keep = self._style_keep = None
        self.d_ws = self.d_rects = 0
        self.ws_bytes = shim.detect_workspace_size(n, k, T)
        self.d_ws = shim.mem_alloc(gpu_id, self.ws_bytes)
        self.d_rects = shim.mem_alloc(gpu_id, 32 * n)

    def __len__(self):
        return self.n

    def __del__(self):
        _release(self, ("d_ws", "d_rects"))


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
        if _is_device(rects):
            d_rects, sb._rects_keep = _device_rects(rects, sb.n, self._gpu_id)
        else:
            import array

            rows = _host_rects(rects, sb.n)
            buf = array.array("i", [v for r in rows for v in r])
            nbytes = 32 * sb.n
            shim.memcpy2d_async(self._gpu_id, sb.d_rects, nbytes, buf.buffer_info()[0], nbytes, nbytes, 1, 0, self._stream)
            shim.stream_sync(self._gpu_id, self._stream)      # `buf` goes with this call
            d_rects = sb.d_rects
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
