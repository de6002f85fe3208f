"""PySemanticPainter: a semantic segmentation head's class logits -> a class map per frame and the classes tinted onto
the frames, on the GPU (vali_semantic_paint).

The logits (N, C, Hs, Ws) are upsampled bilinearly to the frame through the record the frame was placed with, arg-maxed per
pixel, written as labels and blended in place, class by class, in one launch whatever the data: nothing like an
(N, C, H, W) tensor ever exists.  The definition, sample for sample, is in include/vali_hip.h; tests/semantic_model.py
restates it in numpy.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

from ._batch import PAINT_FORMATS, PreparedBatch, frames_of_one_format, surfaces_on_device
from ._native import shim
from ._runargs import alpha_arg, batch_size, host_colours, net_size_arg, run_colours, run_rects
from .enums import PixelFormat, TaskExecInfo
from .surface import Surface
from .tasks import _UNSUPP_CC_PAIR, _SurfaceTask, _rgb2yuv_params, _status
from .tensors import HEAD_CAI, device_float, strided_layout

MAX_CLASSES, MAX_SIDE = 255, 4096


def logits_layout(shape, strides, code, bits):
    """The rules for `logits`, without a device: (N, C, Hs, Ws) with an x stride of 1.  Returns (dtype code, shape,
    strides); ValueError, naming what is wrong, otherwise."""
    code, shape, strides = strided_layout("logits", ("N", "C", "Hs", "Ws"), shape, strides, code, bits)
    n, c, hs, ws = shape
    batch_size(n, "logits")
    if not 1 <= c <= MAX_CLASSES:
        raise ValueError(f"logits: C = {c} is outside 1..{MAX_CLASSES}")
    if not (1 <= hs <= MAX_SIDE and 1 <= ws <= MAX_SIDE):
        raise ValueError(f"logits: Hs x Ws = {hs} x {ws} is outside 1..{MAX_SIDE}")
    if ws > 1 and strides[3] != 1:
        raise ValueError(f"logits: the x stride must be 1, got {strides[3]}")
    return code, shape, strides


def semantic_spec(frame_sizes, logits_view, label_views=None, net_size=(512, 512)):
    """What Prepare checks once the tensor is seen, without a device: `frame_sizes` the (width, height) of the frames,
    `logits_view` (dtype code, shape, strides) as logits_layout returns it, `label_views` None or (format, width, height)
    of every label surface.  Returns (n, c, hs, ws, net_w, net_h)."""
    _, (n, c, hs, ws), _ = logits_view
    if len(frame_sizes) != n:
        raise ValueError(f"frames: {len(frame_sizes)} surfaces for logits of N = {n}")
    net_w, net_h = net_size_arg(net_size)
    if label_views is not None:
        if len(label_views) != n:
            raise ValueError(f"labels: {len(label_views)} surfaces for {n} frames")
        for i, ((fmt, w, h), (fw, fh)) in enumerate(zip(label_views, frame_sizes)):
            if fmt != PixelFormat.Y:
                raise ValueError(f"labels: surface {i} has format {fmt!r}, need Y")
            if (w, h) != (fw, fh):
                raise ValueError(f"labels: surface {i} is {w}x{h}, its frame {fw}x{fh}")
    return n, c, hs, ws, net_w, net_h


def paint_spec(colours, alpha, has_labels):
    """What Run checks of its host arguments: (host colours, or None for a device tensor or no colours; alpha as the C
    ABI takes it)"""
    a = alpha_arg(alpha)
    if colours is None:
        if not has_labels:
            raise ValueError("colours=None paints nothing and only writes labels: Prepare the batch with labels")
        return None, a
    return host_colours("colours", colours), a


class SemanticBatch(PreparedBatch):
    """What PySemanticPainter.Run works on: the frames, the logits and the label surfaces, checked and set up once
    (PySemanticPainter.Prepare).  Keeps the surfaces and the tensor alive."""

    _owned = ("d_frames", "d_labels", "d_rects", "d_colours")

    def __init__(self, gpu_id: int, stream: int, frames: Sequence[Surface], logits, labels=None, net_size=(512, 512)):
        frames = list(frames)
        fmt = frames_of_one_format("SemanticBatch", frames, PAINT_FORMATS, gpu_id)
        seen, view = device_float("logits", logits, logits_layout, gpu_id, *HEAD_CAI)
        label_views = None
        if labels is not None:
            labels = list(labels)
            surfaces_on_device("labels", labels, gpu_id)
            label_views = [(s.Format, s.Width, s.Height) for s in labels]
        n, c, hs, ws, net_w, net_h = semantic_spec([(d.Width, d.Height) for d in frames], view, label_views, net_size)
        self._begin(gpu_id, stream, "Prepare()", frames, rects=n, colours=True)
        code, _, strides = view
        self.n, self.c, self.hs, self.ws = n, c, hs, ws
        self.net_w, self.net_h = net_w, net_h
        self.format = fmt
        self.label_descs = [s.desc() for s in labels] if labels is not None else []
        self.logits = (seen.ptr, code, strides[0], strides[1], strides[2])
        self._keep = [frames, labels, seen.holder]
        if self.label_descs:
            self.d_labels = shim.descs_upload(gpu_id, self.label_descs, stream)


class PySemanticPainter(_SurfaceTask):
    """The class map of a semantic segmentation network (DeepLab, SegFormer, BiSeNet, portrait and road segmenters)
    written per frame and tinted IN PLACE onto a batch of NV12, YUV420, YUV444, RGB, BGR or RGB_PLANAR frames of any
    sizes, in one launch whatever the data, with nothing allocated and no synchronisation, so the call can be captured and
    replayed after its tensors and frames were rewritten in place (vali_semantic_paint).

    sb = Prepare(frames, logits, labels=None, net_size=(512, 512)): `logits` (N, C, Hs, Ws) is a float32, float16 or
    bfloat16 GPU tensor (`__dlpack__`, or `__cuda_array_interface__` for float32 and float16) with an x stride of 1 and
    any n, c, y strides >= 0 (a (1, C, Hs, Ws) tensor expanded over N, a slice of a larger head).  `labels`: None, or N
    surfaces of format Y, labels[i] of the size of frames[i]: every pixel is rewritten by every call with its class, or
    255 outside the frame's source rectangle.  N 1..1024, C 1..255, Hs and Ws 1..4096, net_size (the network input's
    width and height) 1..65535.  C = 1 is a binary head: class 1 where the logit is above 0, else class 0.

    Run(sb, rects, colours, alpha=128, cc_ctx=None): `rects` is the (N, 8) int32 record array the frames were placed with,
    handled as PyDetectionSelector.Run handles it; `colours` packed colours (pack_colour) as a host sequence, uploaded
    when it changes, or an int32 device tensor: class c is painted in colours[c % len(colours)] at `alpha` (None: the
    colour's own, so a class whose colour has alpha 0 stays untouched).  colours=None paints nothing and only writes the
    labels.  `cc_ctx` picks the RGB -> YUV matrix as PySurfaceAnnotator.RunBatch does.
    """

    def Prepare(self, frames: Sequence[Surface], logits, labels: Optional[Sequence[Surface]] = None,
                net_size=(512, 512)) -> SemanticBatch:
        return SemanticBatch(self._gpu_id, self._stream, frames, logits, labels, net_size)

    def RunAsync(self, sb: SemanticBatch, rects, colours, alpha=128, cc_ctx=None) -> Tuple[bool, TaskExecInfo]:
        if not isinstance(sb, SemanticBatch):
            raise ValueError("Run: pass a SemanticBatch (Prepare)")
        host, a = paint_spec(colours, alpha, bool(sb.d_labels))
        dc, nc, params = 0, 0, None
        if colours is not None:
            supported, params = _rgb2yuv_params(sb.format, cc_ctx)
            if not supported:
                return _UNSUPP_CC_PAIR
            dc, nc = run_colours("PySemanticPainter", sb, "colours", colours, host, self._gpu_id, self._stream)
        d_rects = run_rects(sb, rects, self._gpu_id, self._stream)
        d = _status(shim.semantic_paint(sb.descs, sb.d_frames, int(sb.format), sb.logits, sb.c, sb.hs, sb.ws, sb.net_w,
                                        sb.net_h, d_rects, sb.label_descs, sb.d_labels, dc, nc, a, params, self._stream))
        return d.success, d.info

    def Run(self, sb: SemanticBatch, rects, colours, alpha=128, cc_ctx=None) -> Tuple[bool, TaskExecInfo]:
        r = self.RunAsync(sb, rects, colours, alpha, cc_ctx)
        self._sync()
        return r
