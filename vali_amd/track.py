"""PyDetectionTracker: PyDetectionSelector's rows -> the same rows with an identity that lasts, on the GPU
(vali_track_update).

A greedy IoU tracker with a constant-velocity prediction whose whole state is a tensor of the caller's: one launch per
call whatever the data, nothing allocated, no synchronisation, so the chain decode -> preprocess -> network -> select ->
track -> draw -> encode stays on the device and can be captured.  The definition, step for step, is in
include/vali_hip.h; tests/track_model.py restates it in numpy.
"""
from __future__ import annotations

import math
import operator
from typing import Optional, Tuple

from ._batch import PreparedBatch
from ._native import shim
from ._runargs import MAX_FRAMES
from .detect import DetectionStyle
from .enums import TaskExecInfo
from .tasks import MAX_MARKS, _SurfaceTask, _status
from .tensors import declared_shape, device_i32

MAX_DET, MAX_TRACKS, MAX_ROWS, MAX_AGE = 1024, 256, 65535, 1 << 20


def _rows(t):
    """the rows a 2-D tensor declares, -1 for any other rank"""
    shape = declared_shape(t)
    return shape[0] if len(shape) == 2 else -1


def track_spec(det_rows, streams, max_det, max_tracks, mark_rows=None):
    """What Prepare checks before it reads a tensor, without a device: `det_rows` and `mark_rows` are the rows `dets` and
    `marks` declare.  Returns (S, F, N, D, T, R)."""
    S, D, T = operator.index(streams), operator.index(max_det), operator.index(max_tracks)
    if not 1 <= S <= MAX_FRAMES:
        raise ValueError(f"streams = {S} is outside 1..{MAX_FRAMES}")
    if not 1 <= D <= MAX_DET:
        raise ValueError(f"max_det = {D} is outside 1..{MAX_DET}")
    if not 1 <= T <= MAX_TRACKS:
        raise ValueError(f"max_tracks = {T} is outside 1..{MAX_TRACKS}")
    if det_rows < D or det_rows % D:
        raise ValueError(f"dets: need (N * max_det, 8) rows with max_det = {D}, got {det_rows} rows")
    n = det_rows // D
    if n > MAX_FRAMES:
        raise ValueError(f"dets: N = {n} frames; need 1..{MAX_FRAMES}")
    if n * D > MAX_ROWS:
        raise ValueError(f"N * max_det = {n * D} exceeds {MAX_ROWS}")
    if n % S:
        raise ValueError(f"N = {n} frames is not a multiple of streams = {S}: every stream has the same number of frames")
    R = 0
    if mark_rows is not None:
        if mark_rows not in (n * D, 3 * n * D):
            raise ValueError(f"marks: need ({n * D}, 8) rows (outlines) or ({3 * n * D}, 8) (outlines and labels), got "
                             f"{mark_rows}")
        if mark_rows > MAX_MARKS:
            raise ValueError(f"marks: {mark_rows} rows; the annotator takes at most {MAX_MARKS} per call")
        R = mark_rows // (n * D)
    return S, n // S, n, D, T, R


def run_spec(R, iou_thr, new_thr, min_hits, max_age, momentum, style):
    """What Run checks of its arguments: (iou_thr, new_thr, min_hits, max_age, momentum)"""
    iou_thr, new_thr, momentum = float(iou_thr), float(new_thr), float(momentum)
    if not math.isfinite(iou_thr):
        raise ValueError(f"iou_thr must be finite, got {iou_thr}")
    if not math.isfinite(new_thr):
        raise ValueError(f"new_thr must be finite, got {new_thr}")
    if not 0.0 <= momentum <= 1.0:
        raise ValueError(f"momentum = {momentum} is outside 0..1")
    min_hits, max_age = operator.index(min_hits), operator.index(max_age)
    if min_hits < 1:
        raise ValueError(f"min_hits = {min_hits} is below 1")
    if min_hits >= 1 << 31:
        raise ValueError(f"min_hits = {min_hits} does not fit an int32")
    if not 0 <= max_age <= MAX_AGE:
        raise ValueError(f"max_age = {max_age} is outside 0..2^20")
    if R:
        if not isinstance(style, DetectionStyle):
            raise ValueError("style: a DetectionStyle is required when the batch has marks")
        if (R == 3) != (style.label_rects is not None):
            raise ValueError("style: marks of 3 * N * max_det rows need a style with label_rects, N * max_det rows one "
                             "without")
    return iou_thr, new_thr, min_hits, max_age, momentum


class TrackBatch(PreparedBatch):
    """What PyDetectionTracker.Run works on: the selector's rows, the state and the outputs, checked once
    (PyDetectionTracker.Prepare).  Owns no device memory; keeps the tensors alive."""

    def __init__(self, gpu_id: int, stream: int, dets, tracks, clock, tracked, assoc=None, marks=None, streams=1,
                 max_det=100, max_tracks=64):
        for name, t in (("dets", dets), ("tracks", tracks), ("clock", clock), ("tracked", tracked)):
            if t is None:
                raise ValueError(f"{name}: an int32 device tensor is required")
        S, F, n, D, T, R = track_spec(_rows(dets), streams, max_det, max_tracks, None if marks is None else _rows(marks))
        keep = []
        self.d_assoc = self.d_marks = 0
        for name, t, shape in (("dets", dets, (n * D, 8)), ("tracks", tracks, (S * T, 16)), ("clock", clock, (S, 4)),
                               ("tracked", tracked, (n * D, 8)), ("assoc", assoc, (n * D, 4)),
                               ("marks", marks, (R * n * D, 8))):
            if t is not None:
                ptr, _, h = device_i32(name, t, shape, gpu_id)
                setattr(self, "d_" + name, ptr)
                keep.append(h)
        if self.d_tracks % 16:
            raise ValueError("tracks: the tensor must be 16-byte aligned")
        self._begin(gpu_id, stream, None)
        self.n, self.S, self.F, self.D, self.T, self.R = n, S, F, D, T, R
        self._keep = keep
        self._style_keep = None


class PyDetectionTracker(_SurfaceTask):
    """The temporal step after PyDetectionSelector, on the GPU: its rows are associated with tracks by IoU against a
    constant-velocity prediction, and come out again with the track's id where the class was -- in one launch whatever
    the data, with nothing allocated and no synchronisation, so the call can be captured and replayed after `dets` was
    rewritten in place (vali_track_update).

    tb = Prepare(dets, tracks, clock, tracked, assoc=None, marks=None, streams=1, max_det=100, max_tracks=64): all are
    contiguous int32 GPU tensors.  `dets` (N * D, 8) are the selector's rows, D = max_det.  The N frames are `streams`
    streams of F = N / streams consecutive frames each, stream s owning frames s * F .. s * F + F - 1 in time order:
    F = 1 is N live cameras, streams = 1 one file decoded in batches.  `tracks` (streams * T, 16), 16-byte aligned, and
    `clock` (streams, 4) are THE STATE, the caller's: all zero means no tracks; every call reads and rewrites them; a
    stream is reset by zeroing its rows.  A track row is id, class, x, y, w, h, vx bits, vy bits, hits, misses, age,
    score bits, k, 0, 0, 0; a clock row next_id, frames seen, 0, 0.  `tracked` (N * D, 8) gets the dets rows of confirmed
    tracks with the TRACK ID where the class was, every other row (-1, 0, ...): it goes wherever dets goes
    (PyInstanceMasker, PyPoseDrawer, PySurfaceWarper, PyKeypointDecoder), whose colours[class % len] become a colour per
    object.  `assoc`, optional, (N * D, 4): id (tentative tracks too, 0: none), slot (-1: none), hits, class.  `marks`,
    optional, (R * N * D, 8) annotator rows as the selector writes them, with colours[id % len] and
    label_rects[id % len]: a LabelAtlas of "0" .. "99" prints the id's last two digits.
    streams 1..1024, N <= 1024, D 1..1024, N * D <= 65535, T 1..256, R * N * D <= 4096.

    Run(tb, iou_thr=0.3, new_thr=0.5, min_hits=3, max_age=30, momentum=0.5, class_agnostic=False, style=None): per
    frame, the rows in their order (score descending) each take the unmatched track of their class with the greatest IoU
    above `iou_thr` between the row and the track's predicted box; the track's velocity moves by `momentum` towards the
    step it just made.  Unmatched tracks count a miss and die after more than `max_age` of them, or at once while they
    have fewer than `min_hits` hits.  Unmatched rows with a score of at least `new_thr` start tracks in the lowest free
    slots; a row below it continues a track and starts none.  A track shows in `tracked` from its `min_hits`-th hit.
    """

    def Prepare(self, dets, tracks, clock, tracked, assoc=None, marks=None, streams=1, max_det=100,
                max_tracks=64) -> TrackBatch:
        return TrackBatch(self._gpu_id, self._stream, dets, tracks, clock, tracked, assoc, marks, streams, max_det,
                          max_tracks)

    def RunAsync(self, tb: TrackBatch, iou_thr=0.3, new_thr=0.5, min_hits=3, max_age=30, momentum=0.5,
                 class_agnostic=False, style: Optional[DetectionStyle] = None) -> Tuple[bool, TaskExecInfo]:
        if not isinstance(tb, TrackBatch):
            raise ValueError("Run: pass a TrackBatch (Prepare)")
        iou_thr, new_thr, min_hits, max_age, momentum = run_spec(tb.R, iou_thr, new_thr, min_hits, max_age, momentum, style)
        dc = nc = dl = nl = 0
        thickness, label_alpha, text_colour = 1, 0, 0
        if tb.R:
            dc, nc, dl, nl = style.device(self._gpu_id, self._stream)
            thickness, label_alpha, text_colour = style.thickness, style.label_alpha, style.text_colour
            tb._style_keep = style
        d = _status(shim.track_update((tb.S, tb.F, tb.D, tb.T), iou_thr, new_thr, momentum, min_hits, max_age,
                                      1 if class_agnostic else 0, thickness, label_alpha, text_colour, nc, nl, tb.d_dets,
                                      tb.d_tracks, tb.d_clock, tb.d_tracked, tb.d_assoc, tb.d_marks, dc, dl, self._stream))
        return d.success, d.info

    def Run(self, tb: TrackBatch, iou_thr=0.3, new_thr=0.5, min_hits=3, max_age=30, momentum=0.5, class_agnostic=False,
            style: Optional[DetectionStyle] = None) -> Tuple[bool, TaskExecInfo]:
        r = self.RunAsync(tb, iou_thr, new_thr, min_hits, max_age, momentum, class_agnostic, style)
        self._sync()
        return r
