"""PySurfaceWarper: keypoint-aligned and rotated crops of frames, straight into a batch tensor, on the GPU
(vali_warp_fit, vali_warp_tensor).

Every slot of an (M, 3, h, w) float32, float16 or bfloat16 tensor is one affine view of one frame of a batch, sampled
bilinearly, normalised and converted in ONE launch.  The six coefficients of a slot are a row of a device tensor: the
caller's own (rotated boxes, anything computed with torch on the GPU), or fitted on the GPU in one more launch as the
similarity that takes a template -- the five ArcFace points -- onto the keypoints of the selector's detections.  No
matrix, keypoint or box is ever on the host.  The definition, sample for sample, is in include/vali_hip.h;
tests/warp_model.py restates it in numpy.
"""
from __future__ import annotations

import array
import math
import operator
from typing import Sequence, Tuple

from ._batch import PreparedBatch, surfaces_on_device
from ._native import shim
from ._runargs import batch_size, kpt_thr_arg, max_det_arg, run_rects
from .enums import PixelFormat, TaskExecInfo
from .pose import MAX_DET, kpts_layout
from .surface import Surface
from .tasks import _UNSUPP_CC_PAIR, _SurfaceTask, _csc, _nv12_variant, _pad_colour, _status, _tensor_dst
from .tensors import HEAD_CAI, device_float, device_i32

F = PixelFormat
FORMATS = (F.NV12, F.RGB, F.BGR, F.RGB_PLANAR)
MAX_SLOTS = 65535

# The five points insightface publishes for the 112 x 112 ArcFace canvas (left eye, right eye, nose, the two mouth
# corners), published in the convention where pixel centres are integers: plus 0.5 in this one, where pixel X covers
# [X, X + 1).
ARCFACE_112 = tuple((u + 0.5, v + 0.5) for u, v in ((38.2946, 51.6963), (73.5318, 51.5014), (56.0252, 71.7366),
                                                    (41.5493, 92.3655), (70.7299, 92.2041)))


def frames_spec(frames):
    """The rules for the frames, without a device: `frames` is a sequence of (format, width, height).  Returns the
    format."""
    frames = list(frames)
    batch_size(len(frames))
    fmt = frames[0][0]
    for i, (f, w, h) in enumerate(frames):
        if f not in FORMATS:
            raise ValueError(f"frames: surface {i} has format {f!r}; supported: {', '.join(v.name for v in FORMATS)}")
        if f != fmt:
            raise ValueError(f"frames: surface {i} has format {f!r}, surface 0 {fmt!r}: one format per batch")
        if f == F.NV12 and (w | h) & 1:
            raise ValueError(f"frames: surface {i}: NV12 is 4:2:0 and needs an even width and height, got {w}x{h}")
    return fmt


def matrices_spec(m_out, rows=None):
    """form (a): `out` has m_out slots (1..65535) and `matrices`, if its shape `rows` is given, as many rows of 8"""
    if not 1 <= m_out <= MAX_SLOTS:
        raise ValueError(f"out: M = {m_out} is outside 1..{MAX_SLOTS}")
    if rows is not None and tuple(rows) != (m_out, 8):
        raise ValueError(f"matrices: need an int32 tensor of shape ({m_out}, 8) for an out of M = {m_out}, got "
                         f"{tuple(rows)}")
    return m_out


def keypoints_spec(n_frames, kpts_view, m_out, max_det, template):
    """What PrepareKeypoints checks once the tensors are seen, without a device: the view is (dtype code, shape, strides) as
    pose.kpts_layout returns it.  Returns (n, k, p, kdim, D, the template as a flat list of 2 p floats)."""
    _, (n, k, p, kdim), _ = kpts_view
    if n_frames != n:
        raise ValueError(f"frames: {n_frames} surfaces for a tensor of N = {n}")
    D = max_det_arg(max_det, n, MAX_DET, cap=MAX_SLOTS, slots=("out", m_out, " detections"))
    try:
        pairs = [tuple(float(v) for v in pair) for pair in template]
    except TypeError:
        raise ValueError("template: a sequence of (u, v) pairs in canvas coordinates") from None
    if any(len(pair) != 2 for pair in pairs):
        raise ValueError("template: a sequence of (u, v) pairs in canvas coordinates")
    if len(pairs) != p:
        raise ValueError(f"template: {len(pairs)} pairs for keypoints of P = {p}")
    if p < 2:
        raise ValueError(f"kpts: P = {p}; a fit needs at least 2 keypoints")
    if any(math.isinf(v) for pair in pairs for v in pair):
        raise ValueError("template: coordinates are finite, or NaN for a keypoint that takes no part")
    return n, k, p, kdim, D, [v for pair in pairs for v in pair]


def fit_spec(kpt_thr, min_points, p):
    """What Run checks of form (b)'s host arguments: (kpt_thr, min_points)"""
    thr = kpt_thr_arg(kpt_thr)
    mp = operator.index(min_points)
    if not 2 <= mp <= p:
        raise ValueError(f"min_points = {mp} is outside 2..{p} (P = {p})")
    return thr, mp


class WarpBatch(PreparedBatch):
    """What PySurfaceWarper.Run works on: the frames, the tensor, the matrices and -- form (b) -- the keypoints, the
    detections and the template, checked and set up once (PrepareMatrices / PrepareKeypoints).  Keeps the surfaces and
    tensors alive."""

    _owned = ("d_frames", "d_ws", "d_rects", "d_template")     # d_matrices is the caller's, or d_ws under a second name

    def __init__(self, gpu_id: int, stream: int, frames: Sequence[Surface], out, matrices=None, kpts=None, dets=None,
                 max_det=None, template=None):
        frames = list(frames)
        surfaces_on_device("frames", frames, gpu_id)
        self.format = frames_spec([(d.Format, d.Width, d.Height) for d in frames])
        self.dst, self.layout, self.dtype, (m, h, w), oh = _tensor_dst(out, gpu_id)
        self.fitted = kpts is not None
        self.d_matrices, mh, kh, dh = 0, None, None, None
        if self.fitted:
            kseen, (kcode, kshape, kstr) = device_float("kpts", kpts, kpts_layout, gpu_id, *HEAD_CAI)
            n, self.k, self.p, self.kdim, self.D, flat = keypoints_spec(len(frames), (kcode, kshape, kstr), m, max_det,
                                                                         template)
            if dets is None:
                raise ValueError(f"dets: an int32 ({m}, 8) device tensor is required")
            self.d_dets, _, dh = device_i32("dets", dets, (m, 8), gpu_id)
            self.kpts, kh = (kseen.ptr, kcode, *kstr), kseen.holder
        else:
            matrices_spec(m, None)
            if matrices is None:
                raise ValueError(f"matrices: an int32 ({m}, 8) device tensor is required")
        if matrices is not None:
            self.d_matrices, _, mh = device_i32("matrices", matrices, (m, 8), gpu_id)
            if self.d_matrices % 16:
                raise ValueError("matrices: the tensor must be 16-byte aligned")
        self._begin(gpu_id, stream, "Prepare", frames, rects=len(frames) if self.fitted else 0)
        self.n, self.m, self.size = len(frames), m, (w, h)
        self.out = out
        self._keep = [frames, out, oh, mh, kh, dh]
        if self.fitted:
            buf = array.array("f", flat)
            self.d_template = shim.mem_alloc(gpu_id, 4 * len(buf))
            shim.memcpy2d_async(gpu_id, self.d_template, 4 * len(buf), buf.buffer_info()[0], 4 * len(buf), 4 * len(buf), 1,
                                0, stream)
            shim.stream_sync(gpu_id, stream)      # `buf` goes with this call
            if not self.d_matrices:               # the rows live in the batch's workspace
                self.d_ws = shim.mem_alloc(gpu_id, 32 * m)
                self.d_matrices = self.d_ws

    def __len__(self):
        return self.m


class PySurfaceWarper(_SurfaceTask):
    """Affine views of a batch of NV12, RGB, BGR or RGB_PLANAR frames (one format, any sizes, read only) as the slots of
    ONE (M, 3, h, w) float32, float16 or bfloat16 GPU tensor -- the network's input itself: bilinear with edge
    replication, then ((q / 255) / div - mean) / std as PySurfacePreprocessor normalises, with nothing allocated and no
    synchronisation, so a call can be captured and replayed after its tensors and frames were rewritten in place
    (vali_warp_tensor, vali_warp_fit).  `out` is taken exactly as PySurfacePreprocessor.PrepareTensorBatch takes it.

    wb = PrepareMatrices(frames, out, matrices): `matrices` is a contiguous int32 (M, 8) GPU tensor with rows (frame, a,
    b, c, d, e, f, status), the six middle values float32 bit patterns (torch: .view(torch.int32)): canvas position (u, v)
    -- pixel (x, y) has u = x + 0.5, v = y + 0.5 -- samples frame `frame` at (a u + b v + c, d u + e v + f), in the
    convention where pixel X covers [X, X + 1).  A row whose frame is outside 0..N-1 is skipped; `status` is ignored.
    Run(wb, pad=(0, 0, 0), cc_ctx=None) is ONE launch.

    wb = PrepareKeypoints(frames, out, kpts, dets, max_det, template=ARCFACE_112, matrices=None): `kpts` and `dets` are
    what PyPoseDrawer.Prepare takes; M = N * max_det and slot i * max_det + r belongs to that row of `dets`.  `template`
    is a host sequence of P (u, v) pairs in canvas coordinates; a pair with a NaN takes no part.  Run(wb, rects,
    kpt_thr=0.5, min_points=2, pad=(0, 0, 0), cc_ctx=None) fits, per row, the least-squares similarity that takes the
    template onto the row's visible keypoints (PyPoseDrawer's mapping and visibility rule) and samples with it: TWO
    launches.  A row PyPoseDrawer skips, one with fewer than `min_points` used keypoints or with coincident ones is
    skipped.  `matrices`, optional, receives the rows (its status: the number of keypoints used); every row is rewritten
    by every call.

    `pad` is an (R, G, B) triple, through the same normalisation, for pixels that sample nothing and for skipped slots,
    or None: nothing is written there.  `cc_ctx` picks the YUV -> RGB matrix for NV12 frames as PySurfacePreprocessor
    does; for the RGB family it is ignored.
    """

    def __init__(self, gpu_id: int, stream=None, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), div: float = 1.0):
        super().__init__(gpu_id, stream)
        self._norm = (float(div), tuple(float(v) for v in mean), tuple(float(v) for v in std))
        if len(self._norm[1]) != 3 or len(self._norm[2]) != 3:
            raise ValueError("mean / std need 3 values (R, G, B)")
        if self._norm[0] == 0.0 or any(v == 0.0 for v in self._norm[2]):
            raise ValueError("div / std must be non-zero")
        self._params_cache = {}

    def _params(self, cc_ctx):
        coeffs = _nv12_variant(cc_ctx)
        if coeffs is None:
            return None
        p = self._params_cache.get(coeffs)
        if p is None:
            div, mean, std = self._norm
            p = self._params_cache[coeffs] = shim.PreprocParams(_csc(coeffs), div, list(mean), list(std))
        return p

    def PrepareMatrices(self, frames: Sequence[Surface], out, matrices) -> WarpBatch:
        return WarpBatch(self._gpu_id, self._stream, frames, out, matrices)

    def PrepareKeypoints(self, frames: Sequence[Surface], out, kpts, dets, max_det, template=ARCFACE_112,
                         matrices=None) -> WarpBatch:
        if kpts is None:
            raise ValueError("kpts: a float32, float16 or bfloat16 (N, K, P, 3) or (N, K, P, 2) device tensor is required")
        return WarpBatch(self._gpu_id, self._stream, frames, out, matrices, kpts, dets, max_det, template)

    def RunAsync(self, wb: WarpBatch, rects=None, kpt_thr=0.5, min_points=2, pad=(0, 0, 0),
                 cc_ctx=None) -> Tuple[bool, TaskExecInfo]:
        if not isinstance(wb, WarpBatch):
            raise ValueError("Run: pass a WarpBatch (PrepareMatrices / PrepareKeypoints)")
        if wb.fitted:
            if rects is None:
                raise ValueError("rects: a batch from PrepareKeypoints needs the (N, 8) records the frames were placed with")
            thr, mp = fit_spec(kpt_thr, min_points, wb.p)
        elif rects is not None:
            raise ValueError("rects: a batch from PrepareMatrices takes none")
        try:
            on, rgb = _pad_colour(pad)
        except ValueError:
            return False, TaskExecInfo.INVALID_INPUT
        p = self._params(None if wb.format != F.NV12 else cc_ctx)
        if p is None:
            return _UNSUPP_CC_PAIR
        if wb.fitted:
            d_rects = run_rects(wb, rects, self._gpu_id, self._stream)
            d = _status(shim.warp_fit(wb.d_frames, wb.n, wb.kpts, wb.kdim, wb.k, wb.p, wb.D, mp, wb.d_template, thr,
                                      wb.d_dets, d_rects, wb.d_matrices, self._stream))
            if not d.success:
                return d.success, d.info
        d = _status(shim.warp_tensor(wb.descs, wb.d_frames, int(wb.format), wb.d_matrices, wb.dst, p, on, rgb,
                                     self._stream))
        return d.success, d.info

    def Run(self, wb: WarpBatch, rects=None, kpt_thr=0.5, min_points=2, pad=(0, 0, 0),
            cc_ctx=None) -> Tuple[bool, TaskExecInfo]:
        r = self.RunAsync(wb, rects, kpt_thr, min_points, pad, cc_ctx)
        self._sync()
        return r
