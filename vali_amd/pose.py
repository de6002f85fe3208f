"""PyPoseDrawer: a pose head's keypoints -> points in frame pixels and skeletons drawn onto frames, on the GPU
(vali_pose_paint).

The keypoints of the selector's detections are gathered by each detection's k, mapped back through the letterbox, written
to a tensor of points and drawn in place as limbs (capsules) and joints (discs), in row order, in two launches whatever
the data: no keypoint is ever on the host.  The definition, sample for sample, is in include/vali_hip.h;
tests/pose_model.py restates it in numpy.
"""
from __future__ import annotations

import operator
from typing import Sequence, Tuple

from ._batch import PAINT_FORMATS, PreparedBatch, frames_of_one_format
from ._native import shim
from ._runargs import alpha_arg, batch_size, host_colours, kpt_thr_arg, max_det_arg, run_colours, run_rects
from .enums import TaskExecInfo
from .surface import Surface
from .tasks import _UNSUPP_CC_PAIR, _SurfaceTask, _rgb2yuv_params, _status
from .tensors import HEAD_CAI, declared_shape, device_float, device_i32, strided_layout, upload_i32

MAX_HEAD, MAX_POINTS, MAX_LIMBS, MAX_DET, MAX_WIDTH = 1 << 20, 64, 128, 1024, 64

# the 19 limbs of the 17 COCO keypoints, 0-based
COCO_SKELETON = ((15, 13), (13, 11), (16, 14), (14, 12), (11, 12), (5, 11), (6, 12), (5, 6), (5, 7), (6, 8), (7, 9),
                 (8, 10), (1, 2), (0, 1), (0, 2), (1, 3), (2, 4), (3, 5), (4, 6))


def kpts_layout(shape, strides, code, bits):
    """The rules for `kpts`, without a device: (N, K, P, 3) or (N, K, P, 2) with any element strides >= 0.  Returns
    (dtype code, shape, strides); ValueError, naming what is wrong, otherwise."""
    code, shape, strides = strided_layout("kpts", ("N", "K", "P", "3 or 2"), shape, strides, code, bits)
    n, k, p, c = shape
    batch_size(n, "kpts")
    if not 1 <= k <= MAX_HEAD:
        raise ValueError(f"kpts: K = {k} is outside 1..2^20")
    if not 1 <= p <= MAX_POINTS:
        raise ValueError(f"kpts: P = {p} is outside 1..{MAX_POINTS}")
    if c not in (2, 3):
        raise ValueError(f"kpts: the last dimension must be 3 (x, y, confidence) or 2 (x, y), got {shape}")
    return code, shape, strides


def pose_spec(n_frames, kpts_view, max_det=100, limbs=COCO_SKELETON):
    """What Prepare checks once the tensor is seen, without a device: the view is (dtype code, shape, strides) as
    kpts_layout returns it.  Returns (n, k, p, kdim, D, limbs as a flat list)."""
    _, (n, k, p, kdim), _ = kpts_view
    if n_frames != n:
        raise ValueError(f"frames: {n_frames} surfaces for a tensor of N = {n}")
    D = max_det_arg(max_det, n, MAX_DET)
    try:
        pairs = [tuple(operator.index(v) for v in pair) for pair in limbs]
    except TypeError:
        raise ValueError("limbs: a sequence of (a, b) pairs of keypoint indices") from None
    if any(len(pair) != 2 for pair in pairs):
        raise ValueError("limbs: a sequence of (a, b) pairs of keypoint indices")
    if len(pairs) > MAX_LIMBS:
        raise ValueError(f"limbs: {len(pairs)} pairs; at most {MAX_LIMBS}")
    for l, (a, b) in enumerate(pairs):
        if not (0 <= a < p and 0 <= b < p):
            raise ValueError(f"limbs: pair {l} = ({a}, {b}) is outside 0..{p - 1} (P = {p})")
    return n, k, p, kdim, D, [v for pair in pairs for v in pair]


def draw_spec(limb_colours, joint_colours, kpt_thr, thickness, diameter, alpha):
    """What Run checks of its host arguments: (host limb colours or None for a device tensor, host joint colours or None,
    kpt_thr, thickness, diameter, alpha as the C ABI takes it)"""
    thr = kpt_thr_arg(kpt_thr)
    t, d = operator.index(thickness), operator.index(diameter)
    if not 1 <= t <= MAX_WIDTH:
        raise ValueError(f"thickness = {t} is outside 1..{MAX_WIDTH}")
    if not 1 <= d <= MAX_WIDTH:
        raise ValueError(f"diameter = {d} is outside 1..{MAX_WIDTH}")
    a = alpha_arg(alpha)
    return host_colours("limb_colours", limb_colours), host_colours("joint_colours", joint_colours), thr, t, d, a


class PoseBatch(PreparedBatch):
    """What PyPoseDrawer.Run works on: the frames, the head's keypoints, the selector's dets, the limb table, the points
    and the workspace, checked and set up once (PyPoseDrawer.Prepare).  Keeps the surfaces and tensors alive."""

    _owned = ("d_frames", "d_ws", "d_rects", "d_limbs", "d_limb_colours", "d_joint_colours")

    def __init__(self, gpu_id: int, stream: int, frames: Sequence[Surface], kpts, dets, max_det=100, limbs=COCO_SKELETON,
                 points=None):
        frames = list(frames)
        fmt = frames_of_one_format("PoseBatch", frames, PAINT_FORMATS, gpu_id)
        kseen, (kcode, kshape, kstr) = device_float("kpts", kpts, kpts_layout, gpu_id, *HEAD_CAI)
        n, k, p, kdim, D, flat = pose_spec(len(frames), (kcode, kshape, kstr), max_det, limbs)
        if dets is None:
            raise ValueError(f"dets: an int32 ({n * D}, 8) device tensor is required")
        self.d_dets, _, dh = device_i32("dets", dets, (n * D, 8), gpu_id)
        self.d_points, ph = 0, None
        if points is not None:
            self.d_points, _, ph = device_i32("points", points, (n * D, p, 4), gpu_id)
            if self.d_points % 16:
                raise ValueError("points: the tensor must be 16-byte aligned")
        self._begin(gpu_id, stream, "Prepare()", frames, rects=n, colours=True)
        self.n, self.k, self.p, self.kdim, self.D, self.L = n, k, p, kdim, D, len(flat) // 2
        self.format = fmt
        self.kpts = (kseen.ptr, kcode, *kstr)
        self._keep = [frames, kseen.holder, dh, ph]
        self.ws_bytes = shim.pose_workspace_size(n, D, p)
        self.d_ws = shim.mem_alloc(gpu_id, self.ws_bytes)
        if flat:
            self.d_limbs = upload_i32(gpu_id, stream, flat)


def points_spec(n_frames, points_shape, max_det, limbs=COCO_SKELETON):
    """What PreparePoints checks, without a device: `points_shape` is the shape the tensor declares.  Returns (n, p, D,
    limbs as a flat list)."""
    batch_size(n_frames)
    if max_det is None:
        raise ValueError("max_det is required: row i * max_det + r of points is drawn on frame i")
    shape = tuple(int(v) for v in points_shape)
    if len(shape) != 3 or shape[2] != 4:
        raise ValueError(f"points: need an int32 tensor of shape (N * max_det, P, 4), got {shape}")
    p = shape[1]
    if not 1 <= p <= MAX_POINTS:
        raise ValueError(f"points: P = {p} is outside 1..{MAX_POINTS}")
    # the rules for max_det and limbs are Prepare's
    n, _, p, _, D, flat = pose_spec(n_frames, (None, (n_frames, 1, p, 3), None), max_det, limbs)
    if shape[0] != n * D:
        raise ValueError(f"points: {shape[0]} rows for N * max_det = {n} * {D} = {n * D}")
    return n, p, D, flat


class PointsBatch(PreparedBatch):
    """What PyPoseDrawer.RunPoints works on: the frames, the caller's points, the limb table and the workspace, checked
    and set up once (PyPoseDrawer.PreparePoints).  Keeps the surfaces and the tensor alive."""

    _owned = ("d_frames", "d_ws", "d_limbs", "d_limb_colours", "d_joint_colours")

    def __init__(self, gpu_id: int, stream: int, frames: Sequence[Surface], points, max_det=None, limbs=COCO_SKELETON):
        frames = list(frames)
        fmt = frames_of_one_format("PointsBatch", frames, PAINT_FORMATS, gpu_id)
        if points is None:
            raise ValueError("points: an int32 (N * max_det, P, 4) device tensor is required")
        n, p, D, flat = points_spec(len(frames), declared_shape(points), max_det, limbs)
        self.d_points, _, ph = device_i32("points", points, (n * D, p, 4), gpu_id)
        if self.d_points % 16:
            raise ValueError("points: the tensor must be 16-byte aligned")
        self._begin(gpu_id, stream, "PreparePoints()", frames, colours=True)
        self.n, self.p, self.D, self.L = n, p, D, len(flat) // 2
        self.format = fmt
        self._keep = [frames, ph]
        self.ws_bytes = shim.pose_workspace_size(n, D, p)
        self.d_ws = shim.mem_alloc(gpu_id, self.ws_bytes)
        if flat:
            self.d_limbs = upload_i32(gpu_id, stream, flat)


class PyPoseDrawer(_SurfaceTask):
    """The keypoints of a pose network (YOLOv8-pose and its relatives) for the selector's detections: mapped to frame
    pixels, written to `points` and drawn IN PLACE as skeletons onto a batch of NV12, YUV420, YUV444, RGB, BGR or
    RGB_PLANAR frames of any sizes, in two launches whatever the data, with nothing allocated and no synchronisation, so
    the call can be captured and replayed after its tensors and frames were rewritten in place (vali_pose_paint).

    pb = Prepare(frames, kpts, dets, max_det=100, limbs=COCO_SKELETON, points=None): `kpts` (N, K, P, 3) -- x, y,
    confidence in the network input's coordinates -- or (N, K, P, 2) -- every confidence 1.0 -- is a float32, float16 or
    bfloat16 GPU tensor (`__dlpack__`, or `__cuda_array_interface__` for float32 and float16) with any element strides
    >= 0: a YOLOv8-pose head (N, 4 + 1 + 3 P, K) goes in as pred[:, 5:].transpose(1, 2).unflatten(2, (P, 3)), without a
    copy.  `dets` is PyDetectionSelector's (N * max_det, 8) int32 tensor, read on the device only: row i * max_det + r
    belongs to frame i and its `k` picks the keypoints.  `limbs` is a host sequence of (a, b) keypoint pairs, uploaded
    once.  `points`, optional, is a contiguous (N * max_det, P, 4) int32 GPU tensor that every call rewrites in full:
    X, Y, the confidence's float32 bits, flag (0 invisible, 1 visible, 3 visible and inside the frame); rows of skipped
    detections are zero.  N 1..1024, K 1..2^20, P 1..64, at most 128 limbs, max_det 1..1024, N * max_det <= 65535.

    Run(pb, rects, limb_colours, joint_colours, kpt_thr=0.5, thickness=3, diameter=7, alpha=None, cc_ctx=None): `rects`
    is the (N, 8) int32 record array the frames were placed with, handled as PyDetectionSelector.Run handles it; limb l
    is drawn in limb_colours[l % len], joint p in joint_colours[p % len], packed colours (pack_colour) as host sequences,
    uploaded when they change, or int32 device tensors, at `alpha` (None: the colour's own).  A keypoint is visible when
    its confidence is above `kpt_thr`; a limb needs both of its keypoints.  `thickness` and `diameter` are 1..64 pixels.
    `cc_ctx` picks the RGB -> YUV matrix as PySurfaceAnnotator.RunBatch does.

    pb = PreparePoints(frames, points, max_det=D, limbs=COCO_SKELETON) and RunPoints(pb, limb_colours, joint_colours,
    thickness=3, diameter=7, alpha=None, cc_ctx=None) draw points the CALLER holds -- PyKeypointDecoder's, an earlier
    Run's, anything computed on the GPU -- as Run draws its own (vali_pose_paint_points, two launches): `points` is a
    contiguous, 16-byte aligned (N * max_det, P, 4) int32 GPU tensor, read only; point j of row i * max_det + r is drawn
    on frame i when its flag has bit 0 set and -65536 <= X, Y < 131072.  Every other int32 value draws nothing.
    """

    def Prepare(self, frames: Sequence[Surface], kpts, dets, max_det=100, limbs=COCO_SKELETON, points=None) -> PoseBatch:
        return PoseBatch(self._gpu_id, self._stream, frames, kpts, dets, max_det, limbs, points)

    def RunAsync(self, pb: PoseBatch, rects, limb_colours, joint_colours, kpt_thr=0.5, thickness=3, diameter=7,
                 alpha=None, cc_ctx=None) -> Tuple[bool, TaskExecInfo]:
        if not isinstance(pb, PoseBatch):
            raise ValueError("Run: pass a PoseBatch (Prepare)")
        lhost, jhost, thr, t, dia, a = draw_spec(limb_colours, joint_colours, kpt_thr, thickness, diameter, alpha)
        supported, params = _rgb2yuv_params(pb.format, cc_ctx)
        if not supported:
            return _UNSUPP_CC_PAIR
        dlc, nlc = run_colours("PyPoseDrawer", pb, "limb_colours", limb_colours, lhost, self._gpu_id, self._stream)
        djc, njc = run_colours("PyPoseDrawer", pb, "joint_colours", joint_colours, jhost, self._gpu_id, self._stream)
        d_rects = run_rects(pb, rects, self._gpu_id, self._stream)
        d = _status(shim.pose_paint(pb.descs, pb.d_frames, int(pb.format), pb.kpts, pb.kdim, pb.k, pb.p, pb.D, pb.d_limbs,
                                    pb.L, pb.d_dets, d_rects, dlc, nlc, djc, njc, thr, t, dia, a, pb.d_points, params,
                                    pb.d_ws, pb.ws_bytes, self._stream))
        return d.success, d.info

    def Run(self, pb: PoseBatch, rects, limb_colours, joint_colours, kpt_thr=0.5, thickness=3, diameter=7, alpha=None,
            cc_ctx=None) -> Tuple[bool, TaskExecInfo]:
        r = self.RunAsync(pb, rects, limb_colours, joint_colours, kpt_thr, thickness, diameter, alpha, cc_ctx)
        self._sync()
        return r

    def PreparePoints(self, frames: Sequence[Surface], points, max_det=None, limbs=COCO_SKELETON) -> PointsBatch:
        return PointsBatch(self._gpu_id, self._stream, frames, points, max_det, limbs)

    def RunPointsAsync(self, pb: PointsBatch, limb_colours, joint_colours, thickness=3, diameter=7, alpha=None,
                       cc_ctx=None) -> Tuple[bool, TaskExecInfo]:
        if not isinstance(pb, PointsBatch):
            raise ValueError("RunPoints: pass a PointsBatch (PreparePoints)")
        lhost, jhost, _, t, dia, a = draw_spec(limb_colours, joint_colours, 0.0, thickness, diameter, alpha)
        supported, params = _rgb2yuv_params(pb.format, cc_ctx)
        if not supported:
            return _UNSUPP_CC_PAIR
        dlc, nlc = run_colours("PyPoseDrawer", pb, "limb_colours", limb_colours, lhost, self._gpu_id, self._stream)
        djc, njc = run_colours("PyPoseDrawer", pb, "joint_colours", joint_colours, jhost, self._gpu_id, self._stream)
        d = _status(shim.pose_paint_points(pb.descs, pb.d_frames, int(pb.format), pb.d_points, pb.p, pb.D, pb.d_limbs,
                                           pb.L, dlc, nlc, djc, njc, t, dia, a, params, pb.d_ws, pb.ws_bytes,
                                           self._stream))
        return d.success, d.info

    def RunPoints(self, pb: PointsBatch, limb_colours, joint_colours, thickness=3, diameter=7, alpha=None,
                  cc_ctx=None) -> Tuple[bool, TaskExecInfo]:
        r = self.RunPointsAsync(pb, limb_colours, joint_colours, thickness, diameter, alpha, cc_ctx)
        self._sync()
        return r
