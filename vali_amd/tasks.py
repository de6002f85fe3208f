"""PySurfaceConverter / PySurfaceResizer / PySurfaceRotator / PySurfaceUD.

Host-side mirror of the reference's L3 tasks + L4 Py* wrappers: validation, format-pair
dispatch, colour-variant selection and error codes are restated here in Python; the
per-pixel work is one C-ABI call into libvali_hip.so per Run
(reference: src/TC/src/TaskConvertSurface.cpp:966-1095, src/python_vali/src/PySurfaceConverter.cpp:26-161).
"""
from __future__ import annotations

import operator
from typing import List, Optional, Sequence, Tuple

from ._batch import PAINT_FORMATS, PreparedBatch, frames_of_one_format
from ._native import shim
from ._runargs import device_rects
from .enums import (ColorRange, ColorSpace, ColorspaceConversionContext, Interpolation, PixelFormat, TaskExecDetails,
                    TaskExecInfo)
from .runtime import CudaStreamEvent, HipResMgr, is_capturing
from .surface import Surface
from .tensors import DTYPES, FLOAT_DTYPES, device_float, device_i32, is_tensor, upload_i32

F = PixelFormat

# ---- colour matrices ------------------------------------------------------------------
# The constants NVIDIA documents for the NPP functions the reference calls;
# the CSC struct layout is include/vali_hip.h:vali_csc.  (y0, cy, crv, cgu, cgv, cbu)
CSC_NPP_YUV = (0.0, 1.0, 1.140, -0.394, -0.581, 2.032)          # nppiNV12ToRGB / YUV420ToRGB / YUVToRGB
CSC_NPP_709CSC = (16.0, 1.164, 1.793, -0.213, -0.533, 2.112)    # nppiNV12ToRGB_709CSC
CSC_NPP_709HDTV = (0.0, 1.0, 1.5748, -0.1873, -0.4681, 1.8556)  # nppiNV12ToRGB_709HDTV
CSC_NPP_YCBCR = (16.0, 1.164, 1.596, -0.392, -0.813, 2.017)     # nppiYCbCr420ToRGB / YCbCrToBGR

_csc_cache = {}


def _csc(coeffs):
    c = _csc_cache.get(coeffs)
    if c is None:
        c = _csc_cache[coeffs] = shim.Csc(*coeffs)
    return c


def _status(rc: int) -> TaskExecDetails:
    """C status -> TaskExecDetails (the reference maps NppStatus the same way, e.g.
    TaskConvertSurface.cpp:151-155)."""
    if rc == 0:              # shim.OK; the shared immutable success object (hot path)
        return _S_OK
    if rc == shim.ERR_INVALID_ARG:
        return TaskExecDetails.failed(TaskExecInfo.INVALID_INPUT, shim.last_error())
    if rc == shim.ERR_UNSUPPORTED:
        return TaskExecDetails.failed(TaskExecInfo.NOT_SUPPORTED, shim.last_error())
    raise RuntimeError("HIP failure: " + shim.last_error())


_S_OK = TaskExecDetails.ok()
_OK_PAIR = (True, TaskExecInfo.SUCCESS)


def _cc_key(cc_ctx):
    """memo key of a colour context: its VALUES (the object is mutable, as in the reference)"""
    return None if cc_ctx is None else (cc_ctx.color_space, cc_ctx.color_range)
_S_INVALID = TaskExecDetails.failed(TaskExecInfo.INVALID_INPUT, "invalid src / dst")
_S_UNSUPP_CC = TaskExecDetails.failed(TaskExecInfo.UNSUPPORTED_FMT_CONV_PARAMS,
                                      "unsupported cc_ctx params")


def _nv12_variant(cc_ctx: Optional[ColorspaceConversionContext]):
    """Colour-variant switch of nv12_rgb (TaskConvertSurface.cpp:117-149):
    default BT709+JPEG; BT709: JPEG -> 709HDTV else 709CSC; BT601: JPEG -> 'YUV',
    otherwise unsupported; any other colour space unsupported."""
    space = cc_ctx.color_space if cc_ctx else ColorSpace.BT_709
    rng = cc_ctx.color_range if cc_ctx else ColorRange.JPEG
    if space == ColorSpace.BT_709:
        return CSC_NPP_709HDTV if rng == ColorRange.JPEG else CSC_NPP_709CSC
    if space == ColorSpace.BT_601 and rng == ColorRange.JPEG:
        return CSC_NPP_YUV
    return None


_MISSING = object()
_nv12_csc_cache = {}    # (color_space, color_range) | None -> shim.Csc | None (unsupported)


def _nv12_rgb(io, stream: int, cc_ctx, csc=None) -> TaskExecDetails:
    """nv12_rgb / nv12_bgr (TaskConvertSurface.cpp:61-156).  The reference's nv12_bgr
    falls off the end of the function (its return sits after `break`, :100-105); here
    BGR simply follows the RGB logic with the channel order reversed."""
    if csc is None:     # `csc` = a matrix handed in from outside (the multi-GPU broadcast)
        key = (cc_ctx.color_space, cc_ctx.color_range) if cc_ctx is not None else None
        csc = _nv12_csc_cache.get(key, _MISSING)
        if csc is _MISSING:
            coeffs = _nv12_variant(cc_ctx)
            csc = _nv12_csc_cache[key] = _csc(coeffs) if coeffs is not None else None
        if csc is None:
            return _S_UNSUPP_CC
    return _status(io.nv12_to_rgb(stream, csc))


# RGB -> YUV matrices NVIDIA documents for nppiRGBToYUV / nppiRGBToYCbCr;
# rows = (kR, kG, kB, offset) for Y, U/Cb, V/Cr.  Row 0 of the first is nppiRGBToGray.
RGB2YUV_NPP_YUV = ((0.299, 0.587, 0.114, 0.0), (-0.147, -0.289, 0.436, 128.0),
                   (0.615, -0.515, -0.100, 128.0))
RGB2YUV_NPP_YCBCR = ((0.257, 0.504, 0.098, 16.0), (-0.148, -0.291, 0.439, 128.0),
                     (0.439, -0.368, -0.071, 128.0))

_params_cache = {}


def _params(csc=None, rgb2yuv=None):
    key = (csc, rgb2yuv)
    p = _params_cache.get(key)
    if p is None:
        p = _params_cache[key] = shim.CvtParams(_csc(csc) if csc else None,
                                                [list(r) for r in rgb2yuv] if rgb2yuv else [])
    return p


_S_FAIL = TaskExecDetails.failed(TaskExecInfo.FAIL)


def _space_range(cc_ctx, space_default, range_default):
    return ((cc_ctx.color_space if cc_ctx else space_default),
            (cc_ctx.color_range if cc_ctx else range_default))


class _Single:
    """One (src, dst) pair: a C-ABI call per Run."""

    def __init__(self, src, dst):
        self.src, self.dst = src, dst
        self.last = None    # (C-ABI entry, its parameter block) of the call made: the converter's memo

    def convert(self, stream, params):
        self.last = (shim.convert, params)
        return shim.convert(self.src.desc(), self.dst.desc(), params, stream)

    def nv12_to_rgb(self, stream, csc):
        self.last = (shim.nv12_to_rgb, csc)
        return shim.nv12_to_rgb(self.src.desc(), self.dst.desc(), csc, stream)


class _Batched:
    """n pairs of one geometry: ONE launch (device descriptor arrays of a SurfaceBatch)."""

    def __init__(self, batch):
        self.b = batch

    def convert(self, stream, params):
        b = self.b
        return shim.convert_batch(b.d_src, b.d_dst, b.n, int(b.src_format), int(b.dst_format),
                                  b.src_size[0], b.src_size[1], params, stream)

    def nv12_to_rgb(self, stream, csc):
        b = self.b
        return shim.nv12_to_rgb_batch(b.d_src, b.d_dst, b.n, b.src_size[0], b.src_size[1],
                                      int(b.dst_format), csc, stream)


def _convert(io, stream, params) -> TaskExecDetails:
    return _status(io.convert(stream, params))


def _plain(io, stream, cc_ctx, csc=None):
    """Pairs without colour parameters: (de)interleave, swap, copies, element types."""
    return _convert(io, stream, _params())


def _nv12_yuv420(io, stream, cc_ctx, csc=None):
    # nv12_yuv420 (TaskConvertSurface.cpp:158-200): JPEG and MPEG pick two NPP entry points
    # that do the same byte shuffle; any other range is refused.
    _, rng = _space_range(cc_ctx, ColorSpace.BT_601, ColorRange.JPEG)
    if rng not in (ColorRange.JPEG, ColorRange.MPEG):
        return _S_UNSUPP_CC
    return _convert(io, stream, _params())


def _yuv420_rgb(io, stream, cc_ctx, csc=None):
    # yuv420_rgb / yuv420_bgr (:254-344): BT.601 only; JPEG -> "YUV", otherwise YCbCr
    space, rng = _space_range(cc_ctx, ColorSpace.BT_601, ColorRange.JPEG)
    if space != ColorSpace.BT_601:
        return _S_UNSUPP_CC
    return _convert(io, stream,
                    _params(csc=CSC_NPP_YUV if rng == ColorRange.JPEG else CSC_NPP_YCBCR))


def _yuv444_bgr(io, stream, cc_ctx, csc=None):
    # yuv444_bgr (:346-391): MPEG -> YCbCr, JPEG -> YUV, else NPP_NO_OPERATION_WARNING -> FAIL
    space, rng = _space_range(cc_ctx, ColorSpace.BT_601, ColorRange.JPEG)
    if space != ColorSpace.BT_601:
        return _S_UNSUPP_CC
    if rng == ColorRange.MPEG:
        return _convert(io, stream, _params(csc=CSC_NPP_YCBCR))
    if rng == ColorRange.JPEG:
        return _convert(io, stream, _params(csc=CSC_NPP_YUV))
    return _S_FAIL


def _yuv444_rgb(io, stream, cc_ctx, csc=None):
    # yuv444_rgb (:393-434): JPEG only
    space, rng = _space_range(cc_ctx, ColorSpace.BT_601, ColorRange.JPEG)
    if space != ColorSpace.BT_601:
        return _S_UNSUPP_CC
    if rng != ColorRange.JPEG:
        return _S_FAIL
    return _convert(io, stream, _params(csc=CSC_NPP_YUV))


def _rgb_to_yuv(io, stream, cc_ctx, csc=None):
    # bgr_yuv444 / rgb_yuv444 / rgb_planar_yuv444 / rgb_yuv420 (:481-619, :657-704):
    # BT.601 only; JPEG -> nppiRGBToYUV*, MPEG -> nppiRGBToYCbCr*, else FAIL.
    # (The reference's rgb_yuv444 + MPEG writes PACKED YCbCr into plane 0, :557-560 -- a bug;
    # here it produces planar YCbCr like the other variants.)
    space, rng = _space_range(cc_ctx, ColorSpace.BT_601, ColorRange.JPEG)
    if space != ColorSpace.BT_601:
        return _S_UNSUPP_CC
    if rng == ColorRange.JPEG:
        return _convert(io, stream, _params(rgb2yuv=RGB2YUV_NPP_YUV))
    if rng == ColorRange.MPEG:
        return _convert(io, stream, _params(rgb2yuv=RGB2YUV_NPP_YCBCR))
    return _S_FAIL


def _rgb_y(io, stream, cc_ctx, csc=None):
    # rbg8_y (:232-252): nppiRGBToGray
    return _convert(io, stream, _params(rgb2yuv=RGB2YUV_NPP_YUV))


# (src, dst) -> implementation; order is GetSupportedConversions()
# (TaskConvertSurface.cpp:966-994).  NV12 -> RGB_PLANAR is an extension: the fused form
# of the reference's NV12->RGB->RGB_PLANAR chain (BASELINE config 2).
_CONVERSIONS = {
    (F.NV12, F.YUV420): _nv12_yuv420,
    (F.YUV420, F.NV12): _plain,
    (F.P10, F.NV12): _plain,
    (F.P12, F.NV12): _plain,
    (F.NV12, F.RGB): _nv12_rgb,
    (F.NV12, F.BGR): _nv12_rgb,
    (F.RGB, F.RGB_PLANAR): _plain,
    (F.RGB_PLANAR, F.RGB): _plain,
    (F.RGB_PLANAR, F.YUV444): _rgb_to_yuv,
    (F.Y, F.YUV444): _plain,
    (F.YUV420, F.RGB): _yuv420_rgb,
    (F.RGB, F.YUV420): _rgb_to_yuv,
    (F.RGB, F.YUV444): _rgb_to_yuv,
    (F.RGB, F.BGR): _plain,
    (F.BGR, F.RGB): _plain,
    (F.YUV420, F.BGR): _yuv420_rgb,
    (F.YUV444, F.BGR): _yuv444_bgr,
    (F.YUV444, F.RGB): _yuv444_rgb,
    (F.BGR, F.YUV444): _rgb_to_yuv,
    (F.NV12, F.Y): _plain,
    (F.RGB, F.RGB_32F): _plain,
    (F.RGB, F.Y): _rgb_y,
    (F.RGB_32F, F.RGB_32F_PLANAR): _plain,
    (F.NV12, F.RGB_PLANAR): _nv12_rgb,
}


class _SurfaceTask:
    def __init__(self, gpu_id: int, stream=None):
        self._gpu_id = int(gpu_id)
        # stream=None: this GPU's stream from the resource manager (the reference's one-argument constructors,
        # CudaResMgr::GetStream).  An explicit stream is used as handed over (PySurfaceConverter.cpp:33-45) -- also 0,
        # the legacy default stream: torch.cuda.current_stream().cuda_stream is 0 for torch's default stream, and a
        # caller who passes it expects the task to be ordered with their own work there.  A null hipStream_t carries no
        # device, so such a task makes its GPU current on the calling thread before every call (_bind_null_stream).
        self._stream = HipResMgr.Instance().GetStream(self._gpu_id) if stream is None else int(stream)
        if self._stream == 0:
            self._bind_null_stream()
        self._event = CudaStreamEvent(self._stream, self._gpu_id)
        # Memo of recent successful single-surface calls: (src descriptor, dst descriptor, extra
        # key...) -> (C-ABI entry, arguments between the descriptors and the stream).
        # A repeated RunAsync on the same surfaces (the per-frame loop of every sample pipeline,
        # one entry per step of its chain; BASELINE config 2) then costs one C call instead of the
        # task's Python dispatch: 1 - 2.5 us less per call (4.95 -> 3.9 us for the converter, the
        # host's own launch rate).  The memo keeps the (pointer-only) descriptors alive, not the
        # surfaces; a Surface gets a NEW descriptor object when it is re-pointed (Surface._update)
        # and a new Surface has its own, so a stale entry can never match.
        self._memo = {}
        self._batches = {}    # (src descriptors, dst descriptors) -> SurfaceBatch, see _batch_of

    def _bind_null_stream(self):
        """Tasks on the null stream: a null hipStream_t carries no device, so every Run* / PrepareBatch makes the task's
        GPU the thread's current device for the duration of the call and puts the caller's device BACK afterwards (the
        reference's CudaCtxPush / pop, CudaUtils.hpp:77-90): a host application that runs a task on (gpu 1, stream 0)
        keeps allocating on the device it had selected.  Done by wrapping the methods of THIS instance, so tasks on real
        streams -- whose device the library reads off the stream -- keep their call path untouched; the wrappers hold a
        weak reference to the task (no self-referencing cycle: the task's events and memo go when its last user does)."""
        import inspect
        import weakref

        gpu, ref = self._gpu_id, weakref.ref(self)
        for name in dir(type(self)):
            if name.startswith("Run") or name == "PrepareBatch":
                # (getattr_static: the raw class attribute -- getattr resolves descriptors, so a static Run* helper would
                # look like a plain function here and be called with an extra `me`)
                if isinstance(inspect.getattr_static(type(self), name), (staticmethod, classmethod)):
                    continue
                unbound = getattr(type(self), name)
                if not callable(unbound):
                    continue

                def call(*a, _fn=unbound, _name=name, **k):
                    me = ref()
                    if me is None:     # a bound method kept (`f = task.Run`) after the task itself was dropped
                        raise ReferenceError(f"{_name}: the task this method belonged to no longer exists")
                    prev = shim.device_get()
                    if prev != gpu:
                        shim.device_set(gpu)
                    try:
                        return _fn(me, *a, **k)
                    finally:
                        if prev != gpu and prev >= 0:
                            shim.device_set(prev)
                setattr(self, name, call)

    def _batch_of(self, batch, dsts):
        """RunBatch*(srcs, dsts): the descriptor arrays of a (srcs, dsts) pair of lists are uploaded ONCE and
        kept with the task (8 most recent pairs) -- a repeated call costs no allocation, no copy and no
        synchronisation, and the arrays outlive every launch that reads them.  RunBatch*(batch) passes a
        prepared SurfaceBatch through."""
        if isinstance(batch, SurfaceBatch):
            return batch
        if dsts is None:
            raise ValueError("RunBatch: pass a SurfaceBatch, or two lists (srcs, dsts)")
        srcs, dsts = list(batch), list(dsts)
        key = (tuple(s.desc() for s in srcs), tuple(d.desc() for d in dsts))
        b = self._batches.pop(key, None)
        if b is None:
            # a miss while the stream is capturing must fail BEFORE anything is evicted: dropping a cached batch
            # synchronises its stream (SurfaceBatch.__del__), which would invalidate the capture instead of reporting it
            if is_capturing(self._gpu_id, self._stream):
                raise RuntimeError("RunBatch(srcs, dsts): these lists have no prepared batch and one cannot be created "
                                   "while the stream is capturing -- call PrepareBatch() before the capture")
            b = SurfaceBatch(self._gpu_id, self._stream, srcs, dsts)
            # the cache must not pin the caller's surfaces (a task fed fresh lists of 512 2160p frames would hold
            # 8 x 19 GB): it keeps the descriptor arrays only; a hit needs the SAME descriptor objects, i.e. live
            # surfaces that were not re-pointed, and a freed surface's descriptors can never match a new one's
            b._keep = None
            while len(self._batches) >= 8:                     # least recently used first (a hit re-inserts below)
                self._batches.pop(next(iter(self._batches)))
        self._batches[key] = b
        return b

    def _memo_put(self, key, fn, args, keep=None):
        if len(self._memo) >= 16:
            self._memo.clear()
        self._memo[key] = (fn, args, keep)

    @property
    def Stream(self) -> int:
        return self._stream

    def _sync(self):
        # the blocking Run* forms: everything issued on the task's stream has finished.  vali_stream_wait = a completion
        # word the stream writes into pinned host memory, spun on with the GIL released: 8.7 us around a 1 us kernel
        # against 11.8-12.6 us for hipStreamSynchronize (an event record + hipEventSynchronize: the same or worse;
        # interrupts off / ROC_ACTIVE_WAIT_TIMEOUT: no change) -- tools/exp/sync_latency.hip; the launch -> completion
        # round trip of a kernel that announces its own end is 8.15 us on the same box, so that is the floor.
        shim.stream_wait(self._gpu_id, self._stream)


class PySurfaceConverter(_SurfaceTask):
    """GPU colour-space / pixel-format conversion.

    reference: src/python_vali/src/PySurfaceConverter.cpp:26-161 (ctor, Run, RunAsync,
    Conversions, Stream); dispatch ConvertSurface::Run (TaskConvertSurface.cpp:1009-1095).
    RunBatch is new: one launch over a list of same-shaped surfaces.
    """

    def __init__(self, gpu_id: int, stream=None):
        super().__init__(gpu_id, stream)
        self._batch_cache = {}

    @staticmethod
    def Conversions() -> List[Tuple[PixelFormat, PixelFormat]]:
        return list(_CONVERSIONS.keys())

    def _run(self, src: Surface, dst: Surface, cc_ctx) -> TaskExecDetails:
        if src.Width != dst.Width or src.Height != dst.Height:   # Validate(), :1001-1015
            return _S_INVALID
        impl = _CONVERSIONS.get((src.Format, dst.Format))
        if impl is None:                                          # :1085-1089
            raise ValueError(f"Unsupported pixel format conversion: {src.Format.name} -> "
                             f"{dst.Format.name}")
        io = _Single(src, dst)
        d = impl(io, self._stream, cc_ctx)
        if d is _S_OK and io.last is not None:
            self._memo_put((src.desc(), dst.desc(), _cc_key(cc_ctx)), io.last[0], (io.last[1],))
        return d

    def RunAsync(self, src: Surface, dst: Surface,
                 cc_ctx: Optional[ColorspaceConversionContext] = None) -> Tuple[bool, TaskExecInfo]:
        try:
            d1, d2 = src._desc, dst._desc
            m = self._memo.get((d1, d2, None if cc_ctx is None else (cc_ctx.color_space, cc_ctx.color_range)))
        except (AttributeError, TypeError):     # not Surfaces: let the dispatch below complain
            m = None
        if m is not None and m[0](d1, d2, *m[1], self._stream) == 0:
            return _OK_PAIR
        d = self._run(src, dst, cc_ctx)
        return d.success, d.info

    def Run(self, src: Surface, dst: Surface,
            cc_ctx: Optional[ColorspaceConversionContext] = None) -> Tuple[bool, TaskExecInfo]:
        r = self.RunAsync(src, dst, cc_ctx)     # (the memoised C call when the pair repeats)
        self._sync()
        return r

    # -- batched form ------------------------------------------------------------------
    def PrepareBatch(self, srcs: Sequence[Surface], dsts: Sequence[Surface]) -> "SurfaceBatch":
        """Upload the descriptor arrays of a (srcs, dsts) batch once; reuse with RunBatch."""
        return SurfaceBatch(self._gpu_id, self._stream, srcs, dsts)

    def RunBatchAsync(self, batch, dsts=None, cc_ctx=None, csc=None) -> Tuple[bool, TaskExecInfo]:
        """RunBatchAsync(batch, cc_ctx=...) or RunBatchAsync(srcs, dsts, cc_ctx).
        All-or-nothing, no per-item sync (idiom of PyNvJpegEncoder.Run,
        src/python_vali/src/PyNvJpegEncoder.cpp:31-81).  `csc` overrides the matrix
        cc_ctx would select (the multi-GPU pipeline passes the broadcast block)."""
        batch = self._batch_of(batch, dsts)
        impl = _CONVERSIONS.get((batch.src_format, batch.dst_format))
        if impl is None:
            raise ValueError(f"Unsupported pixel format conversion: {batch.src_format.name} -> "
                             f"{batch.dst_format.name}")
        if batch.src_size != batch.dst_size:
            return False, TaskExecInfo.INVALID_INPUT
        d = impl(_Batched(batch), self._stream, cc_ctx, csc)
        return d.success, d.info

    def RunBatch(self, batch, dsts=None, cc_ctx=None, csc=None) -> Tuple[bool, TaskExecInfo]:
        r = self.RunBatchAsync(batch, dsts, cc_ctx, csc)
        self._sync()
        return r


class SurfaceBatch(PreparedBatch):
    """Device-resident descriptor arrays for n (src, dst) surface pairs of one geometry."""

    _owned = ("d_src", "d_dst")

    def __init__(self, gpu_id: int, stream: int, srcs: Sequence[Surface], dsts: Sequence[Surface]):
        srcs, dsts = list(srcs), list(dsts)
        if not srcs or len(srcs) != len(dsts):
            raise ValueError("SurfaceBatch: need equally long, non-empty src and dst lists")
        for group in (srcs, dsts):
            f0, s0 = group[0].Format, (group[0].Width, group[0].Height)
            for s in group:
                if s.Format != f0 or (s.Width, s.Height) != s0 or s.IsEmpty:
                    raise ValueError("SurfaceBatch: surfaces of a batch must share format and size")
        self._begin(gpu_id, stream, "PrepareBatch()")
        self.n = len(srcs)
        self.src_format, self.dst_format = srcs[0].Format, dsts[0].Format
        self.src_size = (srcs[0].Width, srcs[0].Height)
        self.dst_size = (dsts[0].Width, dsts[0].Height)
        self._keep = (srcs, dsts)        # a prepared batch keeps its surfaces alive (the task's own cache does not)
        self.src_components, self.src_planes = srcs[0].NumComponents, srcs[0].NumPlanes
        self.d_src = shim.descs_upload(gpu_id, [s.desc() for s in srcs], stream)
        self.d_dst = shim.descs_upload(gpu_id, [s.desc() for s in dsts], stream)


# ---- PySurfaceUD -------------------------------------------------------------------------
# UDSurface::SupportedConversions() (src/TC/src/UDSurface.cpp:117-133).  The planar-source
# rows (YUV420 -> YUV444, YUV420_10bit -> YUV444_10bit) go through NPP Lanczos in the
# reference (UDPlanar, :33-93): here vali_ud_planar, all three planes in one launch, Lanczos-3.
_UD_CONVERSIONS = [
    (F.NV12, F.YUV444), (F.NV12, F.RGB), (F.NV12, F.RGB_32F), (F.NV12, F.RGB_PLANAR),
    (F.NV12, F.RGB_32F_PLANAR), (F.YUV420, F.YUV444), (F.P10, F.YUV444_10bit), (F.P10, F.RGB_32F),
    (F.P10, F.RGB_32F_PLANAR), (F.YUV420_10bit, F.YUV444_10bit),
]
_UD_SEMIPLANAR = {p for p in _UD_CONVERSIONS if p[0] in (F.NV12, F.P10)}


class PySurfaceUD(_SurfaceTask):
    """Chroma upsample + resize (+ YUV->RGB) in one pass.

    reference: src/python_vali/src/PySurfaceUD.cpp:26-143 (ctor, Run, RunAsync,
    SupportedFormats, Stream); UDSurface::Run (src/TC/src/UDSurface.cpp:135-177).
    As in the reference the dst size alone defines the scale (no size validation).
    """

    @staticmethod
    def SupportedFormats() -> List[Tuple[PixelFormat, PixelFormat]]:
        return list(_UD_CONVERSIONS)

    def _run(self, src: Surface, dst: Surface) -> TaskExecDetails:
        pair = (src.Format, dst.Format)
        if pair not in _UD_CONVERSIONS:                       # UDSurface.cpp:137-149
            return TaskExecDetails.failed(TaskExecInfo.NOT_SUPPORTED)
        if pair not in _UD_SEMIPLANAR:
            # UDPlanar (UDSurface.cpp:33-93): every source plane resized to the matching destination plane
            # with NPPI_INTER_LANCZOS -- one launch over the three planes
            d = _status(shim.ud_planar(src.desc(), dst.desc(), shim.INTERP_LANCZOS, self._stream))
            if d is _S_OK:
                self._memo_put((src.desc(), dst.desc()), shim.ud_planar, (shim.INTERP_LANCZOS,))
            return d
        d = _status(shim.ud_nv12(src.desc(), dst.desc(), self._stream))
        if d is _S_OK:
            self._memo_put((src.desc(), dst.desc()), shim.ud_nv12, ())
        return d

    def RunAsync(self, src: Surface, dst: Surface) -> Tuple[bool, TaskExecInfo]:
        try:
            d1, d2 = src._desc, dst._desc
            m = self._memo.get((d1, d2))
        except (AttributeError, TypeError):
            m = None
        if m is not None and m[0](d1, d2, *m[1], self._stream) == 0:
            return _OK_PAIR
        d = self._run(src, dst)
        return d.success, d.info

    def Run(self, src: Surface, dst: Surface) -> Tuple[bool, TaskExecInfo]:
        r = self.RunAsync(src, dst)
        self._sync()
        return r

    # -- fused UD + quarter-turn rotation (new; BASELINE config 4 as ONE pass) ----------------
    @staticmethod
    def _quarter(angle: float):
        """90 / 180 / 270 (any sign / multiple of 360) -> 1 / 2 / 3; None otherwise."""
        q = float(angle) / 90.0
        return int(round(q)) % 4 if abs(q - round(q)) < 1e-9 and int(round(q)) % 4 else None

    def RunRotatedAsync(self, src: Surface, dst: Surface, angle: float) -> Tuple[bool, TaskExecInfo]:
        """UD with the result written rotated by `angle` (a non-zero multiple of 90 degrees):
        bit-identical to `Run(src, tmp)` + `PySurfaceRotator.Run(tmp, dst, angle)` without the
        intermediate surface.  NV12 -> RGB only; for 90 / 270 `dst` is (UD height) x (UD width)."""
        q = self._quarter(angle)
        if q is None or (src.Format, dst.Format) != (F.NV12, F.RGB):
            return False, TaskExecInfo.NOT_SUPPORTED
        d = _status(shim.ud_nv12_rot(src.desc(), dst.desc(), q, self._stream))
        return d.success, d.info

    def RunRotated(self, src: Surface, dst: Surface, angle: float) -> Tuple[bool, TaskExecInfo]:
        r = self.RunRotatedAsync(src, dst, angle)
        self._sync()
        return r

    def RunRotatedBatchAsync(self, batch, dsts=None, angle: float = 90.0) -> Tuple[bool, TaskExecInfo]:
        batch = self._batch_of(batch, dsts)
        q = self._quarter(angle)
        if q is None or (batch.src_format, batch.dst_format) != (F.NV12, F.RGB):
            return False, TaskExecInfo.NOT_SUPPORTED
        if (batch.src_size[0] | batch.src_size[1]) & 1:       # the one rule for 4:2:0 sizes (include/vali_hip.h)
            return False, TaskExecInfo.INVALID_INPUT
        d = _status(shim.ud_nv12_rot_batch(batch.d_src, batch.d_dst, batch.n, int(batch.src_format),
                                           batch.src_size[0], batch.src_size[1], batch.dst_size[0], batch.dst_size[1],
                                           int(batch.dst_format), q, self._stream))
        return d.success, d.info

    def RunRotatedBatch(self, batch, dsts=None, angle: float = 90.0) -> Tuple[bool, TaskExecInfo]:
        r = self.RunRotatedBatchAsync(batch, dsts, angle)
        self._sync()
        return r

    def RunBatchAsync(self, batch, dsts=None) -> Tuple[bool, TaskExecInfo]:
        batch = self._batch_of(batch, dsts)
        if (batch.src_format, batch.dst_format) not in _UD_CONVERSIONS:
            return False, TaskExecInfo.NOT_SUPPORTED
        if (batch.src_size[0] | batch.src_size[1]) & 1:       # every UD source is 4:2:0: even sizes (include/vali_hip.h)
            return False, TaskExecInfo.INVALID_INPUT
        if (batch.src_format, batch.dst_format) not in _UD_SEMIPLANAR:
            d = _status(shim.ud_planar_batch(batch.d_src, batch.d_dst, batch.n, int(batch.src_format),
                                             int(batch.dst_format), batch.src_size[0], batch.src_size[1],
                                             batch.dst_size[0], batch.dst_size[1], shim.INTERP_LANCZOS, self._stream))
            return d.success, d.info
        d = _status(shim.ud_nv12_batch(batch.d_src, batch.d_dst, batch.n, int(batch.src_format),
                                       batch.src_size[0], batch.src_size[1], batch.dst_size[0], batch.dst_size[1],
                                       int(batch.dst_format), self._stream))
        return d.success, d.info

    def RunBatch(self, batch, dsts=None) -> Tuple[bool, TaskExecInfo]:
        r = self.RunBatchAsync(batch, dsts)
        self._sync()
        return r

    def PrepareBatch(self, srcs: Sequence[Surface], dsts: Sequence[Surface]) -> "SurfaceBatch":
        return SurfaceBatch(self._gpu_id, self._stream, srcs, dsts)


# ---- PySurfacePreprocessor (new: fused inference pre-processing) -------------
class PySurfacePreprocessor(_SurfaceTask):
    """NV12, RGB, BGR or RGB_PLANAR -> (bilinear resize to dst size) -> RGB -> float -> normalised, ONE launch.

    The reference has no such task: its samples and tests/test_TorchSegmentation.py:176-240
    chain PySurfaceConverter NV12->RGB, RGB->RGB_32F, RGB_32F->RGB_32F_PLANAR and then run
    `torch.divide(x, 255.0)` + torchvision `Normalize(mean, std)` (optionally after a
    PySurfaceResizer).  This task is DEFINED as that chain and is bit-identical to running
    it with this library's own tasks (tests/test_gpu_preproc.py):

        out[c] = ((rgb_u8[c] / 255.0) / div - mean[c]) / std[c]          float32, IEEE

    `div=1, mean=0, std=1` is plain NV12 -> RGB_32F[_PLANAR].  Colour variant selection is
    nv12_rgb's (TaskConvertSurface.cpp:117-149).  dst: RGB_32F_PLANAR or RGB_32F.
    8-bit destinations (RGB, BGR, RGB_PLANAR) give the fused PySurfaceResizer ->
    PySurfaceConverter chain (resize + colour conversion, no float stage); they require the
    identity normalisation.

    RGB, BGR and RGB_PLANAR sources (what PyNvJpegDecoder gives for files that are not 4:2:0 of even size) take the
    chain PySurfaceResizer(fmt, LINEAR) -> PySurfaceConverter to the destination's layout -> the same normalisation,
    with the channels named by colour whatever the memory order (vali_rgb_preproc_roi, include/vali_hip.h).  There is
    no colour matrix for them: `cc_ctx` is accepted and ignored.  Nothing about them needs to be even: sizes, crops
    and placements are any integers, a rectangle is at least 1 x 1.
    """

    _RGB_SRC = (F.RGB, F.BGR, F.RGB_PLANAR)
    _DST = (F.RGB_32F_PLANAR, F.RGB_32F, F.RGB, F.BGR, F.RGB_PLANAR)

    @staticmethod
    def SupportedFormats() -> List[Tuple[PixelFormat, PixelFormat]]:
        """every (source, destination) pair the task runs"""
        return [(s, d) for s in (F.NV12,) + PySurfacePreprocessor._RGB_SRC for d in PySurfacePreprocessor._DST]

    def __init__(self, gpu_id: int, stream=None, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0),
                 div: float = 1.0):
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

    @staticmethod
    def _check(src_fmt, dst_fmt, sw, sh, dw, dh):
        if dst_fmt not in PySurfacePreprocessor._DST:
            return TaskExecDetails.failed(TaskExecInfo.NOT_SUPPORTED)
        if src_fmt in PySurfacePreprocessor._RGB_SRC:
            return None
        if src_fmt != F.NV12:
            return TaskExecDetails.failed(TaskExecInfo.NOT_SUPPORTED)
        if (sw | sh | dw | dh) & 1:
            return _S_INVALID
        return None

    def _u8_needs_identity(self, dst_fmt) -> bool:
        """8-bit destinations carry no float stage: a non-identity normalisation cannot apply."""
        return dst_fmt in (F.RGB, F.BGR, F.RGB_PLANAR) and self._norm != (1.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))

    def _run(self, src: Surface, dst: Surface, cc_ctx) -> TaskExecDetails:
        if src is None or dst is None or src.IsEmpty or dst.IsEmpty:
            return _S_INVALID
        bad = self._check(src.Format, dst.Format, src.Width, src.Height, dst.Width, dst.Height)
        if bad:
            return bad
        if self._u8_needs_identity(dst.Format):
            return TaskExecDetails.failed(TaskExecInfo.NOT_SUPPORTED)
        if src.Format in self._RGB_SRC:    # the region kernel with whole rectangles; no colour matrix
            args = ((0, 0, src.Width, src.Height, 0, 0, dst.Width, dst.Height), self._params(None), False, (0, 0, 0))
            d = _status(shim.rgb_preproc_roi(src.desc(), dst.desc(), *args, self._stream))
            if d is _S_OK:
                self._memo_put((src.desc(), dst.desc(), _cc_key(cc_ctx)), shim.rgb_preproc_roi, args)
            return d
        p = self._params(cc_ctx)
        if p is None:
            return _S_UNSUPP_CC
        d = _status(shim.nv12_preproc(src.desc(), dst.desc(), p, self._stream))
        if d is _S_OK:
            self._memo_put((src.desc(), dst.desc(), _cc_key(cc_ctx)), shim.nv12_preproc, (p,))
        return d

    def RunAsync(self, src: Surface, dst: Surface, cc_ctx=None) -> Tuple[bool, TaskExecInfo]:
        try:
            d1, d2 = src._desc, dst._desc
            m = self._memo.get((d1, d2, None if cc_ctx is None else (cc_ctx.color_space, cc_ctx.color_range)))
        except (AttributeError, TypeError):
            m = None
        if m is not None and m[0](d1, d2, *m[1], self._stream) == 0:
            return _OK_PAIR
        d = self._run(src, dst, cc_ctx)
        return d.success, d.info

    def Run(self, src: Surface, dst: Surface, cc_ctx=None) -> Tuple[bool, TaskExecInfo]:
        r = self.RunAsync(src, dst, cc_ctx)
        self._sync()
        return r

    def PrepareBatch(self, srcs: Sequence[Surface], dsts: Sequence[Surface]) -> "SurfaceBatch":
        return SurfaceBatch(self._gpu_id, self._stream, srcs, dsts)

    def RunBatchAsync(self, batch, dsts=None, cc_ctx=None) -> Tuple[bool, TaskExecInfo]:
        batch = self._batch_of(batch, dsts)
        bad = self._check(batch.src_format, batch.dst_format, *batch.src_size, *batch.dst_size)
        if bad:
            return bad.success, bad.info
        if self._u8_needs_identity(batch.dst_format):
            return False, TaskExecInfo.NOT_SUPPORTED
        if batch.src_format in self._RGB_SRC:    # no rectangle records: whole surfaces
            d = _status(shim.rgb_preproc_roi_batch(batch.d_src, batch.d_dst, 0, batch.n, int(batch.src_format),
                                                   batch.dst_size[0], batch.dst_size[1], int(batch.dst_format),
                                                   self._params(None), False, (0, 0, 0), self._stream))
            return d.success, d.info
        p = self._params(cc_ctx)
        if p is None:
            return False, TaskExecInfo.UNSUPPORTED_FMT_CONV_PARAMS
        d = _status(shim.nv12_preproc_batch(batch.d_src, batch.d_dst, batch.n, batch.src_size[0],
                                            batch.src_size[1], batch.dst_size[0], batch.dst_size[1],
                                            int(batch.dst_format), p, self._stream))
        return d.success, d.info

    def RunBatch(self, batch, dsts=None, cc_ctx=None) -> Tuple[bool, TaskExecInfo]:
        r = self.RunBatchAsync(batch, dsts, cc_ctx)
        self._sync()
        return r

    # ---- regions: crop / letterbox / mosaic (vali_nv12_preproc_roi[_batch]) ----
    # src_rect = (x, y, w, h) in source luma pixels, dst_rect in destination pixels, all even for NV12 sources (any
    # integers, at least 1 x 1, for RGB, BGR and RGB_PLANAR sources); None = the whole
    # surface.  Inside dst_rect the result is exactly Run(view of src_rect, view of dst_rect); outside it the pad
    # colour (R, G, B) in u8 through the same normalisation, or -- pad=None -- nothing is written.
    def RunRoiAsync(self, src: Surface, dst: Surface, src_rect=None, dst_rect=None, pad=None,
                    cc_ctx=None) -> Tuple[bool, TaskExecInfo]:
        if src is None or dst is None or src.IsEmpty or dst.IsEmpty:
            return False, TaskExecInfo.INVALID_INPUT
        bad = self._check(src.Format, dst.Format, src.Width, src.Height, dst.Width, dst.Height)
        if bad:
            return bad.success, bad.info
        if self._u8_needs_identity(dst.Format):
            return False, TaskExecInfo.NOT_SUPPORTED
        is_rgb = src.Format in self._RGB_SRC
        try:
            roi = _roi_record(src_rect, dst_rect, (src.Width, src.Height), (dst.Width, dst.Height), even=not is_rgb)
            on, rgb = _pad_colour(pad)
        except ValueError:
            return False, TaskExecInfo.INVALID_INPUT
        if is_rgb:
            d = _status(shim.rgb_preproc_roi(src.desc(), dst.desc(), roi, self._params(None), on, rgb, self._stream))
            return d.success, d.info
        p = self._params(cc_ctx)
        if p is None:
            return False, TaskExecInfo.UNSUPPORTED_FMT_CONV_PARAMS
        d = _status(shim.nv12_preproc_roi(src.desc(), dst.desc(), roi, p, on, rgb, self._stream))
        return d.success, d.info

    def RunRoi(self, src: Surface, dst: Surface, src_rect=None, dst_rect=None, pad=None,
               cc_ctx=None) -> Tuple[bool, TaskExecInfo]:
        r = self.RunRoiAsync(src, dst, src_rect, dst_rect, pad, cc_ctx)
        self._sync()
        return r

    def PrepareRoiBatch(self, srcs: Sequence[Surface], dsts: Sequence[Surface], src_rects=None,
                        dst_rects=None) -> "RoiBatch":
        return RoiBatch(self._gpu_id, self._stream, srcs, dsts, src_rects, dst_rects)

    def RunRoiBatchAsync(self, batch: "RoiBatch", pad=None, cc_ctx=None, rects=None) -> Tuple[bool, TaskExecInfo]:
        """One launch over the items of `batch`.  `rects`: a contiguous device int32 tensor of shape (n, 8) on the
        batch's GPU (__cuda_array_interface__ or DLPack) that replaces the batch's rectangles for this call -- read
        by the kernel, never by the host (detector output: no synchronisation).  Such rectangles are sanitised on the
        device (include/vali_hip.h); the tensor must stay alive until the launch has run."""
        if not isinstance(batch, RoiBatch):
            raise ValueError("RunRoiBatch: pass a RoiBatch (PrepareRoiBatch)")
        is_rgb = batch.src_format in self._RGB_SRC
        if (batch.src_format != F.NV12 and not is_rgb) or batch.dst_format not in self._DST:
            return False, TaskExecInfo.NOT_SUPPORTED
        if self._u8_needs_identity(batch.dst_format):
            return False, TaskExecInfo.NOT_SUPPORTED
        try:
            on, rgb = _pad_colour(pad)
        except ValueError:
            return False, TaskExecInfo.INVALID_INPUT
        p = self._params(None if is_rgb else cc_ctx)
        if p is None:
            return False, TaskExecInfo.UNSUPPORTED_FMT_CONV_PARAMS
        d_roi, _hold = (batch.d_roi, None) if rects is None else device_rects(rects, batch.n, batch.gpu_id)
        if is_rgb:
            d = _status(shim.rgb_preproc_roi_batch(batch.d_src, batch.d_dst, d_roi, batch.n, int(batch.src_format),
                                                   batch.dst_size[0], batch.dst_size[1], int(batch.dst_format), p, on,
                                                   rgb, self._stream))
            return d.success, d.info
        d = _status(shim.nv12_preproc_roi_batch(batch.d_src, batch.d_dst, d_roi, batch.n, batch.dst_size[0],
                                                batch.dst_size[1], int(batch.dst_format), p, on, rgb, self._stream))
        return d.success, d.info

    def RunRoiBatch(self, batch: "RoiBatch", pad=None, cc_ctx=None, rects=None) -> Tuple[bool, TaskExecInfo]:
        r = self.RunRoiBatchAsync(batch, pad, cc_ctx, rects)
        self._sync()
        return r

    # ---- regions into ONE batch tensor (vali_nv12_preproc_roi_tensor / vali_rgb_preproc_roi_tensor) ----
    # `out`: a float32, float16 or bfloat16 device tensor of logical shape (N, 3, H, W), handed over by DLPack (or
    # __cuda_array_interface__), contiguous, a slice that keeps rows contiguous, or channels last.  out[i, c, y, x] is the
    # float32 that RunRoiBatch writes to an RGB_32F_PLANAR canvas of H x W, converted to out's dtype round-to-nearest-
    # even: no surfaces, no torch.stack, no .half().
    def PrepareTensorBatch(self, srcs: Sequence[Surface], out, src_rects=None, dst_rects=None) -> "TensorBatch":
        return TensorBatch(self._gpu_id, self._stream, srcs, out, src_rects, dst_rects)

    def RunTensorBatchAsync(self, batch: "TensorBatch", pad=None, cc_ctx=None, rects=None) -> Tuple[bool, TaskExecInfo]:
        """One launch over the items of `batch`; `pad`, `cc_ctx` and `rects` as for RunRoiBatchAsync."""
        if not isinstance(batch, TensorBatch):
            raise ValueError("RunTensorBatch: pass a TensorBatch (PrepareTensorBatch)")
        is_rgb = batch.src_format in self._RGB_SRC
        if batch.src_format != F.NV12 and not is_rgb:
            return False, TaskExecInfo.NOT_SUPPORTED
        try:
            on, rgb = _pad_colour(pad)
        except ValueError:
            return False, TaskExecInfo.INVALID_INPUT
        p = self._params(None if is_rgb else cc_ctx)
        if p is None:
            return False, TaskExecInfo.UNSUPPORTED_FMT_CONV_PARAMS
        d_roi, _hold = (batch.d_roi, None) if rects is None else device_rects(rects, batch.n, batch.gpu_id)
        if is_rgb:
            d = _status(shim.rgb_preproc_roi_tensor(batch.d_src, d_roi, int(batch.src_format), batch.dst, p, on, rgb,
                                                    self._stream))
        else:
            d = _status(shim.nv12_preproc_roi_tensor(batch.d_src, d_roi, batch.dst, p, on, rgb, self._stream))
        return d.success, d.info

    def RunTensorBatch(self, batch: "TensorBatch", pad=None, cc_ctx=None, rects=None) -> Tuple[bool, TaskExecInfo]:
        r = self.RunTensorBatchAsync(batch, pad, cc_ctx, rects)
        self._sync()
        return r


def letterbox_rect(src_w: int, src_h: int, dst_w: int, dst_h: int) -> Tuple[int, int, int, int]:
    """The centred, aspect-preserving, even placement (x, y, w, h) of a src_w x src_h picture inside a
    dst_w x dst_h canvas: s = min(dst_w / src_w, dst_h / src_h); w = min(dst_w, 2 * round(src_w * s / 2)) (h likewise);
    x = ((dst_w - w) // 4) * 2 (y likewise).  1920 x 1080 -> 640 x 640 gives (0, 140, 640, 360)."""
    src_w, src_h, dst_w, dst_h = (int(v) for v in (src_w, src_h, dst_w, dst_h))
    if min(src_w, src_h, dst_w, dst_h) <= 0:
        raise ValueError("letterbox_rect: sizes must be positive")
    s = min(dst_w / src_w, dst_h / src_h)
    w = min(dst_w, 2 * round(src_w * s / 2))
    h = min(dst_h, 2 * round(src_h * s / 2))
    return ((dst_w - w) // 4) * 2, ((dst_h - h) // 4) * 2, w, h


def _rect(r, size, what, even=True):
    """A host rectangle (x, y, w, h): even, at least 2 x 2, inside `size` (even=False: any integers, at least 1 x 1);
    None = the whole surface."""
    if r is None:
        return (0, 0, size[0], size[1])
    try:
        x, y, w, h = (operator.index(v) for v in r)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: a rectangle is four integers (x, y, w, h)") from None
    if not even:
        if w < 1 or h < 1 or x < 0 or y < 0 or x + w > size[0] or y + h > size[1]:
            raise ValueError(f"{what}: {(x, y, w, h)} must be at least 1 x 1 and inside {size[0]} x {size[1]}")
        return (x, y, w, h)
    if (x | y | w | h) & 1 or w < 2 or h < 2 or x < 0 or y < 0 or x + w > size[0] or y + h > size[1]:
        raise ValueError(f"{what}: {(x, y, w, h)} must be even, at least 2 x 2 and inside {size[0]} x {size[1]}")
    return (x, y, w, h)


def _roi_record(src_rect, dst_rect, src_size, dst_size, even=True):
    return _rect(src_rect, src_size, "src_rect", even) + _rect(dst_rect, dst_size, "dst_rect", even)


def _roi_batch_records(srcs, dsts, src_rects=None, dst_rects=None):
    """RoiBatch's host checks, without a device: (the sources' one format, the rectangle records).  All sources
    share ONE format; NV12 sources, their destinations and rectangles are even, RGB / BGR / RGB_PLANAR ones are any
    integers with rectangles of at least 1 x 1.  ValueError otherwise."""
    srcs, dsts = list(srcs), list(dsts)
    n = len(srcs)
    if not n or len(dsts) != n:
        raise ValueError("RoiBatch: need equally long, non-empty src and dst lists")
    if n > 65535:
        raise ValueError("RoiBatch: at most 65535 items")
    src_rects = [None] * n if src_rects is None else list(src_rects)
    dst_rects = [None] * n if dst_rects is None else list(dst_rects)
    if len(src_rects) != n or len(dst_rects) != n:
        raise ValueError("RoiBatch: src_rects / dst_rects need one entry per item")
    if any(s is None or s.IsEmpty for s in srcs):
        raise ValueError("RoiBatch: sources must be non-empty surfaces")
    src_format = srcs[0].Format
    if any(s.Format != src_format for s in srcs):
        raise ValueError("RoiBatch: the sources of a batch must share one format")
    even = src_format not in PySurfacePreprocessor._RGB_SRC
    if even and any((s.Width | s.Height) & 1 for s in srcs):
        raise ValueError("RoiBatch: sources must be non-empty surfaces of even size")
    if dsts[0] is None:
        raise ValueError("RoiBatch: destinations must be non-empty surfaces")
    f0, s0 = dsts[0].Format, (dsts[0].Width, dsts[0].Height)
    for d in dsts:
        if d is None or d.IsEmpty or d.Format != f0 or (d.Width, d.Height) != s0 or (even and (d.Width | d.Height) & 1):
            raise ValueError("RoiBatch: destinations must share format and (for NV12 sources: even) size")
    return src_format, [_roi_record(sr, dr, (s.Width, s.Height), s0, even)
                        for s, sr, dr in zip(srcs, src_rects, dst_rects)]


def _pad_colour(pad):
    """pad=None: pixels outside the placement are left alone; (r, g, b) in 0..255: they take that colour"""
    if pad is None:
        return False, (0, 0, 0)
    try:
        rgb = tuple(operator.index(v) for v in pad)
    except (TypeError, ValueError):
        raise ValueError("pad: None or (r, g, b)") from None
    if len(rgb) != 3 or any(not 0 <= v <= 255 for v in rgb):
        raise ValueError("pad: None or (r, g, b) in 0..255")
    return True, rgb


class RoiBatch(PreparedBatch):
    """Device-resident arrays for n region items: source descriptors (one format, any sizes, repeats allowed),
    destination descriptors (one format and size) and rectangle records, uploaded once
    (PySurfacePreprocessor.PrepareRoiBatch)."""

    _owned = ("d_src", "d_dst", "d_roi")

    def __init__(self, gpu_id: int, stream: int, srcs: Sequence[Surface], dsts: Sequence[Surface], src_rects=None,
                 dst_rects=None):
        srcs, dsts = list(srcs), list(dsts)
        self.src_format, self.rects = _roi_batch_records(srcs, dsts, src_rects, dst_rects)
        n = len(srcs)
        f0, s0 = dsts[0].Format, (dsts[0].Width, dsts[0].Height)
        self._begin(gpu_id, stream, "PrepareRoiBatch()")
        self.n = n
        self.src_formats = tuple(s.Format for s in srcs)
        self.dst_format, self.dst_size = f0, s0
        self._keep = (srcs, dsts)
        self.d_src = shim.descs_upload(gpu_id, [s.desc() for s in srcs], stream)
        self.d_dst = shim.descs_upload(gpu_id, [d.desc() for d in dsts], stream)
        self.d_roi = shim.rois_upload(gpu_id, self.rects, stream)


# DLPack dtype (code, bits) -> (name, enum vali_dtype) of a destination tensor, and of one the JPEG encoder reads: uint8 too
_TENSOR_DTYPES, _TENSOR_SRC_DTYPES = FLOAT_DTYPES, DTYPES


def _layout(who, dtypes, shape, strides, code, bits):
    """the rules tensor_layout and tensor_src_layout share; `who` starts the messages"""
    shape = tuple(int(v) for v in shape)
    dtype = dtypes.get((int(code), int(bits)))
    if dtype is None:
        names = [d[0] for d in dtypes.values()]
        raise ValueError(f"{who}: the dtype must be {', '.join(names[:-1])} or {names[-1]} "
                         f"(DLPack code {code}, {bits} bits)")
    if len(shape) != 4:
        raise ValueError(f"{who}: need a 4-D tensor (N, 3, H, W), got {len(shape)}-D {shape}")
    if strides is None:
        strides = (3 * shape[2] * shape[3], shape[2] * shape[3], shape[3], 1)
    strides = tuple(int(v) for v in strides)
    if len(strides) != 4:
        raise ValueError(f"{who}: {len(strides)} strides for a 4-D tensor")
    n, c, h, w = shape
    if c != 3:
        raise ValueError(f"{who}: need 3 channels (N, 3, H, W), got C = {c}")
    if n < 1 or h < 1 or w < 1:
        raise ValueError(f"{who}: empty tensor {shape}")
    if n > 65535:
        raise ValueError(f"{who}: at most 65535 items")
    if any(v < 0 for v in strides):
        raise ValueError(f"{who}: negative strides {strides} (a flipped view) are not supported")
    sn, sc, sy, sx = strides
    # a dimension of size 1 has no meaningful stride: give it the one its layout would have
    if sx == 1 or (w == 1 and sc != 1):
        layout, row = "planar", w
    elif sc == 1 and (sx == 3 or w == 1):
        layout, row = "packed", 3 * w
    else:
        raise ValueError(f"{who}: strides {strides} are neither planar (x stride 1) nor channels last (c stride 1, "
                         "x stride 3) -- a transposed or strided view")
    if (h > 1 and sy < row) or (layout == "planar" and sc < 1) or (n > 1 and sn < 1):
        raise ValueError(f"{who}: strides {strides} of a {layout} {shape} tensor: rows overlap -- a transposed or "
                         "broadcast view")
    return layout, dtype[0]


def tensor_layout(shape, strides, code, bits):
    """Classify a destination tensor from its DLPack view, without a device: ("planar" | "packed", dtype name).
    `shape` is the logical (N, 3, H, W), `strides` are in elements.  planar: x stride 1 (contiguous tensors and every
    slice that keeps rows contiguous); packed: c stride 1 and x stride 3 (channels last).  ValueError, naming what is
    wrong, for everything else."""
    return _layout("out", _TENSOR_DTYPES, shape, strides, code, bits)


def tensor_src_layout(shape, strides, code, bits):
    """tensor_layout's rules for a tensor that is read (PyNvJpegEncoder.RunTensor): uint8 (DLPack code 1, 8 bits) is a
    dtype too, and the messages speak of `tensor`."""
    return _layout("tensor", _TENSOR_SRC_DTYPES, shape, strides, code, bits)


def _tensor_view(who, layout_of, cai_types, t, gpu_id):
    """(ptr, layout, dtype name, (n, h, w), (sn, sc, sy) in elements, holder) of a device tensor on `gpu_id`, seen
    through __dlpack__ or __cuda_array_interface__ (`cai_types`: the typestrs it may have there)"""
    seen, (layout, dtype) = device_float(who, t, layout_of, gpu_id, cai_types)
    n, _, h, w = seen.shape
    sn, sc, sy, _ = seen.strides or (3 * h * w, h * w, w, 1)
    row = w if layout == "planar" else 3 * w
    # strides of dimensions of size 1 are arbitrary: the kernel's addressing needs them positive and rows apart
    return seen.ptr, layout, dtype, (n, h, w), (max(sn, 1), max(sc, 1), max(sy, row)), seen.holder


def _tensor_dst(out, gpu_id):
    """(shim.TensorDst, layout, dtype name, (n, h, w), holder) of a destination tensor on `gpu_id`"""
    ptr, layout, dtype, (n, h, w), (sn, sc, sy), holder = _tensor_view(
        "out", tensor_layout, ("<f4", "<f2"), out, gpu_id)
    code = {"float32": shim.DTYPE_F32, "float16": shim.DTYPE_F16, "bfloat16": shim.DTYPE_BF16}[dtype]
    dst = shim.TensorDst(ptr, code, 1 if layout == "packed" else 0, n, w, h, sn, sc, sy)
    return dst, layout, dtype, (n, h, w), holder


def _tensor_src(tensor, gpu_id):
    """(shim.TensorSrc, layout, dtype name, (n, h, w), (ptr, stride_n, stride_c, stride_y), holder) of a tensor the
    JPEG encoder on `gpu_id` reads; strides in elements"""
    ptr, layout, dtype, (n, h, w), (sn, sc, sy), holder = _tensor_view(
        "tensor", tensor_src_layout, ("<f4", "<f2", "|u1"), tensor, gpu_id)
    code = {"float32": shim.DTYPE_F32, "float16": shim.DTYPE_F16, "bfloat16": shim.DTYPE_BF16,
            "uint8": shim.DTYPE_U8}[dtype]
    src = shim.TensorSrc(ptr, code, 1 if layout == "packed" else 0, n, w, h, sn, sc, sy)
    return src, layout, dtype, (n, h, w), (ptr, sn, sc, sy), holder


class _Canvas:
    """what _roi_batch_records reads of a destination: the tensor's canvas stands in for N equal surfaces"""
    IsEmpty = False

    def __init__(self, w, h):
        self.Format, self.Width, self.Height = F.RGB_32F_PLANAR, w, h


class TensorBatch(PreparedBatch):
    """Device-resident arrays for n region items that land in ONE batch tensor: source descriptors (one format, any
    sizes, repeats allowed) and rectangle records, uploaded once (PySurfacePreprocessor.PrepareTensorBatch).  Keeps the
    sources and the tensor alive."""

    _owned = ("d_src", "d_roi")

    def __init__(self, gpu_id: int, stream: int, srcs: Sequence[Surface], out, src_rects=None, dst_rects=None):
        srcs = list(srcs)
        self.dst, self.layout, self.dtype, (n, h, w), holder = _tensor_dst(out, gpu_id)
        if len(srcs) != n:
            raise ValueError(f"TensorBatch: {len(srcs)} sources for a tensor of {n} items")
        canvas = _Canvas(w, h)
        self.src_format, self.rects = _roi_batch_records(srcs, [canvas] * n, src_rects, dst_rects)
        self._begin(gpu_id, stream, "PrepareTensorBatch()")
        self.n = n
        self.dst_size = (w, h)
        self.out = out
        self._keep = (srcs, out, holder)
        self.d_src = shim.descs_upload(gpu_id, [s.desc() for s in srcs], stream)
        self.d_roi = shim.rois_upload(gpu_id, self.rects, stream)


# ---- PySurfaceRotator --------------------------------------------------------------------
# ---- PySurfacePostprocessor: a batch tensor back into video frames ----------------------------------
def _f32(v: float) -> float:
    """a double rounded to float32 once"""
    import struct

    return struct.unpack("<f", struct.pack("<f", v))[0]


def _bt709_rgb2yuv(mpeg: bool):
    """BT.709 RGB -> YCbCr (include/vali_hip.h spells the formulas and the numbers out): Kr = 0.2126, Kb = 0.0722; full
    range, or the Y row x 219 / 255 + 16 and the chroma rows x 224 / 255 + 128; computed in double, rounded once."""
    kr, kb = 0.2126, 0.0722
    kg = 1.0 - kr - kb
    rows = ((kr, kg, kb), (-kr / (2 * (1 - kb)), -kg / (2 * (1 - kb)), 0.5), (0.5, -kg / (2 * (1 - kr)), -kb / (2 * (1 - kr))))
    ys, cs, y0 = (219.0 / 255.0, 224.0 / 255.0, 16.0) if mpeg else (1.0, 1.0, 0.0)
    return tuple(tuple(_f32(v * (ys if k == 0 else cs)) for v in row) + ((y0 if k == 0 else 128.0),)
                 for k, row in enumerate(rows))


RGB2YUV_BT709_JPEG = _bt709_rgb2yuv(False)
RGB2YUV_BT709_MPEG = _bt709_rgb2yuv(True)


class FrameBatch(PreparedBatch):
    """One (N, 3, H, W) tensor and the N surfaces it is written into: the destination descriptors uploaded once
    (PySurfacePostprocessor.PrepareTensorBatch).  Keeps the tensor and the surfaces alive."""

    _owned = ("d_dst",)

    def __init__(self, gpu_id: int, stream: int, tensor, dsts: Sequence[Surface]):
        self.src, self.layout, self.dtype, (n, h, w), _, holder = _tensor_src(tensor, gpu_id)
        dsts = list(dsts)
        if len(dsts) != n:
            raise ValueError(f"FrameBatch: {len(dsts)} surfaces for a tensor of {n} items")

        def same_size(i, d):
            if (d.Width, d.Height) != (w, h):
                raise ValueError(f"FrameBatch: surface {i} is {d.Width}x{d.Height}, the tensor's items are {w}x{h}: "
                                 "the sizes must be equal (no resizing on the way out)")

        fmt = frames_of_one_format("FrameBatch", dsts, PySurfacePostprocessor._DST, gpu_id, same_size)
        self._begin(gpu_id, stream, "PrepareTensorBatch()")
        self.n = n
        self.size = (w, h)
        self.dst_format = fmt
        self.tensor = tensor
        self._keep = (tensor, holder, dsts)
        self.d_dst = shim.descs_upload(gpu_id, [d.desc() for d in dsts], stream)


class PySurfacePostprocessor(_SurfaceTask):
    """One (N, 3, H, W) tensor -> N NV12, YUV420, YUV444, RGB or RGB_PLANAR surfaces of W x H, ONE launch
    (vali_tensor_to_surfaces): the way from a network's output back to what PyNvEncoder, the resizer, the rotator and the
    JPEG encoder take.  The mirror image of PySurfacePreprocessor.RunTensorBatch.

    The reference has no such task.  It is DEFINED as the chain it replaces and is byte-identical to it
    (tests/test_gpu_postproc.py):

        p = torch.nan_to_num(x.float() * scale + offset, nan=0.0).round().clamp(0, 255).to(torch.uint8)
        per item: Surface.from_dlpack(p as H x W x 3, RGB) -> PySurfaceConverter RGB -> YUV420 [-> NV12] / YUV444 / RGB_PLANAR

    `tensor`: float32, float16, bfloat16 or uint8 through `__dlpack__` or `__cuda_array_interface__`; contiguous, a slice
    that keeps rows contiguous, or channels last (the rules and messages of PyNvJpegEncoder.RunTensor).
    `scale`, `offset`: a number or three, per TENSOR channel; scale=None is 255 for the float dtypes, 1 for uint8.
    `channels`: "RGB" or "BGR", the order of the tensor's channels.
    `cc_ctx`: None or BT_601 + JPEG -> nppiRGBToYUV's matrix, BT_601 + MPEG -> nppiRGBToYCbCr's (the two PySurfaceConverter
    uses); BT_709 + JPEG / MPEG -> RGB2YUV_BT709_JPEG / _MPEG, this project's own (the reference has no RGB -> YUV call
    for BT.709); anything else: (False, UNSUPPORTED_FMT_CONV_PARAMS), nothing is launched.  Ignored for RGB destinations.
    """

    _DST = (F.NV12, F.YUV420, F.YUV444, F.RGB, F.RGB_PLANAR)
    _MATRICES = {
        (ColorSpace.BT_601, ColorRange.JPEG): RGB2YUV_NPP_YUV,
        (ColorSpace.BT_601, ColorRange.MPEG): RGB2YUV_NPP_YCBCR,
        (ColorSpace.BT_709, ColorRange.JPEG): RGB2YUV_BT709_JPEG,
        (ColorSpace.BT_709, ColorRange.MPEG): RGB2YUV_BT709_MPEG,
    }

    @staticmethod
    def SupportedFormats() -> List[PixelFormat]:
        """every destination format the task writes"""
        return list(PySurfacePostprocessor._DST)

    @staticmethod
    def Matrix(cc_ctx=None):
        """the RGB -> YUV rows (kR, kG, kB, offset) of Y, U, V that `cc_ctx` selects, or None if it selects none"""
        space, rng = _space_range(cc_ctx, ColorSpace.BT_601, ColorRange.JPEG)
        return PySurfacePostprocessor._MATRICES.get((space, rng))

    def PrepareTensorBatch(self, tensor, dsts: Sequence[Surface]) -> FrameBatch:
        return FrameBatch(self._gpu_id, self._stream, tensor, dsts)

    def RunTensorBatchAsync(self, batch: FrameBatch, scale=None, offset=0.0, cc_ctx=None,
                            channels: str = "RGB") -> Tuple[bool, TaskExecInfo]:
        """One launch over the items of `batch`."""
        from .codecs import _triple

        if not isinstance(batch, FrameBatch):
            raise ValueError("RunTensorBatch: pass a FrameBatch (PrepareTensorBatch)")
        if channels not in ("RGB", "BGR"):
            raise ValueError(f"channels: 'RGB' or 'BGR', got {channels!r}")
        offset = _triple("offset", offset)
        scale = _triple("scale", (1.0 if batch.dtype == "uint8" else 255.0) if scale is None else scale)
        supported, params = _rgb2yuv_params(batch.dst_format, cc_ctx)
        if not supported:
            return _UNSUPP_CC_PAIR
        d = _status(shim.tensor_to_surfaces(batch.src, scale, offset, 1 if channels == "BGR" else 0, batch.d_dst,
                                            int(batch.dst_format), params, self._stream))
        return d.success, d.info

    def RunTensorBatch(self, batch: FrameBatch, scale=None, offset=0.0, cc_ctx=None,
                       channels: str = "RGB") -> Tuple[bool, TaskExecInfo]:
        r = self.RunTensorBatchAsync(batch, scale, offset, cc_ctx, channels)
        self._sync()
        return r


_UNSUPP_CC_PAIR = (_S_UNSUPP_CC.success, _S_UNSUPP_CC.info)


def _rgb2yuv_params(fmt, cc_ctx):
    """(supported, params) for a task that writes RGB values into frames of `fmt`: the params carry the RGB -> YUV matrix
    `cc_ctx` picks (PySurfacePostprocessor.Matrix) and are None for the RGB formats; not supported: it picks none"""
    if fmt not in (F.NV12, F.YUV420, F.YUV444):
        return True, None
    mat = PySurfacePostprocessor.Matrix(cc_ctx)
    return (False, None) if mat is None else (True, _params(rgb2yuv=mat))


# ---- PySurfaceAnnotator: outlines, fills and pixelation from GPU-held marks ------------------------------
MARK_NONE, MARK_BOX, MARK_FILL, MARK_PIXELATE, MARK_STAMP = 0, 1, 2, 3, 4
MAX_MARKS = 4096
_PIXELATE_CELLS = (4, 8, 16, 32)


def pack_colour(r: int, g: int, b: int, a: int = 255) -> int:
    """the int32 a mark row carries as its colour: bits a << 24 | r << 16 | g << 8 | b (negative for a >= 128)"""
    r, g, b, a = (operator.index(v) for v in (r, g, b, a))
    if any(not 0 <= v <= 255 for v in (r, g, b, a)):
        raise ValueError("pack_colour: r, g, b, a in 0..255")
    v = a << 24 | r << 16 | g << 8 | b
    return v - (1 << 32) if v >= 1 << 31 else v


def pack_uv(u: int, v: int) -> int:
    """the `arg` of a MARK_STAMP row: the stamp's origin (u, v) in the atlas, u | v << 16 as an int32"""
    u, v = operator.index(u), operator.index(v)
    if not (0 <= u <= 65535 and 0 <= v <= 65535):
        raise ValueError("pack_uv: u, v in 0..65535")
    a = u | v << 16
    return a - (1 << 32) if a >= 1 << 31 else a


def _host_marks(rows, sizes, is420, atlas_size=None):
    """a host sequence of (frame, x, y, w, h, kind, arg, colour): the rules the kernel applies to a device tensor, with
    ValueErrors where the kernel would skip the row -- except kind 0 and unknown kinds, which are skipped here too.
    MARK_STAMP is a known kind when the call has an atlas (atlas_size = (AW, AH))"""
    out = []
    for i, row in enumerate(rows):
        try:
            r = tuple(operator.index(v) for v in row)
        except TypeError:
            raise ValueError(f"marks: row {i} must be 8 integers (frame, x, y, w, h, kind, arg, colour)") from None
        if len(r) != 8:
            raise ValueError(f"marks: row {i} has {len(r)} values, need 8 (frame, x, y, w, h, kind, arg, colour)")
        if any(not -(1 << 31) <= v < (1 << 31) for v in r):
            raise ValueError(f"marks: row {i}: every value must fit an int32 (colours: pack_colour)")
        frame, x, y, w, h, kind, arg, _ = r
        out.append(r)
        if kind not in (MARK_BOX, MARK_FILL, MARK_PIXELATE) and not (kind == MARK_STAMP and atlas_size is not None):
            continue
        if not 0 <= frame < len(sizes):
            raise ValueError(f"marks: row {i}: frame {frame} is outside 0..{len(sizes) - 1}")
        if w < 1 or h < 1:
            raise ValueError(f"marks: row {i}: the rectangle is {w}x{h}; width and height must be at least 1")
        if kind == MARK_BOX and arg < 1:
            raise ValueError(f"marks: row {i}: MARK_BOX needs a thickness of at least 1, got {arg}")
        if kind == MARK_PIXELATE and arg not in _PIXELATE_CELLS:
            raise ValueError(f"marks: row {i}: MARK_PIXELATE needs a cell of 4, 8, 16 or 32, got {arg}")
        if kind == MARK_STAMP:
            u, v = arg & 0xFFFF, (arg >> 16) & 0xFFFF
            if u >= atlas_size[0] or v >= atlas_size[1]:
                raise ValueError(f"marks: row {i}: the stamp's origin ({u}, {v}) is outside the atlas "
                                 f"({atlas_size[0]}x{atlas_size[1]}); arg: pack_uv")
        x0, y0, x1, y1 = x, y, x + w, y + h
        if is420 and kind != MARK_STAMP:      # (a stamp is not snapped; snapping never changes the answer below)
            x0, y0, x1, y1 = x0 & ~1, y0 & ~1, (x1 + 1) & ~1, (y1 + 1) & ~1
        fw, fh = sizes[frame]
        if x0 >= fw or y0 >= fh or x1 <= 0 or y1 <= 0:
            raise ValueError(f"marks: row {i}: the rectangle ({x}, {y}, {w}, {h}) does not meet frame {frame} ({fw}x{fh})")
    return out


def _atlas_size(atlas, gpu_id):
    """(AW, AH) of a coverage atlas: a Surface of format Y on the task's device"""
    fmt = getattr(atlas, "Format", None)
    if fmt is None or not hasattr(atlas, "desc"):
        raise ValueError(f"atlas: need a Surface of format Y, got {type(atlas).__name__}")
    if fmt != F.Y:
        raise ValueError(f"atlas: the surface has format {fmt!r}; a coverage atlas is one 8-bit plane, format Y")
    if atlas.IsEmpty:
        raise ValueError("atlas: the surface is empty")
    dev = getattr(atlas, "DeviceId", gpu_id)
    if dev != gpu_id:
        raise ValueError(f"atlas: the surface is on device {dev}, the task on {gpu_id}")
    return atlas.Width, atlas.Height


class AnnotateBatch(PreparedBatch):
    """The frames PySurfaceAnnotator.RunBatch draws on: N >= 0 surfaces of one format, any sizes; descriptors, the
    kernel's workspace and a staging buffer for host-side marks are set up once (PySurfaceAnnotator.PrepareBatch).
    Keeps the surfaces alive."""

    _owned = ("d_frames", "d_ws", "d_marks")

    def __init__(self, gpu_id: int, stream: int, frames: Sequence[Surface]):
        frames = list(frames)
        fmt = frames_of_one_format("AnnotateBatch", frames, PAINT_FORMATS, gpu_id)
        self._begin(gpu_id, stream, "PrepareBatch()" if frames else None, frames)     # no frames: nothing is allocated
        self.n = len(frames)
        self.format = fmt
        self._keep = frames
        self._marks_keep = None
        self.ws_bytes = 0
        if frames:
            self.ws_bytes = shim.annotate_workspace_size(self.descs)
            self.d_ws = shim.mem_alloc(gpu_id, self.ws_bytes)
            self.d_marks = shim.mem_alloc(gpu_id, MAX_MARKS * 32)


class PySurfaceAnnotator(_SurfaceTask):
    """Outlines (MARK_BOX), filled or translucent regions (MARK_FILL) and pixelation (MARK_PIXELATE) drawn IN PLACE onto a
    batch of NV12, YUV420, YUV444, RGB, BGR or RGB_PLANAR frames of any sizes, in two launches whatever the marks
    (vali_annotate_batch): the step between a detector's output and PyNvEncoder or the JPEG encoder.

    `marks`: an int32 (M, 8) contiguous GPU tensor (`__dlpack__` or `__cuda_array_interface__`), M <= 4096, rows
    (frame, x, y, w, h, kind, arg, colour) -- its VALUES are never read on the host, so a detector's boxes are drawn
    without a device-to-host synchronisation; a row is skipped when its kind is MARK_NONE or unknown, its frame is outside
    the batch, w < 1 or h < 1, arg is invalid for the kind (BOX: thickness >= 1; PIXELATE: cell 4, 8, 16 or 32) or the
    rectangle does not meet its frame.  Or a host sequence of such 8-tuples, checked here (the last four are ValueErrors)
    and uploaded with one blocking copy on the task's stream.  Marks are applied in row order.  `colour`: pack_colour().
    The definition, sample for sample, is in include/vali_hip.h; the reference has no such task.

    `atlas` (RunBatch): a coverage atlas for MARK_STAMP rows -- a Surface of format Y on the task's device (Surface.Make,
    or Surface.from_dlpack(t, vali.Y) of a uint8 (H, W) GPU tensor: a pitched view at any address).  A STAMP row blends
    its colour into its w x h rectangle with the per-pixel weight atlas[v + dy][u + dx], (u, v) = its `arg` (pack_uv), at
    scale 1:1; beyond the atlas the weight is zero.  Labels: render_labels / LabelAtlas.  Without an atlas kind 4 is an
    unknown kind.  The batch keeps the atlas alive, as it keeps a marks tensor.

    `cc_ctx` picks the RGB -> YUV matrix for colours on YUV frames exactly as PySurfacePostprocessor.Matrix does; an
    unsupported one gives (False, UNSUPPORTED_FMT_CONV_PARAMS) and nothing is launched.  Ignored for RGB formats.
    """

    _FORMATS = PAINT_FORMATS

    @staticmethod
    def SupportedFormats() -> List[PixelFormat]:
        return list(PAINT_FORMATS)

    def PrepareBatch(self, frames: Sequence[Surface]) -> AnnotateBatch:
        return AnnotateBatch(self._gpu_id, self._stream, frames)

    def RunBatchAsync(self, batch: AnnotateBatch, marks, cc_ctx=None, atlas=None) -> Tuple[bool, TaskExecInfo]:
        if not isinstance(batch, AnnotateBatch):
            raise ValueError("RunBatch: pass an AnnotateBatch (PrepareBatch)")
        atlas_size = _atlas_size(atlas, self._gpu_id) if atlas is not None else None
        if is_tensor(marks):      # the values are the kernel's to sanitise
            ptr, (m, _), batch._marks_keep = device_i32("marks", marks, (None, 8), self._gpu_id, "the batch", "(M, 8)",
                                                        least=0)
            if m > MAX_MARKS:
                raise ValueError(f"marks: {m} rows; at most {MAX_MARKS} per call")
            host = None
        else:
            try:
                rows = list(marks)
            except TypeError:
                raise ValueError("marks: a device tensor with __cuda_array_interface__ or __dlpack__, or a sequence of "
                                 "8-tuples") from None
            if len(rows) > MAX_MARKS:
                raise ValueError(f"marks: {len(rows)} rows; at most {MAX_MARKS} per call")
            host = _host_marks(rows, batch.sizes, batch.format in (F.NV12, F.YUV420), atlas_size)
            ptr, m = batch.d_marks, len(host)
        supported, params = _rgb2yuv_params(batch.format, cc_ctx)
        if not supported:
            return _UNSUPP_CC_PAIR
        if batch.n == 0 or m == 0:
            return _OK_PAIR
        if host is not None:
            upload_i32(self._gpu_id, self._stream, [v for r in host for v in r], ptr)
        batch._atlas_keep = atlas
        d = _status(shim.annotate_batch(batch.descs, batch.d_frames, int(batch.format), ptr, m, params, batch.d_ws,
                                        batch.ws_bytes, self._stream, atlas.desc() if atlas is not None else None))
        return d.success, d.info

    def RunBatch(self, batch: AnnotateBatch, marks, cc_ctx=None, atlas=None) -> Tuple[bool, TaskExecInfo]:
        r = self.RunBatchAsync(batch, marks, cc_ctx, atlas)
        self._sync()
        return r


def render_labels(labels, font=None, pad: int = 1):
    """Text labels as a coverage atlas for MARK_STAMP rows (host only; needs Pillow): returns (atlas, rects), `atlas` a
    (H, W) uint8 numpy array and `rects` an (L, 4) int32 array of (u, v, w, h).  Each label is one strip -- its text,
    antialiased, with `pad` pixels of zero coverage around it -- and the strips are stacked top to bottom from column 0.
    `font`: a PIL ImageFont; None uses ImageFont.load_default(), which is built into Pillow.  Whole-label strips keep a
    detector's class ids on the GPU: gather rects[class_id] there and build the STAMP rows with a few tensor operations."""
    try:
        from PIL import Image, ImageDraw, ImageFont
    except Exception as exc:  # pragma: no cover - depends on the environment
        raise RuntimeError(f"render_labels: Pillow (PIL) is not importable ({exc})") from exc
    import numpy as np

    labels = [str(t) for t in labels]
    pad = operator.index(pad)
    if pad < 0:
        raise ValueError("render_labels: pad must be at least 0")
    if not labels:
        raise ValueError("render_labels: no labels")
    if font is None:
        font = ImageFont.load_default()
    try:        # one height and one baseline for every label of a scalable font
        ascent, descent = font.getmetrics()
        line = ascent + descent
    except AttributeError:
        line = None
    strips = []
    for text in labels:
        left, top, right, bottom = (int(v) for v in font.getbbox(text)) if text else (0, 0, 0, 0)
        if line is not None:
            top, bottom = min(top, 0), max(bottom, line)
        w, h = max(right - left, 1) + 2 * pad, max(bottom - top, 1) + 2 * pad
        img = Image.new("L", (w, h), 0)
        if text:
            ImageDraw.Draw(img).text((pad - left, pad - top), text, fill=255, font=font)
        strips.append(np.asarray(img, dtype=np.uint8))
    width = max(s.shape[1] for s in strips)
    height = sum(s.shape[0] for s in strips)
    if width > 65535 or height > 65535:
        raise ValueError(f"render_labels: the atlas would be {width}x{height}; an atlas is at most 65535 on a side")
    atlas = np.zeros((height, width), np.uint8)
    rects = np.zeros((len(strips), 4), np.int32)
    v = 0
    for i, s in enumerate(strips):
        atlas[v:v + s.shape[0], :s.shape[1]] = s
        rects[i] = (0, v, s.shape[1], s.shape[0])
        v += s.shape[0]
    return atlas, rects


class LabelAtlas:
    """render_labels, uploaded once: `.surface` (the Y surface RunBatch takes as `atlas`), `.rects` ((L, 4) int32 numpy,
    (u, v, w, h) of each label) and `.labels`."""

    def __init__(self, gpu_id: int, labels, font=None, pad: int = 1):
        from .transfer import PyFrameUploader

        self.labels = [str(t) for t in labels]
        atlas, self.rects = render_labels(self.labels, font, pad)
        self.surface = Surface.Make(F.Y, atlas.shape[1], atlas.shape[0], gpu_id)
        ok, info = PyFrameUploader(gpu_id).Run(atlas.reshape(-1), self.surface)
        if not ok:
            raise RuntimeError(f"LabelAtlas: the upload failed ({info})")


_ROT_FORMATS = [F.Y, F.GRAY12, F.RGB, F.BGR, F.RGB_PLANAR, F.YUV420, F.YUV422, F.YUV444, F.RGB_32F,
                F.RGB_32F_PLANAR, F.YUV444_10bit, F.YUV420_10bit]
# format -> (driver, element size); RotateSurface::Run switch (RotateSurface.cpp:168-208)
_ROT_IMPL = {
    F.Y: ("planar", 1), F.RGB: ("packed", 1), F.BGR: ("packed", 1), F.RGB_PLANAR: ("planar", 1),
    F.YUV420: ("planar", 1), F.YUV422: ("planar", 1), F.YUV444: ("planar", 1),
    F.RGB_32F: ("packed", 4), F.RGB_32F_PLANAR: ("planar", 4), F.YUV444_10bit: ("planar", 2),
    F.YUV420_10bit: ("planar", 2),
}


class PySurfaceRotator(_SurfaceTask):
    """Rotate a Surface by an arbitrary angle (bilinear) with optional shift.

    reference: src/python_vali/src/PySurfaceRotator.cpp:26-200; RotateSurface::Run
    (src/TC/src/RotateSurface.cpp:161-214).  Multiples of 90 degrees with zero shifts are
    normalised so the image lands exactly inside the (transposed) destination.
    Deviation: for that special case the reference hands the LUMA-sized shifts to every
    plane, which pushes the half-size chroma planes of YUV420/422 out of their
    destination; here each plane gets the shifts derived from its own size.
    """

    def __init__(self, gpu_id: int, stream=None):
        super().__init__(gpu_id, stream)

    @property
    def SupportedFormats(self) -> List[PixelFormat]:
        return list(_ROT_FORMATS)

    @staticmethod
    def _normalise(angle: float, shift_x: float, shift_y: float):
        """PySurfaceRotator::Run (:40-73): multiples of 90 degrees with zero shifts become
        (normalised angle, per-plane canonical shifts)."""
        import math

        if math.fmod(angle, 90.0) == 0.0 and shift_x == 0.0 and shift_y == 0.0:
            return float((int(round(angle)) + 360) % 360), True
        return float(angle), False

    @staticmethod
    def _check(src_format, dst_format, num_components, num_planes) -> Optional[TaskExecDetails]:
        if src_format != dst_format:                                     # RotateSurface.cpp:162-164
            return TaskExecDetails.failed(TaskExecInfo.SRC_DST_FMT_MISMATCH)
        impl = _ROT_IMPL.get(src_format)
        if impl is None:                                                 # :204-206
            return TaskExecDetails.failed(TaskExecInfo.NOT_SUPPORTED)
        kind, _ = impl
        if kind == "planar" and num_components != num_planes:            # RotPlanar, :135-136
            return TaskExecDetails.failed(TaskExecInfo.INVALID_INPUT)
        if kind == "packed" and num_planes != 1:                         # RotPacked, :152-153
            return TaskExecDetails.failed(TaskExecInfo.INVALID_INPUT)
        return None

    def _run(self, src: Surface, dst: Surface, angle: float, shift_x: float, shift_y: float
             ) -> TaskExecDetails:
        err = self._check(src.Format, dst.Format, src.NumComponents, src.NumPlanes)
        if err is not None:
            return err
        key = (src.desc(), dst.desc(), angle, shift_x, shift_y)
        angle, per_plane = self._normalise(angle, shift_x, shift_y)
        d = _status(shim.rotate(src.desc(), dst.desc(), angle, shift_x, shift_y, int(per_plane),
                                self._stream))
        if d is _S_OK:
            self._memo_put(key, shim.rotate, (angle, shift_x, shift_y, int(per_plane)))
        return d

    def PrepareBatch(self, srcs: Sequence[Surface], dsts: Sequence[Surface]) -> "SurfaceBatch":
        return SurfaceBatch(self._gpu_id, self._stream, srcs, dsts)

    def RunBatchAsync(self, batch, dsts=None, angle: float = 0.0, shift_x: float = 0.0,
                      shift_y: float = 0.0) -> Tuple[bool, TaskExecInfo]:
        """One launch rotates every plane of every surface of the batch."""
        batch = self._batch_of(batch, dsts)
        err = self._check(batch.src_format, batch.dst_format, batch.src_components, batch.src_planes)
        if err is not None:
            return False, err.info
        angle, per_plane = self._normalise(float(angle), float(shift_x), float(shift_y))
        d = _status(shim.rotate_batch(batch.d_src, batch.d_dst, batch.n, int(batch.src_format),
                                      batch.src_size[0], batch.src_size[1], batch.dst_size[0],
                                      batch.dst_size[1], angle, float(shift_x), float(shift_y),
                                      int(per_plane), self._stream))
        return d.success, d.info

    def RunBatch(self, batch, dsts=None, angle: float = 0.0, shift_x: float = 0.0,
                 shift_y: float = 0.0) -> Tuple[bool, TaskExecInfo]:
        r = self.RunBatchAsync(batch, dsts, angle, shift_x, shift_y)
        self._sync()
        return r

    def RunAsync(self, src: Surface, dst: Surface, angle: float, shift_x: float = 0.0,
                 shift_y: float = 0.0) -> Tuple[bool, TaskExecInfo]:
        angle, shift_x, shift_y = float(angle), float(shift_x), float(shift_y)
        try:
            d1, d2 = src._desc, dst._desc
            m = self._memo.get((d1, d2, angle, shift_x, shift_y))
        except (AttributeError, TypeError):
            m = None
        if m is not None and m[0](d1, d2, *m[1], self._stream) == 0:
            return _OK_PAIR
        d = self._run(src, dst, angle, shift_x, shift_y)
        return d.success, d.info

    def Run(self, src: Surface, dst: Surface, angle: float, shift_x: float = 0.0,
            shift_y: float = 0.0) -> Tuple[bool, TaskExecInfo]:
        r = self.RunAsync(src, dst, angle, shift_x, shift_y)
        self._sync()
        return r


# ---- PySurfaceResizer --------------------------------------------------------------------
_RESIZE_FORMATS = (F.RGB, F.BGR, F.YUV420, F.YUV444, F.RGB_PLANAR, F.RGB_32F, F.RGB_32F_PLANAR, F.NV12,
                   # beyond the reference's list (TaskResizeSurface.cpp:293-309): same kernel
                   F.Y, F.P10, F.P12, F.YUV422, F.YUV420_10bit, F.YUV444_10bit)


class PySurfaceResizer(_SurfaceTask):
    """Resize a Surface to the size of the destination Surface.

    reference: src/python_vali/src/PySurfaceResizer.cpp:28-147; ResizeSurface
    (src/TC/src/TaskResizeSurface.cpp:293-328).  One launch resizes every plane (NV12 needs
    five NPP launches and two temporaries in the reference).  The default filter is the reference's:
    every nppiResize call site passes NPPI_INTER_LANCZOS (TaskResizeSurface.cpp:67,116,224,273), so
    `PySurfaceResizer(format, gpu_id[, stream])` is the 6x6 Lanczos-3 -- 3 lobes, normalised taps on the
    grid src = dst * scale, pinned against NPP output at a non-integer ratio at 45.6 dB
    (tests/test_oracle_reference_pins.py).  `interpolation=Interpolation.LINEAR` selects the bilinear
    filter BASELINE.json config 3 names, `Interpolation.CUBIC` the 4x4 Catmull-Rom bicubic (both
    extensions: the reference has no switch).
    RGB_PLANAR: the reference resizes the 3 stacked planes as ONE W x 3H image so rows
    bleed across channel seams (TaskResizeSurface.cpp:298, Surfaces.hpp:409); here each
    channel is resized on its own.
    """

    def __init__(self, format: PixelFormat, gpu_id: int, stream=None,
                 interpolation: Interpolation = Interpolation.LANCZOS):
        fmt = PixelFormat(format)
        if fmt not in _RESIZE_FORMATS:                       # TaskResizeSurface.cpp:307-308
            raise RuntimeError("pixel format not supported")
        super().__init__(gpu_id, stream)
        self._format = fmt
        self._interp = int(Interpolation(interpolation))

    @property
    def Interpolation(self) -> Interpolation:
        return Interpolation(self._interp)

    @property
    def Format(self) -> PixelFormat:
        return self._format

    def _run(self, src: Surface, dst: Surface) -> TaskExecDetails:
        if src is None or dst is None or src.IsEmpty or dst.IsEmpty:
            return _S_INVALID
        if dst.Format != src.Format or src.Format != self._format:   # :46-48, :93-95
            return _S_INVALID
        d = _status(shim.resize(src.desc(), dst.desc(), self._interp, self._stream))
        if d is _S_OK:
            self._memo_put((src.desc(), dst.desc()), shim.resize, (self._interp,))
        return d

    def RunAsync(self, src: Surface, dst: Surface) -> Tuple[bool, TaskExecInfo]:
        try:
            d1, d2 = src._desc, dst._desc
            m = self._memo.get((d1, d2))
        except (AttributeError, TypeError):
            m = None
        if m is not None and m[0](d1, d2, *m[1], self._stream) == 0:
            return _OK_PAIR
        d = self._run(src, dst)
        return d.success, d.info

    def Run(self, src: Surface, dst: Surface) -> Tuple[bool, TaskExecInfo]:
        r = self.RunAsync(src, dst)
        self._sync()
        return r

    def PrepareBatch(self, srcs: Sequence[Surface], dsts: Sequence[Surface]) -> "SurfaceBatch":
        return SurfaceBatch(self._gpu_id, self._stream, srcs, dsts)

    def RunBatchAsync(self, batch, dsts=None) -> Tuple[bool, TaskExecInfo]:
        batch = self._batch_of(batch, dsts)
        if batch.src_format != batch.dst_format or batch.src_format != self._format:
            return False, TaskExecInfo.INVALID_INPUT
        d = _status(shim.resize_batch(batch.d_src, batch.d_dst, batch.n, int(self._format),
                                      batch.src_size[0], batch.src_size[1],
                                      batch.dst_size[0], batch.dst_size[1], self._interp,
                                      self._stream))
        return d.success, d.info

    def RunBatch(self, batch, dsts=None) -> Tuple[bool, TaskExecInfo]:
        r = self.RunBatchAsync(batch, dsts)
        self._sync()
        return r
