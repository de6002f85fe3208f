"""What every prepared batch -- the object a task's Prepare* call returns -- shares: the refusal to be made while the stream
is capturing, the device arrays it owns and their teardown after its stream, the bookkeeping of a list of frames, and the
rules for such a list."""
from __future__ import annotations

from ._native import shim
from .enums import PixelFormat
from .runtime import is_capturing

F = PixelFormat

# the formats the tasks that draw on frames take (PySurfaceAnnotator.SupportedFormats)
PAINT_FORMATS = (F.NV12, F.YUV420, F.YUV444, F.RGB, F.BGR, F.RGB_PLANAR)


def _release(batch, names):
    """The teardown of a prepared batch (its __del__): free the device arrays it names, after the batch's stream."""
    if any(getattr(batch, name, 0) for name in names):
        try:    # a launch issued on the batch's stream may still be using the arrays
            shim.stream_sync(batch.gpu_id, batch._stream)
        except Exception:
            pass
    for name in names:
        p = getattr(batch, name, 0)
        if p:
            try:
                shim.mem_free(batch.gpu_id, p)
            except Exception:
                pass
            setattr(batch, name, 0)


def not_empty(who, i, surface):
    if surface is None or surface.IsEmpty:
        raise ValueError(f"{who}: surface {i} is empty")


def on_device(who, i, surface, gpu_id):
    dev = getattr(surface, "DeviceId", gpu_id)
    if dev != gpu_id:
        raise ValueError(f"{who}: surface {i} is on device {dev}, the task on {gpu_id}")


def surfaces_on_device(who, surfaces, gpu_id):
    """The rules for surfaces of any formats: none empty, all on `gpu_id`."""
    for i, d in enumerate(surfaces):
        not_empty(who, i, d)
        on_device(who, i, d, gpu_id)


def frames_of_one_format(who, frames, formats, gpu_id, also=None):
    """The rules for the surfaces a batch writes to: none empty, one of `formats` and the same for all, 4:2:0 ones of even
    size, all on `gpu_id`.  `also(i, surface)`: the caller's own check, made once the surface's format is known.
    Returns the format (None for no surfaces)."""
    fmt = None
    for i, d in enumerate(frames):
        not_empty(who, i, d)
        if d.Format not in formats:
            raise ValueError(f"{who}: surface {i} has format {d.Format!r}; supported: "
                             f"{', '.join(f.name for f in formats)}")
        if fmt is not None and d.Format != fmt:
            raise ValueError(f"{who}: surface {i} has format {d.Format!r}, surface 0 {fmt!r}: one format per batch")
        fmt = d.Format
        if also is not None:
            also(i, d)
        if fmt in (F.NV12, F.YUV420) and (d.Width | d.Height) & 1:
            raise ValueError(f"{who}: surface {i}: {fmt.name} is 4:2:0 and needs an even width and height, "
                             f"got {d.Width}x{d.Height}")
        on_device(who, i, d, gpu_id)
    return fmt


class PreparedBatch:
    """The base of every prepared batch.  A subclass names in `_owned` the device arrays it allocates; every other d_*
    attribute is the caller's memory and is never freed here.  Nothing is set up by the class itself, so an object that
    was never initialised, or only in part, tears down in silence."""

    _owned = ()

    def _begin(self, gpu_id, stream, hint, frames=None, rects=0, colours=False):
        """What a constructor calls after all its host-side checks and before its first allocation.  `hint` names the
        Prepare call in the refusal; None: this batch allocates nothing, so there is nothing to refuse.
        `frames`: the surfaces the batch draws on or reads -- their sizes, descriptors and the descriptors' device copy.
        `rects`: the number of records of the staging buffer that run_rects uploads host `rects` into.
        `colours`: the batch takes colours through run_colours."""
        if hint is not None and is_capturing(gpu_id, stream):
            # the uploads allocate and synchronise: both are illegal while the stream records a graph, and the recorded
            # launches would keep reading arrays that die with this object
            raise RuntimeError(f"{type(self).__name__}: cannot be created while the stream is capturing -- {hint} "
                               "before the StreamCapture block and Keep() the batch with the capture")
        self.gpu_id, self._stream = gpu_id, stream
        for name in self._owned:      # a constructor that fails half-way tears down what it got so far
            setattr(self, name, 0)
        if colours:
            self._colours_keep, self._colours = {}, {}        # run_colours: the device tensors, the last host colours
        if frames is not None:
            self.sizes = [(d.Width, d.Height) for d in frames]
            self.descs = [d.desc() for d in frames]
            if frames:
                self.d_frames = shim.descs_upload(gpu_id, self.descs, stream)
        if rects:
            self._rects_keep = None
            self.d_rects = shim.mem_alloc(gpu_id, 32 * rects)

    def __len__(self):
        return self.n

    def __del__(self):
        _release(self, self._owned)
