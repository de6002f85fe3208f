"""A caller's device tensor as the tasks read it: one look through `__cuda_array_interface__` or `__dlpack__`, one rule for
the device it is on, the int32 and the float intake built on the two, the strided float layout the heads share, and the
one way host int32 values get to the device.  Surface.from_dlpack / from_cai (surface.py) mirror the reference's messages
and are not part of this.
"""
from __future__ import annotations

import array
from typing import NamedTuple, Optional

from ._native import shim
from .enums import DLDeviceType

# DLPack (code, bits) -> (name, enum vali_dtype): kDLInt = 0, kDLUInt = 1, kDLFloat = 2, kDLBfloat = 4
DTYPES = {(2, 32): ("float32", 0), (2, 16): ("float16", 1), (4, 16): ("bfloat16", 2), (1, 8): ("uint8", 3)}
FLOAT_DTYPES = {k: v for k, v in DTYPES.items() if k != (1, 8)}
_TYPESTRS = {"<f4": (2, 32), "<f2": (2, 16), "|u1": (1, 8), "<i4": (0, 32), "|i4": (0, 32)}      # bfloat16 has none
# device_float's last two arguments for a network head: float32 and float16 have a typestr
HEAD_CAI = (("<f4", "<f2"), " (bfloat16: __dlpack__)")
_GPUS = (int(DLDeviceType.kDLROCM), int(DLDeviceType.kDLCUDA))
_CAI, _DLPACK = "__cuda_array_interface__", "__dlpack__"


class Seen(NamedTuple):
    """what one look at a tensor gives, before anything is judged"""
    ptr: int
    code: Optional[int]          # DLPack dtype code and bits; None for a typestr this project has no use for
    bits: Optional[int]
    shape: tuple
    strides: Optional[tuple]     # in elements; None: compact row-major; None inside: no whole number of elements
    device: Optional[int]        # through __dlpack__: the device id, -1 off the GPU; None: for _device to find
    holder: object               # keeps the memory alive
    typestr: Optional[str]       # None through __dlpack__


def is_tensor(t):
    """speaks one of the two protocols, wherever it lives"""
    return hasattr(t, _CAI) or hasattr(t, _DLPACK)


def is_device(t):
    """a device tensor, as opposed to host values (numpy arrays speak DLPack too: theirs is the CPU's)"""
    if hasattr(t, _CAI):
        return True
    if hasattr(t, _DLPACK):
        where = getattr(t, "__dlpack_device__", None)
        return where is None or int(where()[0]) != int(DLDeviceType.kDLCPU)
    return False


def declared_shape(t):
    """the shape a tensor declares, for a check that needs a count before the tensor is read (SelectBatch's marks)"""
    return tuple(int(v) for v in (t.__cuda_array_interface__["shape"] if hasattr(t, _CAI) else getattr(t, "shape", ())))


def _see(who, t, cai_first):
    order = (_CAI, _DLPACK) if cai_first else (_DLPACK, _CAI)
    for protocol in order:
        how = getattr(t, protocol, None)      # one read: torch builds its __cuda_array_interface__ on every one
        if how is None:
            continue
        if protocol == _DLPACK:
            info, holder = shim.dlpack_import(how())
            if info["lanes"] != 1:
                raise ValueError(f"{who}: vector dtypes are not supported")
            device = int(info["device_id"]) if info["device_type"] in _GPUS else -1
            return Seen(int(info["ptr"]), info["code"], info["bits"], tuple(info["shape"]), tuple(info["strides"]),
                        device, holder, None)
        cai = how
        code, bits = _TYPESTRS.get(cai["typestr"], (None, None))
        strides = cai.get("strides") if bits else None
        if strides is not None:
            strides = tuple(None if int(v) % (bits // 8) else int(v) // (bits // 8) for v in strides)
        return Seen(int(cai["data"][0]), code, bits, tuple(int(v) for v in cai["shape"]), strides, None, t,
                    cai["typestr"])
    raise ValueError(f"{who}: a device tensor with {order[0]} or {order[1]}")


def _device(who, t, seen, gpu_id, on):
    """The one device rule: a DLPack tensor says where it is; otherwise a `.device` of type "cuda" with an integer
    index does, one of another type is not on the GPU, and the pointer is asked for everything else (a null pointer
    of no elements is wherever it is needed)."""
    device = seen.device
    if device is None:
        dev = getattr(t, "device", None)
        kind, index = getattr(dev, "type", None), getattr(dev, "index", None)
        if kind is not None and kind != "cuda":
            device = -1
        elif kind == "cuda" and isinstance(index, int):
            device = index
        else:
            device = shim.ptr_device(seen.ptr) if seen.ptr or 0 not in seen.shape else gpu_id
    if device < 0:
        raise ValueError(f"{who}: the tensor must live on the GPU")
    if device != gpu_id:
        raise ValueError(f"{who}: the tensor is on device {device}, {on} on {gpu_id}")


def device_i32(who, t, shape, gpu_id, on="the task", want=None, least=1, dlpack_got=True):
    """(device pointer, shape, holder) of a contiguous int32 device tensor of `shape` on `gpu_id`; a None in `shape`
    is a dimension of any size from `least`.  Shape, dtype, contiguity and device are all the host checks: the values
    are the kernels' to sanitise.  `want` words the shape and `on` the owner of `gpu_id` in the messages."""
    seen = _see(who, t, True)
    got = seen.shape
    if ((seen.code, seen.bits) != (0, 32) or len(got) != len(shape)
            or any(g < least if w is None else g != w for g, w in zip(got, shape))):
        want = want or "(" + "x".join(str(v) for v in shape) + ")"
        tail = f", got {seen.typestr} {got}" if seen.typestr else f", got shape {got}" if dlpack_got else ""
        raise ValueError(f"{who}: need an int32 tensor of shape {want}{tail}")
    if seen.strides is not None:
        expect = 1
        for size, st in zip(reversed(got), reversed(seen.strides)):
            if size > 1 and st != expect:
                raise ValueError(f"{who}: the tensor must be contiguous")
            expect *= size
    _device(who, t, seen, gpu_id, on)
    return seen.ptr, got, seen.holder


def device_float(who, t, layout_of, gpu_id, cai_types, hint=""):
    """(Seen, what layout_of(shape, strides in elements or None, DLPack code, bits) returned) of a device tensor on
    `gpu_id`; __dlpack__ first, because bfloat16 has no typestr.  `cai_types`: the typestrs taken through
    __cuda_array_interface__; `hint` follows them in the message."""
    seen = _see(who, t, False)
    if seen.typestr is not None:
        if seen.typestr not in cai_types:
            names = " or ".join(DTYPES[_TYPESTRS[v]][0] for v in cai_types)
            raise ValueError(f"{who}: the dtype must be {names} through __cuda_array_interface__{hint}, got {seen.typestr}")
        if seen.strides is not None and None in seen.strides:
            raise ValueError(f"{who}: strides that are no multiple of the element size")
    layout = layout_of(seen.shape, seen.strides, seen.code, seen.bits)
    _device(who, t, seen, gpu_id, "the task")
    return seen, layout


def strided_layout(who, dims, shape, strides, code, bits, limits=None):
    """a float32, float16 or bfloat16 view of len(dims) dimensions with element strides >= 0: (dtype code, shape,
    strides).  `limits(shape)`, if any, is asked after the rank and before the strides."""
    dtype = FLOAT_DTYPES.get((int(code), int(bits)))
    if dtype is None:
        raise ValueError(f"{who}: the dtype must be float32, float16 or bfloat16 (DLPack code {code}, {bits} bits)")
    shape = tuple(int(v) for v in shape)
    if len(shape) != len(dims):
        raise ValueError(f"{who}: need a {len(dims)}-D tensor ({', '.join(dims)}), got {len(shape)}-D {shape}")
    if limits is not None:
        limits(shape)
    if strides is None:
        strides, step = [], 1
        for size in reversed(shape):
            strides.insert(0, step)
            step *= size
    strides = tuple(int(v) for v in strides)
    if len(strides) != len(shape):
        raise ValueError(f"{who}: {len(strides)} strides for a {len(shape)}-D tensor")
    if any(v < 0 for v in strides):
        raise ValueError(f"{who}: negative strides {strides} (a flipped view) are not supported")
    if any(v > 1 << 40 for v in strides):
        raise ValueError(f"{who}: strides {strides} beyond 2^40 elements")
    return dtype[1], shape, strides


def upload_i32(gpu_id, stream, values, dst=0):
    """host int32 `values` on the device, at `dst` or in memory allocated here and now the caller's: one blocking copy
    on `stream`.  Returns the device pointer."""
    buf = array.array("i", values)
    nbytes = 4 * len(buf)
    if not dst:
        dst = shim.mem_alloc(gpu_id, nbytes)
    shim.memcpy2d_async(gpu_id, dst, nbytes, buf.buffer_info()[0], nbytes, nbytes, 1, 0, stream)
    shim.stream_sync(gpu_id, stream)      # `buf` goes with this call
    return dst
