"""The argument rules the tasks fed by a network's head share, each stated once.  At Prepare time: the number of frames,
`max_det` and `net_size`; at Run time: `kpt_thr`, and `rects`, colours and `alpha`, each as a device tensor or as host
values."""
from __future__ import annotations

import math
import operator

from ._native import shim
from .runtime import is_capturing
from .tensors import device_i32, is_device, upload_i32

MAX_FRAMES, MAX_NET = 1024, 65535


def batch_size(n, who=None):
    """the N of the head tensor `who`, or the number of frames: 1..MAX_FRAMES"""
    if not 1 <= n <= MAX_FRAMES:
        raise ValueError(f"{who}: N = {n} is outside 1..{MAX_FRAMES}" if who else
                         f"frames: {n} surfaces; need 1..{MAX_FRAMES}")


def max_det_arg(max_det, n, most, most_text=None, cap=65535, slots=None):
    """`max_det` as an integer D in 1..most (`most_text`: how the message names that bound) with N * D <= cap (None: no
    cap).  `slots` = (who, M, what they are): the tensor `who` has one slot per detection, M = N * D."""
    D = operator.index(max_det)
    if not 1 <= D <= most:
        raise ValueError(f"max_det = {D} is outside 1..{most_text or most}")
    if cap is not None and n * D > cap:
        raise ValueError(f"N * max_det = {n * D} exceeds {cap}")
    if slots is not None:
        who, m, what = slots
        if m != n * D:
            raise ValueError(f"{who}: M = {m} slots for N * max_det = {n} * {D} = {n * D}{what}")
    return D


def net_size_arg(net_size):
    """(width, height) of the network's input, each 1..MAX_NET"""
    try:
        net_w, net_h = (operator.index(v) for v in net_size)
    except (TypeError, ValueError):
        raise ValueError("net_size: two integers (width, height) of the network's input") from None
    if not (1 <= net_w <= MAX_NET and 1 <= net_h <= MAX_NET):
        raise ValueError(f"net_size = ({net_w}, {net_h}) is outside 1..{MAX_NET}")
    return net_w, net_h


def kpt_thr_arg(kpt_thr):
    thr = float(kpt_thr)
    if math.isnan(thr):
        raise ValueError("kpt_thr must not be a NaN")
    return thr


def device_rects(rects, n, gpu_id):
    """(device pointer, holder) of the (n, 8) int32 records of a batch on `gpu_id`, as a device tensor"""
    ptr, _, holder = device_i32("rects", rects, (n, 8), gpu_id, "the batch", f"({n}, 8)", dlpack_got=False)
    return ptr, holder


def host_rects(rects, n):
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


def run_rects(batch, rects, gpu_id, stream):
    """the device pointer of `rects` for one Run: a device tensor, which `batch` then keeps alive, or host rows, uploaded
    into the batch's staging buffer with one blocking copy"""
    if is_device(rects):
        d_rects, batch._rects_keep = device_rects(rects, batch.n, gpu_id)
        return d_rects
    return upload_i32(gpu_id, stream, [v for r in host_rects(rects, batch.n) for v in r], batch.d_rects)


def alpha_arg(alpha):
    """`alpha` as the C ABI takes it: None -> -1 (the colours' own), else 0..255"""
    if alpha is None:
        return -1
    a = operator.index(alpha)
    if not 0 <= a <= 255:
        raise ValueError(f"alpha = {a} is outside 0..255 (None keeps the colours' own)")
    return a


def host_colours(name, colours):
    """None for a device tensor, else the packed colours of a host sequence"""
    if is_device(colours):
        return None
    try:
        host = [operator.index(v) for v in colours]
    except TypeError:
        raise ValueError(f"{name}: an int32 device tensor or a sequence of packed colours (pack_colour)") from None
    if not host:
        raise ValueError(f"{name}: at least one colour")
    if any(not -(1 << 31) <= v < (1 << 31) for v in host):
        raise ValueError(f"{name}: every colour must fit an int32 (pack_colour)")
    return host


def run_colours(task, batch, name, colours, host, gpu_id, stream):
    """(device pointer, count) of the colours `name` for one Run.  A device tensor (`host` is None) is checked and kept
    alive in batch._colours_keep[name]; host colours are uploaded when they differ from batch._colours[name], into
    memory the batch owns as d_<name>."""
    attr = "d_" + name
    if host is None:
        dc, (nc,), batch._colours_keep[name] = device_i32(name, colours, (None,), gpu_id, want="(n,), n >= 1")
        return dc, nc
    if batch._colours.get(name) != host:
        if is_capturing(gpu_id, stream):
            raise RuntimeError(f"{task}: host {name} cannot be uploaded while the stream is capturing -- Run once with "
                               "them before the capture, or pass a device tensor")
        shim.stream_sync(gpu_id, stream)      # a launch may still read the colours it replaces
        if getattr(batch, attr):
            shim.mem_free(gpu_id, getattr(batch, attr))
            setattr(batch, attr, 0)
        setattr(batch, attr, upload_i32(gpu_id, stream, host))
        batch._colours[name] = host
    return getattr(batch, attr), len(host)
