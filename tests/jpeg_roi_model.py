"""The files of PyNvJpegEncoder.RunRoi, for the tests only: crop the host image, then the model of the whole-surface
encoder for that crop (tests/jpeg_model.py, jpeg_subsample_model.py, jpeg_optimize_model.py, each pinned to Pillow).
Nothing here knows how the GPU encoder finds its rectangle."""
from __future__ import annotations

import numpy as np

import jpeg_model as jm
import jpeg_optimize_model as om
import jpeg_subsample_model as sm

RGB_FORMATS = (jm.RGB, jm.BGR, jm.RGB_PLANAR)


def crop(fmt, host, sw, sh, rect):
    """rectangle (x, y, w, h) of a tightly packed sw x sh host image of `fmt`, as a tightly packed w x h one"""
    x, y, w, h = rect
    host = np.asarray(host, np.uint8).reshape(-1)
    if fmt in (jm.RGB, jm.BGR):
        return np.ascontiguousarray(host.reshape(sh, sw, 3)[y:y + h, x:x + w]).reshape(-1)
    if fmt == jm.RGB_PLANAR:
        return np.ascontiguousarray(host.reshape(3, sh, sw)[:, y:y + h, x:x + w]).reshape(-1)
    dx, dy = {jm.YUV444: (1, 1), jm.YUV422: (2, 1), jm.YUV420: (2, 2)}[fmt]
    assert x % dx == 0 and w % dx == 0 and y % dy == 0 and h % dy == 0, (fmt, rect)
    cw, ch = jm.chroma_size(fmt, sw, sh)
    luma = host[:sw * sh].reshape(sh, sw)[y:y + h, x:x + w]
    chroma = host[sw * sh:].reshape(2, ch, cw)[:, y // dy:(y + h) // dy, x // dx:(x + w) // dx]
    return np.concatenate([luma.reshape(-1), chroma.reshape(-1)])


def encode_crop(fmt, host, w, h, quality, samp=None, optimize=False):
    """the file of a whole w x h image: what Run writes with Context(quality, fmt, samp, optimize)"""
    if optimize:
        return om.encode(fmt, host, w, h, quality, samp)
    if fmt in RGB_FORMATS:
        return sm.encode(fmt, host, w, h, quality, samp or "444")
    return jm.encode(fmt, host, w, h, quality)


def encode(fmt, host, sw, sh, rect, quality, samp=None, optimize=False):
    """file of rectangle `rect` (None: the whole image) of the sw x sh host image"""
    rect = (0, 0, sw, sh) if rect is None else rect
    return encode_crop(fmt, crop(fmt, host, sw, sh, rect), rect[2], rect[3], quality, samp, optimize)
