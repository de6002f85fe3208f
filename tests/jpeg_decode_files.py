"""JPEG files for the decoder tests: Pillow's encoder (any sampling it writes, restart markers through
restart_marker_blocks), and tests/jpeg_model.py's encoder for what Pillow cannot write (4:4:0, any restart interval)."""
from __future__ import annotations

import io

import numpy as np

import jpeg_model as jm

SAMPLINGS = ("444", "422", "420", "440", "gray")
_PIL_SUB = {"444": 0, "422": 1, "420": 2}


def picture(w, h, content="frame", seed=0, frame=None):
    rng = np.random.default_rng(seed)
    if content == "noise" or frame is None:
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    fh, fw = frame.shape[:2]
    return np.ascontiguousarray(np.tile(np.roll(frame, 31 * seed, 1), (-(-h // fh), -(-w // fw), 1))[:h, :w])


def pillow_file(rgb, sampling, quality, restart_blocks=0):
    from PIL import Image

    out = io.BytesIO()
    kw = {"restart_marker_blocks": restart_blocks} if restart_blocks else {}
    if sampling == "gray":
        Image.fromarray(rgb).convert("L").save(out, "JPEG", quality=quality, **kw)
    else:
        Image.fromarray(rgb).save(out, "JPEG", quality=quality, subsampling=_PIL_SUB[sampling], **kw)
    return out.getvalue()


def model_file(rgb, H, V, quality, R=0):
    """jpeg_model's encoder with luma sampling (H, V), chroma subsampled by taking every H-th / V-th sample"""
    h, w = rgb.shape[:2]
    y, u, v = jm.rgb_to_ycc(rgb)
    cw, ch = -(-w // H), -(-h // V)
    planes = [y, u[::V, ::H][:ch, :cw], v[::V, ::H][:ch, :cw]]
    saved = jm.sampling
    jm.sampling = lambda fmt: (H, V)
    try:
        coefs, comp, bpm = jm.scan_blocks(jm.YUV444, planes, w, h, quality)
        return jm.header(w, h, jm.YUV444, quality, R) + jm.huffman(coefs, comp, bpm, R) + b"\xff\xd9"
    finally:
        jm.sampling = saved


def make_file(sampling, w, h, quality, content="frame", seed=0, frame=None, restart=False):
    """a file of that sampling; restart=True: restart markers (Pillow: every 2 MCU rows' worth of blocks;
    4:4:0: the model's encoder, 1 MCU per interval)"""
    rgb = picture(w, h, content, seed, frame)
    if sampling == "440":
        return model_file(rgb, 1, 2, quality, R=1 if restart else 0)
    return pillow_file(rgb, sampling, quality, restart_blocks=7 if restart else 0)
