"""Model of MARK_STAMP (include/vali_hip.h, "marks on frames": stamps) on top of tests/annotate_model.py: numpy and Python
integers, written from the definition.  `atlas` is a 2-D uint8 array (AH, AW) or None (no atlas: kind 4 is unknown)."""
import numpy as np

import annotate_model as am

STAMP = 4


def pack_uv(u, v):
    a = u | v << 16
    return a - (1 << 32) if a >= 1 << 31 else a


def unpack_uv(arg):
    a = int(arg) & 0xFFFFFFFF
    return a & 0xFFFF, (a >> 16) & 0xFFFF


def resolve(row, n, sizes, fmt, atlas=None):
    """None for a row that is skipped; for a stamp (frame, STAMP, (x0, y0, x1, y1), (u, v)) -- the rectangle as given,
    NOT snapped; the other kinds as annotate_model.resolve"""
    frame, x, y, w, h, kind, arg, _ = (int(v) for v in row)
    if kind != STAMP:
        return am.resolve(row, n, sizes, fmt)
    if atlas is None or not 0 <= frame < n or w < 1 or h < 1:
        return None
    u, v = unpack_uv(arg)
    if u >= atlas.shape[1] or v >= atlas.shape[0]:
        return None
    fw, fh = sizes[frame]
    if x >= fw or y >= fh or x + w <= 0 or y + h <= 0:
        return None
    return frame, STAMP, (x, y, x + w, y + h), (u, v)


def coverage(atlas, rect, uv, fw, fh):
    """cov(px, py) of every pixel of a fw x fh frame, as an (fh, fw) int64 array"""
    x0, y0, x1, y1 = rect
    u, v = uv
    ah, aw = atlas.shape
    cov = np.zeros((fh, fw), np.int64)
    # 0 <= dx < w, u + dx < AW, and the pixel is in the frame
    px0, px1 = max(x0, 0), min(x1, x0 + (aw - u), fw)
    py0, py1 = max(y0, 0), min(y1, y0 + (ah - v), fh)
    if px0 < px1 and py0 < py1:
        cov[py0:py1, px0:px1] = atlas[v + py0 - y0:v + py1 - y0, u + px0 - x0:u + px1 - x0]
    return cov


def weights(cov, sh):
    """the weight k of every sample of a plane at shift sh"""
    if not sh:
        return cov
    return (cov[0::2, 0::2] + cov[0::2, 1::2] + cov[1::2, 0::2] + cov[1::2, 1::2] + 2) >> 2


def apply_stamp(flat, fmt, w, h, rect, uv, colour, atlas, rows=None):
    r, g, b, a = am.unpack_colour(colour)
    col = am.yuv_of(r, g, b, rows) if fmt in am.YUV else (r, g, b)
    cov = coverage(atlas, rect, uv, w, h)
    for view, sh, ci in am.channels(fmt, flat, w, h):
        ae = (weights(cov, sh) * a + 127) // 255
        v = view.astype(np.int64)
        view[...] = ((v * (255 - ae) + col[ci] * ae + 127) // 255).astype(np.uint8)


def apply(frames, fmt, sizes, marks, rows=None, atlas=None):
    """annotate_model.apply with stamps: `marks` onto `frames` in row order; returns the indices of the rows drawn"""
    drawn = []
    for i, row in enumerate(marks):
        res = resolve(row, len(frames), sizes, fmt, atlas)
        if res is None:
            continue
        frame, kind, rect, arg = res
        fw, fh = sizes[frame]
        if kind == STAMP:
            apply_stamp(frames[frame], fmt, fw, fh, rect, arg, int(row[7]), atlas, rows)
        else:
            am.apply_mark(frames[frame], fmt, fw, fh, kind, rect, arg, int(row[7]), rows)
        drawn.append(i)
    return drawn
