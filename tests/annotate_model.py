"""Model of vali_annotate_batch / PySurfaceAnnotator (include/vali_hip.h, "marks on frames"): numpy and Python integers,
marks applied one after another, each to the result of the one before.

A frame is its flat, tightly packed host image (Surface.HostSize layout); channels() gives writable 2-D views of it,
one per stored channel, so a mark is a handful of slice operations per channel.
"""
import numpy as np

FORMATS = ("NV12", "YUV420", "YUV444", "RGB", "BGR", "RGB_PLANAR")
YUV = ("NV12", "YUV420", "YUV444")
S420 = ("NV12", "YUV420")
NONE, BOX, FILL, PIXELATE = 0, 1, 2, 3
CELLS = (4, 8, 16, 32)
TILE = 64          # the kernel's tile side (vali_amd/csrc/tile_paint.hpp: kTile)
MAX_MARKS = 4096


def host_size(fmt, w, h):
    return w * h * 3 // 2 if fmt in S420 else w * h * 3


def channels(fmt, flat, w, h):
    """[(2-D view, shift, colour index)]: the stored channels of a flat host image; colour index 0, 1, 2 = r, g, b or
    Y, U, V; shift 1 = a 4:2:0 chroma channel"""
    assert flat.size == host_size(fmt, w, h) and flat.dtype == np.uint8
    if fmt in ("RGB", "BGR"):
        px = flat.reshape(h, w, 3)
        order = (0, 1, 2) if fmt == "RGB" else (2, 1, 0)          # a BGR surface stores b first
        return [(px[:, :, k], 0, order[k]) for k in range(3)]
    if fmt in ("RGB_PLANAR", "YUV444"):
        return [(flat[c * w * h:(c + 1) * w * h].reshape(h, w), 0, c) for c in range(3)]
    y = flat[:w * h].reshape(h, w)
    if fmt == "NV12":
        uv = flat[w * h:].reshape(h // 2, w // 2, 2)
        return [(y, 0, 0), (uv[:, :, 0], 1, 1), (uv[:, :, 1], 1, 2)]
    c = (w // 2) * (h // 2)
    return [(y, 0, 0), (flat[w * h:w * h + c].reshape(h // 2, w // 2), 1, 1), (flat[w * h + c:].reshape(h // 2, w // 2), 1, 2)]


def pack_colour(r, g, b, a=255):
    v = a << 24 | r << 16 | g << 8 | b
    return v - (1 << 32) if v >= 1 << 31 else v


def unpack_colour(colour):
    v = colour & 0xFFFFFFFF
    return (v >> 16) & 255, (v >> 8) & 255, v & 255, v >> 24


def yuv_of(r, g, b, rows):
    """the Y, U, V PySurfacePostprocessor writes into a YUV444 surface for the uint8 pixel (r, g, b):
    sat_u8(rint(fmaf(kB, b, fmaf(kG, g, fmaf(kR, r, offset))))) -- each fmaf is exact in float64 and rounded to float32 once"""
    out = []
    for k in range(3):
        m = [np.float32(v) for v in rows[k]]
        acc = m[3]
        for coef, v in ((m[0], r), (m[1], g), (m[2], b)):
            acc = np.float32(np.float64(coef) * np.float64(v) + np.float64(acc))
        out.append(int(np.clip(np.rint(acc), 0, 255)))
    return tuple(out)


def resolve(row, n, sizes, fmt):
    """None for a row that is skipped; else (frame, kind, (x0, y0, x1, y1), t or cell): the rectangle after snapping,
    UNCLIPPED, as Python integers"""
    frame, x, y, w, h, kind, arg, _ = (int(v) for v in row)
    if kind not in (BOX, FILL, PIXELATE) or not 0 <= frame < n or w < 1 or h < 1:
        return None
    if (kind == BOX and arg < 1) or (kind == PIXELATE and arg not in CELLS):
        return None
    x0, y0, x1, y1 = x, y, x + w, y + h
    if fmt in S420:
        x0, y0, x1, y1 = x0 & ~1, y0 & ~1, (x1 + 1) & ~1, (y1 + 1) & ~1
        if kind == BOX:
            arg = (arg + 1) & ~1
    fw, fh = sizes[frame]
    if x0 >= fw or y0 >= fh or x1 <= 0 or y1 <= 0:
        return None
    return frame, kind, (x0, y0, x1, y1), arg


def _blend(view, sel, c, a):
    v = view[sel].astype(np.int64)
    view[sel] = ((v * (255 - a) + c * a + 127) // 255).astype(np.uint8)


def apply_mark(flat, fmt, w, h, kind, rect, arg, colour, rows=None):
    """one resolved mark onto one frame, in place"""
    x0, y0, x1, y1 = rect
    r, g, b, a = unpack_colour(colour)
    col = yuv_of(r, g, b, rows) if fmt in YUV else (r, g, b)
    for view, sh, ci in channels(fmt, flat, w, h):
        pw, ph = w >> sh, h >> sh
        # 4:2:0 rectangles are even after snapping, so the chroma rectangle is exactly half
        cx0, cy0, cx1, cy1 = max(x0 >> sh, 0), max(y0 >> sh, 0), min(x1 >> sh, pw), min(y1 >> sh, ph)
        if kind == FILL:
            _blend(view, (slice(cy0, cy1), slice(cx0, cx1)), col[ci], a)
        elif kind == BOX:
            t = arg >> sh
            yy, xx = np.mgrid[cy0:cy1, cx0:cx1]
            inner = (xx >= (x0 >> sh) + t) & (xx < (x1 >> sh) - t) & (yy >= (y0 >> sh) + t) & (yy < (y1 >> sh) - t)
            sub = view[cy0:cy1, cx0:cx1]
            _blend(sub, ~inner, col[ci], a)
        else:
            s = arg >> sh
            gx0, gy0 = cx0 // s * s, cy0 // s * s
            gx1, gy1 = min(-(-cx1 // s) * s, pw), min(-(-cy1 // s) * s, ph)
            for by in range(gy0, gy1, s):
                for bx in range(gx0, gx1, s):
                    cell = view[by:min(by + s, ph), bx:min(bx + s, pw)]
                    cnt = cell.size
                    cell[...] = (int(cell.sum(dtype=np.int64)) + cnt // 2) // cnt


def apply(frames, fmt, sizes, marks, rows=None):
    """`marks` (rows of 8 integers) onto `frames` (flat host images, changed in place), in row order; returns the indices
    of the rows that were not skipped"""
    drawn = []
    for i, row in enumerate(marks):
        res = resolve(row, len(frames), sizes, fmt)
        if res is None:
            continue
        frame, kind, rect, arg = res
        apply_mark(frames[frame], fmt, sizes[frame][0], sizes[frame][1], kind, rect, arg, int(row[7]), rows)
        drawn.append(i)
    return drawn


def noise_frame(fmt, w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, host_size(fmt, w, h), dtype=np.uint8)


def plane_shapes(fmt, w, h):
    """(rows, bytes per row) of each plane as the surface stores them, in host-image order"""
    if fmt in ("RGB", "BGR"):
        return [(h, 3 * w)]
    if fmt == "RGB_PLANAR":
        return [(3 * h, w)]
    if fmt == "YUV444":
        return [(h, w)] * 3
    if fmt == "NV12":
        return [(h * 3 // 2, w)]
    return [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
