"""Model of vali_mask_paint / PyInstanceMasker (include/vali_hip.h, "instance masks"): numpy float32 with one rounding per
operation, and Python integers, written from the definition.

`protos` (N, M, Hp, Wp) and `coeffs` (N, K, M) are float32 arrays (holding exactly the values of a float16 / bfloat16
tensor where the GPU gets one; N may be 1 for protos: a broadcast), `dets` rows of 8 integers, `rects` rows of 8 integers
(src_x, src_y, src_w, src_h, dst_x, dst_y, dst_w, dst_h).  A frame is its flat, tightly packed host image
(annotate_model.channels gives the views).
"""
import numpy as np

import annotate_model as am

F32 = np.float32


def logits(coeffs_row, protos_i):
    """step 2: L (Hp, Wp) float32; the product and the sum rounded separately, m ascending"""
    acc = np.zeros(protos_i.shape[1:], F32)
    with np.errstate(all="ignore"):
        for m in range(protos_i.shape[0]):
            acc = (acc + (F32(coeffs_row[m]) * protos_i[m].astype(F32)).astype(F32)).astype(F32)
    return acc


def taps(px, src, src_n, dst, dst_n, P, net):
    """step 3 along one axis for the integer pixel positions `px` (an int array): (i0, i1, t)"""
    px = np.asarray(px, np.int64)
    scale = F32(F32(dst_n) / F32(src_n))
    k = F32(F32(P) / F32(net))
    g = (((px.astype(F32) + F32(0.5)).astype(F32) - F32(src)).astype(F32) * scale).astype(F32)
    g = (g + F32(dst)).astype(F32)
    f = ((g * k).astype(F32) - F32(0.5)).astype(F32)
    x0 = np.floor(f).astype(F32)
    t = (f - x0).astype(F32)
    i = np.clip(x0, F32(-1), F32(P)).astype(np.int64)
    return np.clip(i, 0, P - 1), np.clip(i + 1, 0, P - 1), t


def resolve(row, i, size, K, rect):
    """step 1: None for a row that is skipped, else the box clipped to the frame (x0, y0, x1, y1)"""
    frame, x, y, w, h, _, _, k = (int(v) for v in row)
    if frame != i or w < 1 or h < 1 or not 0 <= k < K:
        return None
    if min(int(rect[2]), int(rect[3]), int(rect[6]), int(rect[7])) < 1:
        return None
    W, H = size
    if x >= W or y >= H or x + w <= 0 or y + h <= 0:
        return None
    return max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)


def sample(L, box, rect, net_size):
    """steps 3 and 4 for the pixels of the clipped box: (v, used) -- v the interpolated logits (y1 - y0, x1 - x0) float32,
    used the prototype range (c0, c1, r0, r1) the box reads, ends included"""
    x0, y0, x1, y1 = box
    hp, wp = L.shape
    sx, sy, sw, sh, dx, dy, dw, dh = (int(v) for v in rect)
    ix0, ix1, tx = taps(np.arange(x0, x1), sx, sw, dx, dw, wp, net_size[0])
    iy0, iy1, ty = taps(np.arange(y0, y1), sy, sh, dy, dh, hp, net_size[1])
    with np.errstate(all="ignore"):
        def lerp(rows):
            a, b = L[rows][:, ix0], L[rows][:, ix1]
            return (a + (tx[None, :] * (b - a).astype(F32)).astype(F32)).astype(F32)
        top, bot = lerp(iy0), lerp(iy1)
        v = (top + (ty[:, None] * (bot - top).astype(F32)).astype(F32)).astype(F32)
    return v, (int(ix0.min()), int(ix1.max()), int(iy0.min()), int(iy1.max()))


def row_mask(row, i, size, protos, coeffs, rect, net_size):
    """None for a skipped row, else (box, inside): inside a bool array over the clipped box (steps 1 to 5)"""
    box = resolve(row, i, size, coeffs.shape[1], rect)
    if box is None:
        return None
    pi = protos[i if protos.shape[0] > 1 else 0]
    L = logits(coeffs[i, int(row[7])], pi)
    v, _ = sample(L, box, rect, net_size)
    with np.errstate(invalid="ignore"):
        return box, v > 0            # a NaN is never in


def colour_of(cls, colours, alpha):
    """the packed colour of class `cls` with `alpha` (None: its own)"""
    c = int(colours[int(cls) % len(colours)]) & 0xFFFFFFFF        # Python's %: the non-negative remainder
    if alpha is not None:
        c = (c & 0x00FFFFFF) | int(alpha) << 24
    return c - (1 << 32) if c >= 1 << 31 else c


def blend(flat, fmt, w, h, box, inside, colour, rows=None):
    """step 6: one mask onto one frame, in place"""
    r, g, b, a = am.unpack_colour(colour)
    col = am.yuv_of(r, g, b, rows) if fmt in am.YUV else (r, g, b)
    cov = np.zeros((h, w), np.int64)
    x0, y0, x1, y1 = box
    cov[y0:y1, x0:x1] = inside.astype(np.int64) * 255
    for view, sh, ci in am.channels(fmt, flat, w, h):
        k = cov if not sh else (cov[0::2, 0::2] + cov[0::2, 1::2] + cov[1::2, 0::2] + cov[1::2, 1::2] + 2) >> 2
        ae = (k * a + 127) // 255
        v = view.astype(np.int64)
        view[...] = ((v * (255 - ae) + col[ci] * ae + 127) // 255).astype(np.uint8)


def apply(frames, fmt, sizes, dets, D, protos, coeffs, rects, colours, alpha, net_size, rows=None):
    """the masks of `dets` ((N * D) rows) onto `frames`, in row order; returns [(row index, box, inside, colour)] of the
    rows that were not skipped"""
    drawn = []
    for i in range(len(frames)):
        for r in range(D):
            row = dets[i * D + r]
            got = row_mask(row, i, sizes[i], protos, coeffs, rects[i], net_size)
            if got is None:
                continue
            box, inside = got
            colour = colour_of(row[5], colours, alpha)
            blend(frames[i], fmt, sizes[i][0], sizes[i][1], box, inside, colour, rows)
            drawn.append((i * D + r, box, inside, colour))
    return drawn


def stamp_atlas(drawn, dets):
    """the masks of apply() as a coverage atlas (255 / 0, one under the other) and the STAMP rows that paint them:
    vali_annotate_batch_atlas with these gives the same frames (step 7)"""
    width = max([b[2] - b[0] for _, b, _, _ in drawn] + [1])
    height = sum(b[3] - b[1] for _, b, _, _ in drawn)
    assert height <= 65535
    atlas = np.zeros((max(height, 1), width), np.uint8)
    marks, v = [], 0
    for idx, (x0, y0, x1, y1), inside, colour in drawn:
        atlas[v:v + y1 - y0, :x1 - x0] = inside.astype(np.uint8) * 255
        arg = v << 16
        marks.append((int(dets[idx][0]), x0, y0, x1 - x0, y1 - y0, 4, arg - (1 << 32) if arg >= 1 << 31 else arg, colour))
        v += y1 - y0
    return atlas, marks
