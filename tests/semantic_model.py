"""Model of vali_semantic_paint / PySemanticPainter (include/vali_hip.h, "semantic maps"): numpy float32 with one rounding
per operation, and Python integers, written from the definition.

`logits` (N, C, Hs, Ws) is a float32 array (holding exactly the values of a float16 / bfloat16 tensor where the GPU gets
one; N may be 1: a broadcast), `rects` rows of 8 integers (src_x, src_y, src_w, src_h, dst_x, dst_y, dst_w, dst_h).  A frame
is its flat, tightly packed host image (annotate_model.channels gives the views); a label map is an (H, W) uint8 array.
"""
import numpy as np

import annotate_model as am
import mask_model as mm

F32 = np.float32
OUTSIDE = 255
TILE, PASS_ROWS, STAGE_CELLS = 64, 32, 8192          # vali_amd/csrc/semantic.hip: kTile, kPassRows, kStage


def region(rect, size):
    """steps 1 and 2: None for a skipped record or an empty intersection, else (x0, y0, x1, y1) inside the frame"""
    sx, sy, sw, sh, _, _, dw, dh = (int(v) for v in rect)
    if min(sw, sh, dw, dh) < 1:
        return None
    W, H = size
    x0, y0, x1, y1 = max(sx, 0), max(sy, 0), min(sx + sw, W), min(sy + sh, H)
    return (x0, y0, x1, y1) if x0 < x1 and y0 < y1 else None


def values(planes, box, rect, net_size):
    """step 3 for the pixels of `box`: v (C, y1 - y0, x1 - x0) float32 of the planes (C, Hs, Ws)"""
    x0, y0, x1, y1 = box
    _, hs, ws = planes.shape
    sx, sy, sw, sh, dx, dy, dw, dh = (int(v) for v in rect)
    ix0, ix1, tx = mm.taps(np.arange(x0, x1), sx, sw, dx, dw, ws, net_size[0])
    iy0, iy1, ty = mm.taps(np.arange(y0, y1), sy, sh, dy, dh, hs, net_size[1])
    L = planes.astype(F32)
    with np.errstate(all="ignore"):
        def lerp(rows):
            a, b = L[:, rows][:, :, ix0], L[:, rows][:, :, ix1]
            return (a + (tx[None, None, :] * (b - a).astype(F32)).astype(F32)).astype(F32)
        top, bot = lerp(iy0), lerp(iy1)
        return (top + (ty[None, :, None] * (bot - top).astype(F32)).astype(F32)).astype(F32)


def classes(v):
    """step 4 on v (C, h, w): the label of every pixel"""
    with np.errstate(invalid="ignore"):
        if v.shape[0] == 1:
            return (v[0] > 0).astype(np.uint8)               # a NaN and -0.0 are not above 0
        best = np.full(v.shape[1:], -np.inf, F32)
        label = np.zeros(v.shape[1:], np.uint8)
        for c in range(v.shape[0]):
            win = v[c] > best                                 # the lowest class wins ties, a NaN never wins
            best = np.where(win, v[c], best)
            label[win] = c
        return label


def label_map(planes, size, rect, net_size):
    """steps 1 to 4 and 6: the (H, W) uint8 labels of one frame, 255 outside the region"""
    W, H = size
    out = np.full((H, W), OUTSIDE, np.uint8)
    box = region(rect, size)
    if box is not None:
        x0, y0, x1, y1 = box
        out[y0:y1, x0:x1] = classes(values(planes, box, rect, net_size))
    return out


def blend(flat, fmt, w, h, labels, colours, alpha, rows=None):
    """step 5: the classes of one label map onto one frame, in place, ascending"""
    for c in sorted(set(np.unique(labels).tolist()) - {OUTSIDE}):
        r, g, b, a = am.unpack_colour(mm.colour_of(c, colours, alpha))
        col = am.yuv_of(r, g, b, rows) if fmt in am.YUV else (r, g, b)
        on = (labels == c).astype(np.int64)
        for view, sh, ci in am.channels(fmt, flat, w, h):
            if sh:
                count = on[0::2, 0::2] + on[0::2, 1::2] + on[1::2, 0::2] + on[1::2, 1::2]
                k = (255 * count + 2) >> 2
            else:
                k = 255 * on
            ae = (k * a + 127) // 255
            v = view.astype(np.int64)
            view[...] = ((v * (255 - ae) + col[ci] * ae + 127) // 255).astype(np.uint8)


def apply(frames, fmt, sizes, logits, rects, colours, alpha, net_size, rows=None):
    """the whole call: paints `frames` in place (colours None: not at all) and returns the label map of every frame"""
    out = []
    for i, size in enumerate(sizes):
        planes = logits[i if logits.shape[0] > 1 else 0]
        labels = label_map(planes, size, rects[i], net_size)
        if colours is not None:
            blend(frames[i], fmt, size[0], size[1], labels, colours, alpha, rows)
        out.append(labels)
    return out


def stamp_atlas(label_maps, colours, alpha):
    """the classes of the label maps as a coverage atlas (255 / 0, one under the other) and the STAMP rows that paint
    them, one per frame and class present, ascending: vali_annotate_batch_atlas with these gives the same frames"""
    pieces, marks, v = [], [], 0
    for i, labels in enumerate(label_maps):
        for c in sorted(set(np.unique(labels).tolist()) - {OUTSIDE}):
            ys, xs = np.nonzero(labels == c)
            x0, y0, x1, y1 = int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1
            pieces.append((labels[y0:y1, x0:x1] == c).astype(np.uint8) * 255)
            arg = v << 16
            marks.append((i, x0, y0, x1 - x0, y1 - y0, 4, arg - (1 << 32) if arg >= 1 << 31 else arg,
                          mm.colour_of(c, colours, alpha)))
            v += y1 - y0
    assert v <= 65535 and len(marks) <= am.MAX_MARKS
    atlas = np.zeros((max(v, 1), max([p.shape[1] for p in pieces] + [1])), np.uint8)
    v = 0
    for p in pieces:
        atlas[v:v + p.shape[0], :p.shape[1]] = p
        v += p.shape[0]
    return atlas, marks


def tile_paths(size, rect, hs, ws, net_size):
    """{(tile x, tile y, pass): "staged" | "direct"} for every pass (32 rows of a 64 x 64 tile) that holds a region
    pixel, by the kernel's footprint rule: staged when the logits cells its pixels sample, at an odd row pitch, fit the
    LDS stage"""
    box = region(rect, size)
    out = {}
    if box is None:
        return out
    x0, y0, x1, y1 = box
    sx, sy, sw, sh, dx, dy, dw, dh = (int(v) for v in rect)
    for ty in range(0, size[1], TILE):
        for tx in range(0, size[0], TILE):
            cx0, cx1 = max(x0, tx), min(x1, tx + TILE)
            if cx0 >= cx1:
                continue
            i0, i1, _ = mm.taps(np.array([cx0, cx1 - 1]), sx, sw, dx, dw, ws, net_size[0])
            fw = int(i1[1]) - int(i0[0]) + 1
            for p, py in enumerate(range(ty, ty + TILE, PASS_ROWS)):
                cy0, cy1 = max(y0, py), min(y1, py + PASS_ROWS)
                if cy0 >= cy1:
                    continue
                j0, j1, _ = mm.taps(np.array([cy0, cy1 - 1]), sy, sh, dy, dh, hs, net_size[1])
                fh = int(j1[1]) - int(j0[0]) + 1
                out[(tx // TILE, ty // TILE, p)] = "staged" if fh * (fw | 1) <= STAGE_CELLS else "direct"
    return out
