"""The definition of vali_detect_select (include/vali_hip.h, "detections") restated in numpy float32: every operation is
one IEEE float32 operation, nothing is fused.  Inputs are float32 arrays (a float16 / bfloat16 head is converted first,
which is exact).  tests/test_detect_host.py checks this model against a second, scalar implementation; the GPU tests
compare the kernels with it bit for bit."""
import numpy as np

F = np.float32
MARK_BOX, MARK_FILL, MARK_STAMP = 1, 2, 4
I32_MAX = 2**31 - 1


def pack_colour(r, g, b, a=255):
    v = a << 24 | r << 16 | g << 8 | b
    return v - (1 << 32) if v >= 1 << 31 else v


def i32(v):
    """wrap to int32"""
    return np.asarray(v, np.int64).astype(np.uint32).view(np.int32) if np.ndim(v) else int(np.int64(v).astype(np.uint32).view(np.int32))


def frame_edges(rec):
    """(ok, dx, dy, dx2, dy2) of a record (src_x, src_y, src_w, src_h, dst_x, dst_y, dst_w, dst_h)"""
    sx, sy, sw, sh, dx, dy, dw, dh = (int(v) for v in rec)
    ok = sw >= 1 and sh >= 1 and dw >= 1 and dh >= 1
    return ok, F(dx), F(dy), F(dx + dw), F(dy + dh)


def candidates(boxes, scores, rec, score_thr, box_format, T):
    """steps 1-4 for one frame: (k, cls, s, box (n, 4)) of the candidates that go on, in order"""
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, F), np.zeros((0, 4), F))
    ok, dx, dy, dx2, dy2 = frame_edges(rec)
    if not ok:
        return empty
    v = np.where(np.isnan(scores), F(-np.inf), scores).astype(F)
    s, cls = v.max(1), v.argmax(1)
    b = boxes.astype(F)
    if box_format == "cxcywh":
        hw, hh = b[:, 2] * F(0.5), b[:, 3] * F(0.5)
        x1, x2, y1, y2 = b[:, 0] - hw, b[:, 0] + hw, b[:, 1] - hh, b[:, 1] + hh
    else:
        x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    x1, y1 = np.where(dx > x1, dx, x1), np.where(dy > y1, dy, y1)
    x2, y2 = np.where(dx2 < x2, dx2, x2), np.where(dy2 < y2, dy2, y2)
    box = np.stack([x1, y1, x2, y2], 1).astype(F)
    good = (s > F(score_thr)) & np.isfinite(box).all(1) & (x2 > x1) & (y2 > y1)
    k = np.flatnonzero(good)
    order = np.lexsort((k, -s[k]))[:T]          # -0.0 and 0.0 compare equal; equal scores by k
    k = k[order]
    return k, cls[k], s[k], box[k]


def suppression(box, cls, iou_thr, class_agnostic):
    """sup[i, j]: i suppresses j (were i kept); only i < j matters"""
    x1, y1, x2, y2 = (box[:, c] for c in range(4))
    iw = np.maximum(np.minimum(x2[:, None], x2[None, :]) - np.maximum(x1[:, None], x1[None, :]), F(0))
    ih = np.maximum(np.minimum(y2[:, None], y2[None, :]) - np.maximum(y1[:, None], y1[None, :]), F(0))
    inter = iw * ih
    a = (x2 - x1) * (y2 - y1)
    uni = (a[:, None] + a[None, :]) - inter
    sup = inter > F(iou_thr) * uni
    if not class_agnostic:
        sup &= cls[:, None] == cls[None, :]
    return sup


def nms(box, cls, iou_thr, class_agnostic, D):
    """indices of the first D kept"""
    sup = suppression(box, cls, iou_thr, class_agnostic)
    gone = np.zeros(len(box), bool)
    kept = []
    for i in range(len(box)):
        if gone[i]:
            continue
        kept.append(i)
        if len(kept) == D:
            break
        gone[i + 1:] |= sup[i, i + 1:]
    return np.asarray(kept, np.int64)


def to_pixels(box, rec):
    """step 6: (x, y, w, h) int64 arrays"""
    sx_, sy_, sw, sh, dx_, dy_, dw, dh = (int(v) for v in rec)
    sx, sy = F(sw) / F(dw), F(sh) / F(dh)
    out = []
    for lo, hi, d, s, o, span in ((0, 2, dx_, sx, sx_, sw), (1, 3, dy_, sy, sy_, sh)):
        a = np.floor((box[:, lo] - F(d)) * s + F(o))
        b = np.ceil((box[:, hi] - F(d)) * s + F(o))
        a = np.minimum(np.maximum(a, F(o)), F(o + span)).astype(np.int64)
        b = np.minimum(np.maximum(b, F(o)), F(o + span)).astype(np.int64)
        out.append((np.minimum(a, I32_MAX), np.minimum(np.maximum(b - a, 1), I32_MAX)))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def score_bits(s):
    s = np.asarray(s, F).copy()
    s[s == 0] = 0.0
    return s.view(np.int32)


def select(boxes, scores, rects, score_thr=0.25, iou_thr=0.45, class_agnostic=False, box_format="xyxy", T=1024, D=100):
    """(dets (N * D, 8) int32, counts (N,) int32)"""
    boxes, scores = np.asarray(boxes, F), np.asarray(scores, F)
    n = boxes.shape[0]
    dets = np.zeros((n * D, 8), np.int32)
    dets[:, 0] = -1
    counts = np.zeros(n, np.int32)
    with np.errstate(all="ignore"):
        for i in range(n):
            k, cls, s, box = candidates(boxes[i], scores[i], rects[i], score_thr, box_format, T)
            if not len(k):
                continue
            keep = nms(box, cls, iou_thr, class_agnostic, D)
            x, y, w, h = to_pixels(box[keep], rects[i])
            m = len(keep)
            rows = dets[i * D:i * D + m]
            rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4] = i, x, y, w, h
            rows[:, 5], rows[:, 6], rows[:, 7] = cls[keep], score_bits(s[keep]), k[keep]
            counts[i] = m
    return dets, counts


def rois_of(dets, crop):
    """(N * D, 8): x, y, w, h, px, py, pw, ph; unused rows all zero"""
    out = np.zeros_like(dets)
    used = dets[:, 0] >= 0
    out[used, :4] = dets[used, 1:5]
    out[used, 4:] = np.asarray(crop, np.int32)
    return out


def marks_of(dets, colours, thickness=2, label_rects=None, label_alpha=200, text_colour=pack_colour(0, 0, 0)):
    """(R * N * D, 8) annotator rows: outlines, then label backgrounds, then texts"""
    colours = np.asarray(colours, np.int64)
    m = len(dets)
    used = dets[:, 0] >= 0
    cls = dets[:, 5].astype(np.int64)
    col = colours[cls % len(colours)]
    out = np.zeros(((3 if label_rects is not None else 1) * m, 8), np.int32)
    box = out[:m]
    box[used, :5] = dets[used, :5]
    box[used, 5], box[used, 6], box[used, 7] = MARK_BOX, thickness, i32(col[used])
    if label_rects is not None:
        lr = np.asarray(label_rects, np.int64).reshape(-1, 4)
        lab = used & (cls < len(lr))
        r = lr[np.where(lab, cls, 0)]
        bg, tx = out[m:2 * m], out[2 * m:]
        for rows in (bg, tx):
            rows[lab, 0], rows[lab, 1] = dets[lab, 0], dets[lab, 1]
            rows[lab, 2] = i32(dets[lab, 2].astype(np.int64) - r[lab, 3])
            rows[lab, 3], rows[lab, 4] = i32(r[lab, 2]), i32(r[lab, 3])
        bg[lab, 5], bg[lab, 7] = MARK_FILL, i32((col[lab] & 0x00FFFFFF) | (label_alpha << 24))
        tx[lab, 5], tx[lab, 6], tx[lab, 7] = MARK_STAMP, i32(r[lab, 0] | (r[lab, 1] << 16)), text_colour
    return out
