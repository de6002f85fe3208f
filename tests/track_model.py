"""The definition of vali_track_update (include/vali_hip.h, "tracks") restated in numpy: every float operation is one IEEE
float32 operation, nothing is fused.  The rows are walked one by one in Python, the tracks of a stream are numpy
arrays.  tests/test_track_host.py checks it on hand-made cases with the expected rows written out and on planted objects;
the GPU tests compare the kernel with it bit for bit."""
import numpy as np

from detect_model import MARK_BOX, MARK_FILL, MARK_STAMP, i32, pack_colour

F = np.float32
SAT = 1 << 30
I32_MAX = 2**31 - 1
# a track row
ID, CLS, X, Y, W, H, VX, VY, HITS, MISSES, AGE, SCORE, K = range(13)


def _f(bits):
    """the float32 an int carries as its bits"""
    return np.asarray(bits, np.int64).astype(np.uint32).view(F) if np.ndim(bits) else np.array([bits], np.int64).astype(np.uint32).view(F)[0]


def _bits(v):
    return int(np.array([v], F).view(np.int32)[0])


def _sat_inc(v):
    return min(int(v) + 1, SAT)


def _read_tracks(rows):
    """the (T, 16) rows of one stream as they are read: free rows zero, counters clamped, values 13..15 zero"""
    t = np.asarray(rows, np.int64).copy()
    live = (t[:, ID] >= 1) & (t[:, W] >= 1) & (t[:, H] >= 1)
    t[~live] = 0
    t[:, HITS:AGE + 1] = np.clip(t[:, HITS:AGE + 1], 0, SAT)
    t[:, 13:] = 0
    return t


def _frame(t, next_id, i, rows, p):
    """one frame of one stream: t (T, 16) int64 is rewritten; returns (next_id, tracked (D, 8), assoc (D, 4))"""
    iou_thr, new_thr, mom = F(p["iou_thr"]), F(p["new_thr"]), F(p["momentum"])
    T, D = len(t), len(rows)
    tracked = np.zeros((D, 8), np.int64)
    tracked[:, 0] = -1
    assoc = np.zeros((D, 4), np.int64)
    assoc[:, 1] = -1
    # 1. prediction
    live = t[:, ID] >= 1
    g = (t[:, MISSES] + 1).astype(F)
    vx, vy = _f(t[:, VX]), _f(t[:, VY])
    fw, fh = t[:, W].astype(F), t[:, H].astype(F)
    px0, py0 = t[:, X].astype(F) + vx * g, t[:, Y].astype(F) + vy * g
    px1, py1 = px0 + fw, py0 + fh
    pa = fw * fh
    matched = np.zeros(T, bool)
    rows = np.asarray(rows, np.int64)
    # 2. valid rows
    valid = (rows[:, 0] == i) & (rows[:, 3] >= 1) & (rows[:, 4] >= 1)
    births = []
    for r in np.flatnonzero(valid):
        _, x, y, w, h, cls, sbits, k = (int(v) for v in rows[r])
        dx0, dy0, dw, dh = F(x), F(y), F(w), F(h)
        dx1, dy1, da = dx0 + dw, dy0 + dh, dw * dh
        # 3. association
        cand = live & ~matched
        if not p["class_agnostic"]:
            cand &= t[:, CLS] == cls
        iw = np.where(dx1 < px1, dx1, px1) - np.where(dx0 > px0, dx0, px0)
        ih = np.where(dy1 < py1, dy1, py1) - np.where(dy0 > py0, dy0, py0)
        cand &= (iw > 0) & (ih > 0)
        inter = iw * ih
        uni = (pa + da) - inter
        iou = inter / uni
        cand &= iou > iou_thr
        if not cand.any():
            if _f(sbits) >= new_thr:
                births.append(r)
            continue
        best = iou[cand].max()
        j = int(np.flatnonzero(cand & (iou == best))[0])
        # 4. update
        step_x = (F((2 * x + w) - (2 * int(t[j, X]) + int(t[j, W]))) * F(0.5)) / g[j]
        step_y = (F((2 * y + h) - (2 * int(t[j, Y]) + int(t[j, H]))) * F(0.5)) / g[j]
        t[j, VX], t[j, VY] = _bits(vx[j] + mom * (step_x - vx[j])), _bits(vy[j] + mom * (step_y - vy[j]))
        t[j, CLS], t[j, X], t[j, Y], t[j, W], t[j, H], t[j, SCORE], t[j, K] = cls, x, y, w, h, sbits, k
        t[j, HITS], t[j, MISSES], t[j, AGE] = _sat_inc(t[j, HITS]), 0, _sat_inc(t[j, AGE])
        matched[j] = True
        assoc[r] = t[j, ID], j, t[j, HITS], cls
        if t[j, HITS] >= p["min_hits"]:
            tracked[r] = i, x, y, w, h, t[j, ID], sbits, k
    # 5. unmatched live tracks
    for j in np.flatnonzero(live & ~matched):
        t[j, MISSES], t[j, AGE] = _sat_inc(t[j, MISSES]), _sat_inc(t[j, AGE])
        if t[j, MISSES] > p["max_age"] or t[j, HITS] < p["min_hits"]:
            t[j] = 0
    # 6. births
    for r in births:
        free = np.flatnonzero(t[:, ID] == 0)
        if not len(free):
            break
        j = int(free[0])
        _, x, y, w, h, cls, sbits, k = (int(v) for v in rows[r])
        t[j] = 0
        t[j, :13] = next_id, cls, x, y, w, h, 0, 0, 1, 0, 1, sbits, k
        assoc[r] = next_id, j, 1, cls
        if 1 >= p["min_hits"]:
            tracked[r] = i, x, y, w, h, next_id, sbits, k
        next_id = 1 if next_id == I32_MAX else next_id + 1
    return next_id, tracked, assoc


def update(dets, tracks, clock, streams, max_det, max_tracks, iou_thr=0.3, new_thr=0.5, min_hits=3, max_age=30,
           momentum=0.5, class_agnostic=False):
    """One call: returns (tracks, clock, tracked, assoc) as new int32 arrays; the arguments are left as they are."""
    S, D, T = streams, max_det, max_tracks
    dets = np.asarray(dets, np.int32).reshape(-1, 8)
    n = len(dets) // D
    assert len(dets) == n * D and n % S == 0
    Fr = n // S
    p = dict(iou_thr=iou_thr, new_thr=new_thr, min_hits=min_hits, max_age=max_age, momentum=momentum,
             class_agnostic=class_agnostic)
    tracks = np.asarray(tracks, np.int32).reshape(S * T, 16)
    clock = np.asarray(clock, np.int32).reshape(S, 4)
    out_t, out_c = np.zeros((S * T, 16), np.int64), np.zeros((S, 4), np.int64)
    tracked, assoc = np.zeros((n * D, 8), np.int64), np.zeros((n * D, 4), np.int64)
    with np.errstate(all="ignore"):
        for s in range(S):
            t = _read_tracks(tracks[s * T:(s + 1) * T])
            next_id = max(int(clock[s, 0]), 1)
            for f in range(Fr):
                i = s * Fr + f
                next_id, tracked[i * D:(i + 1) * D], assoc[i * D:(i + 1) * D] = _frame(t, next_id, i, dets[i * D:(i + 1) * D], p)
            out_t[s * T:(s + 1) * T] = t
            out_c[s] = next_id, int(clock[s, 1]) + Fr, 0, 0
    return i32(out_t), i32(out_c), i32(tracked), i32(assoc)


def marks_of(tracked, colours, thickness=2, label_rects=None, label_alpha=200, text_colour=pack_colour(0, 0, 0)):
    """(R * N * D, 8) annotator rows of the tracked rows: outlines, then label backgrounds, then texts, coloured and
    labelled by the id"""
    colours = np.asarray(colours, np.int64)
    m = len(tracked)
    used = tracked[:, 0] >= 0
    ids = tracked[:, 5].astype(np.int64)
    col = colours[ids % len(colours)]
    out = np.zeros(((3 if label_rects is not None else 1) * m, 8), np.int32)
    box = out[:m]
    box[used, :5] = tracked[used, :5]
    box[used, 5], box[used, 6], box[used, 7] = MARK_BOX, thickness, i32(col[used])
    if label_rects is not None:
        lr = np.asarray(label_rects, np.int64).reshape(-1, 4)
        r = lr[ids % len(lr)]
        bg, tx = out[m:2 * m], out[2 * m:]
        for rows in (bg, tx):
            rows[used, 0], rows[used, 1] = tracked[used, 0], tracked[used, 1]
            rows[used, 2] = i32(tracked[used, 2].astype(np.int64) - r[used, 3])
            rows[used, 3], rows[used, 4] = i32(r[used, 2]), i32(r[used, 3])
        bg[used, 5], bg[used, 7] = MARK_FILL, i32((col[used] & 0x00FFFFFF) | (label_alpha << 24))
        tx[used, 5], tx[used, 6], tx[used, 7] = MARK_STAMP, i32(r[used, 0] | (r[used, 1] << 16)), text_colour
    return out


def det_rows(n, D, boxes):
    """(n * D, 8) int32 rows as PyDetectionSelector writes them from {frame: [(x, y, w, h, class, score), ...]}, each
    frame's rows by score descending; k is the position in the list"""
    out = np.zeros((n * D, 8), np.int32)
    out[:, 0] = -1
    for i, items in boxes.items():
        order = sorted(range(len(items)), key=lambda q: -items[q][5])
        assert len(order) <= D
        for r, q in enumerate(order):
            x, y, w, h, cls, score = items[q]
            out[i * D + r] = i, x, y, w, h, cls, _bits(F(score)), q
    return out
