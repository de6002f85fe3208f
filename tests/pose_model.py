"""Model of vali_pose_paint / PyPoseDrawer (include/vali_hip.h, "pose skeletons"): numpy float32 with one rounding per
operation for the mapping, numpy int64 and Python integers for the coverage, written from the definition.

`kpts` (N, K, P, 3 or 2) is a float32 array (holding exactly the values of a float16 / bfloat16 tensor where the GPU gets
one), `dets` rows of 8 integers, `rects` rows of 8 integers (src_x, src_y, src_w, src_h, dst_x, dst_y, dst_w, dst_h),
`limbs` pairs of keypoint indices.  A frame is its flat, tightly packed host image (annotate_model.channels gives the
views).  Step 1 (which rows are drawn) and the blend of a coverage are the masks': mask_model.resolve, mask_model.blend.
"""
import numpy as np

import mask_model as mm

F32 = np.float32
LO, HI = F32(-65536.0), F32(131072.0)

COCO_SKELETON = ((15, 13), (13, 11), (16, 14), (14, 12), (11, 12), (5, 11), (6, 12), (5, 6), (5, 7), (6, 8), (7, 9),
                 (8, 10), (1, 2), (0, 1), (0, 2), (1, 3), (2, 4), (3, 5), (4, 6))


def map_axis(v, dst, src_n, dst_n, src):
    """step 2 along one axis: (v - dst) * (src_n / dst_n) + src, every operation rounded to float32"""
    scale = F32(F32(src_n) / F32(dst_n))
    with np.errstate(all="ignore"):
        return (((np.asarray(v, F32) - F32(dst)).astype(F32) * scale).astype(F32) + F32(src)).astype(F32)


def row_points(kp, rect, size, thr):
    """steps 2 and 3 for the (P, 3) or (P, 2) keypoints of one drawn row: (P, 4) int64 rows X, Y, conf bits, flag"""
    kp = np.asarray(kp, F32)
    sx, sy, sw, sh, dx, dy, dw, dh = (int(v) for v in rect)
    kx, ky = kp[:, 0], kp[:, 1]
    conf = kp[:, 2].copy() if kp.shape[1] == 3 else np.ones(len(kp), F32)
    fx, fy = map_axis(kx, dx, sw, dw, sx), map_axis(ky, dy, sh, dh, sy)
    with np.errstate(all="ignore"):
        vis = (conf > F32(thr)) & np.isfinite(kx) & np.isfinite(ky) & (fx >= LO) & (fx < HI) & (fy >= LO) & (fy < HI)
        X = np.where(vis, np.floor(np.where(vis, fx, 0)), 0).astype(np.int64)
        Y = np.where(vis, np.floor(np.where(vis, fy, 0)), 0).astype(np.int64)
    inside = vis & (X >= 0) & (X < size[0]) & (Y >= 0) & (Y < size[1])
    flag = np.where(inside, 3, np.where(vis, 1, 0))
    return np.stack([X, Y, conf.view(np.int32).astype(np.int64), flag], 1)


def limb_cover(A, B, t, xs, ys):
    """step 4 for the pixels xs x ys (int arrays): a bool array (len(ys), len(xs)).  int64 throughout: coordinates are
    below 2^18 in magnitude, so every product fits but c * c; 4 c^2 >= 2^62 > t^2 L2 where |c| >= 2^30
    (tests/test_pose_host.py checks all of it against Python integers)."""
    px, py = np.meshgrid(np.asarray(xs, np.int64), np.asarray(ys, np.int64))
    ax, ay, bx, by, t = int(A[0]), int(A[1]), int(B[0]), int(B[1]), int(t)
    ex, ey = bx - ax, by - ay
    qx, qy = px - ax, py - ay
    cap_a = 4 * (qx * qx + qy * qy) <= t * t
    L2 = ex * ex + ey * ey
    if L2 == 0:
        return cap_a
    cap_b = 4 * ((px - bx) ** 2 + (py - by) ** 2) <= t * t
    s = qx * ex + qy * ey
    c = qx * ey - qy * ex
    far = np.abs(c) >= 1 << 30
    c = np.where(far, 0, c)
    mid = ~far & (4 * c * c <= t * t * L2)
    return np.where(s <= 0, cap_a, np.where(s >= L2, cap_b, mid))


def joint_cover(C, d, xs, ys):
    """a disc of diameter d at C: 4 |P - C|^2 <= d^2"""
    return limb_cover(C, C, d, xs, ys)


def covers_exact(A, B, t, P):
    """step 4 for one pixel in Python integers, as the definition states it"""
    ex, ey = int(B[0]) - int(A[0]), int(B[1]) - int(A[1])
    qx, qy = int(P[0]) - int(A[0]), int(P[1]) - int(A[1])
    L2, s = ex * ex + ey * ey, qx * ex + qy * ey
    if L2 == 0 or s <= 0:
        return 4 * (qx * qx + qy * qy) <= t * t
    if s >= L2:
        return 4 * ((int(P[0]) - int(B[0])) ** 2 + (int(P[1]) - int(B[1])) ** 2) <= t * t
    c = qx * ey - qy * ex
    return 4 * c * c <= t * t * L2


def points_of(sizes, dets, D, kpts, rects, thr):
    """(N * D, P, 4) int32: every row of every call; skipped rows are zero"""
    n, K, P = kpts.shape[0], kpts.shape[1], kpts.shape[2]
    out = np.zeros((n * D, P, 4), np.int32)
    for i in range(n):
        for r in range(D):
            row = dets[i * D + r]
            if mm.resolve(row, i, sizes[i], K, rects[i]) is None:
                continue
            out[i * D + r] = row_points(kpts[i, int(row[7])], rects[i], sizes[i], thr).astype(np.int32)
    return out


def shapes_of(points_row, limbs, thickness, diameter):
    """step 5 for one drawn row: [(shape index, A, B, width)] -- the limbs whose two keypoints are visible in table order,
    then the visible joints; shape index l for limb l, len(limbs) + p for joint p"""
    out = []
    for l, (a, b) in enumerate(limbs):
        if points_row[a][3] and points_row[b][3]:
            out.append((l, points_row[a][:2], points_row[b][:2], thickness))
    for p, pt in enumerate(points_row):
        if pt[3]:
            out.append((len(limbs) + p, pt[:2], pt[:2], diameter))
    return out


def apply(frames, fmt, sizes, dets, D, kpts, rects, limbs, limb_colours, joint_colours, thr=0.5, thickness=3, diameter=7,
          alpha=None, rows=None):
    """the skeletons of `dets` ((N * D) rows) onto `frames`, rows ascending, limbs then joints; returns (points, drawn):
    drawn = [(row index, shape index, frame, cover (H, W) bool, colour)] of every shape of every drawn row"""
    points = points_of(sizes, dets, D, kpts, rects, thr)
    K, L = kpts.shape[1], len(limbs)
    drawn = []
    for i in range(len(frames)):
        w, h = sizes[i]
        for r in range(D):
            idx = i * D + r
            if mm.resolve(dets[idx], i, sizes[i], K, rects[i]) is None:
                continue
            for j, A, B, width in shapes_of(points[idx].astype(np.int64), limbs, thickness, diameter):
                cover = limb_cover(A, B, width, np.arange(w), np.arange(h))
                colour = mm.colour_of(j, limb_colours, alpha) if j < L else mm.colour_of(j - L, joint_colours, alpha)
                mm.blend(frames[i], fmt, w, h, (0, 0, w, h), cover, colour, rows)
                drawn.append((idx, j, i, cover, colour))
    return points, drawn


def stamp_atlas(drawn):
    """the shapes of apply() as a coverage atlas (255 / 0, one under the other) and the STAMP rows that paint them:
    vali_annotate_batch_atlas with these gives the same frames (step 6).  A shape that covers no pixel of its frame has no
    row."""
    boxes = []
    for _, _, _, cover, _ in drawn:
        ys, xs = np.flatnonzero(cover.any(1)), np.flatnonzero(cover.any(0))
        boxes.append(None if not len(xs) else (int(xs[0]), int(ys[0]), int(xs[-1]) + 1, int(ys[-1]) + 1))
    width = max([b[2] - b[0] for b in boxes if b] + [1])
    height = sum(b[3] - b[1] for b in boxes if b)
    assert height <= 65535
    atlas = np.zeros((max(height, 1), width), np.uint8)
    marks, v = [], 0
    for (_, _, frame, cover, colour), b in zip(drawn, boxes):
        if b is None:
            continue
        x0, y0, x1, y1 = b
        atlas[v:v + y1 - y0, :x1 - x0] = cover[y0:y1, x0:x1].astype(np.uint8) * 255
        arg = v << 16
        marks.append((frame, x0, y0, x1 - x0, y1 - y0, 4, arg - (1 << 32) if arg >= 1 << 31 else arg, colour))
        v += y1 - y0
    return atlas, marks
