"""Model of vali_kpt_decode / PyKeypointDecoder (include/vali_hip.h, "keypoint decode"): numpy float32 with one rounding
per operation, written from the definition.

`heat` (M, P, Hh, Wh) -- or `simcc_x` (M, P, Wx) and `simcc_y` (M, P, Wy) -- is a float32 array (holding exactly the
values of a float16 / bfloat16 tensor where the GPU gets one), `rows` (M, 8) int32: matrices (frame, a, b, c, d, e, f,
status; the six middle values float32 bit patterns) with D = 0, or roi records (src_x, src_y, src_w, src_h, dst_x, dst_y,
dst_w, dst_h) with D = max_det.  `sizes` are the frames' (W, H).  Which NaN a step yields is not defined: compare kpts
with same_floats().  sanitise() is the rule vali_pose_paint_points reads caller-made points by.
"""
import numpy as np

from pose_model import HI, LO, map_axis

F32 = np.float32
NAN_BITS = 0x7fc00000


def peak(v):
    """step 2 for one map in row-major order: (index, value) or None.  Written as the definition says it, not as the
    kernel finds it: the greatest non-NaN element, then the lowest index that compares equal to it."""
    v = np.asarray(v, F32).ravel()
    ok = ~np.isnan(v)
    if not ok.any():
        return None
    top = v[ok].max()
    i = int(np.flatnonzero(ok & (v == top))[0])
    return i, v[i]


def quarter(h, xp, yp):
    """step 3: (ox, oy)"""
    def off(hi, lo):
        with np.errstate(all="ignore"):
            d = F32(hi) - F32(lo)
        return F32(0.25) if d > 0 else F32(-0.25) if d < 0 else F32(0.0)
    hh, wh = h.shape
    ox = off(h[yp, xp + 1], h[yp, xp - 1]) if 0 < xp < wh - 1 else F32(0.0)
    oy = off(h[yp + 1, xp], h[yp - 1, xp]) if 0 < yp < hh - 1 else F32(0.0)
    return ox, oy


def canvas_pos(p, o, size, cells, align):
    """step 4 along one axis"""
    s = F32(F32(size) / F32(cells))
    if align == "centre":
        return F32(F32(F32(F32(p) + F32(0.5)) + o) * s)
    assert align == "index"
    return F32(F32(F32(F32(p) + o) * s) + F32(0.5))


def slot_frame(row, m, n, D):
    """step 1: the frame of slot m, or None for a skipped slot"""
    row = [int(v) for v in row]
    if D == 0:
        return row[0] if 0 <= row[0] < n else None
    return m // D if min(row[2], row[3], row[6], row[7]) >= 1 else None


def to_frame(row, D, cu, cv):
    """step 5"""
    with np.errstate(all="ignore"):
        if D == 0:
            a, b, c, d, e, f = np.asarray(row[1:7], np.int32).view(F32)
            fx = F32(F32(F32(a * cu) + F32(b * cv)) + c)
            fy = F32(F32(F32(d * cu) + F32(e * cv)) + f)
            return fx, fy
        sx, sy, sw, sh, dx, dy, dw, dh = (int(v) for v in row)
        return F32(map_axis(cu, dx, sw, dw, sx)), F32(map_axis(cv, dy, sh, dh, sy))


def _row(conf, thr, cu, cv, fx, fy, size):
    """step 6: the points row and the kpts row"""
    with np.errstate(all="ignore"):
        vis = bool(conf > F32(thr)) and bool(fx >= LO) and bool(fx < HI) and bool(fy >= LO) and bool(fy < HI)
    X = Y = flag = 0
    if vis:
        X, Y = int(np.floor(fx)), int(np.floor(fy))
        flag = 3 if 0 <= X < size[0] and 0 <= Y < size[1] else 1
    bits = int(np.asarray(conf, F32).view(np.int32))
    return (X, Y, bits, flag), (fx, fy, conf)


def decode(sizes, rows, D, canvas, heat=None, simcc=None, thr=0.3, refine="quarter", align="centre"):
    """(points (M, P, 4) int32, kpts (M, P, 3) float32) of one call"""
    if heat is not None:
        heat = np.asarray(heat, F32)
        M, P, hh, wh = heat.shape
    else:
        vx, vy = (np.asarray(v, F32) for v in simcc)
        assert refine == "none"
        (M, P, wh), hh = vx.shape, vy.shape[2]
    points, kpts = np.zeros((M, P, 4), np.int32), np.zeros((M, P, 3), F32)
    for m in range(M):
        frame = slot_frame(rows[m], m, len(sizes), D)
        if frame is None:
            continue
        for j in range(P):
            ox = oy = F32(0.0)
            if heat is not None:
                pk = peak(heat[m, j])
                if pk is not None:
                    yp, xp = divmod(pk[0], wh)
                    conf = pk[1]
                    if refine == "quarter":
                        ox, oy = quarter(heat[m, j], xp, yp)
            else:
                px, py = peak(vx[m, j]), peak(vy[m, j])
                pk = None if px is None or py is None else (px, py)
                if pk is not None:
                    xp, yp = px[0], py[0]
                    conf = py[1] if py[1] < px[1] else px[1]
            if pk is None:
                points[m, j] = (0, 0, NAN_BITS, 0)
                kpts[m, j] = (0, 0, np.nan)
                continue
            cu, cv = canvas_pos(xp, ox, canvas[0], wh, align), canvas_pos(yp, oy, canvas[1], hh, align)
            fx, fy = to_frame(rows[m], D, cu, cv)
            pt, kp = _row(conf, thr, cu, cv, fx, fy, sizes[frame])
            points[m, j] = np.asarray(pt, np.int64).astype(np.int32)
            kpts[m, j] = kp
    return points, kpts


def same_floats(got, want):
    """bit for bit, except that any NaN equals any NaN"""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan]))


def sanitise(points, sizes, D):
    """caller-made points (N * D, P, 4) as vali_pose_paint_points reads them: visible when flag & 1 and -65536 <= X, Y <
    131072, flag 3 inside the row's frame; every other row all zero"""
    points = np.asarray(points, np.int64)
    out = np.zeros(points.shape, np.int32)
    for r in range(points.shape[0]):
        w, h = sizes[r // D]
        for j, (x, y, z, flag) in enumerate(points[r]):
            if flag & 1 and -65536 <= x < 131072 and -65536 <= y < 131072:
                out[r, j] = (x, y, z, 3 if 0 <= x < w and 0 <= y < h else 1)
    return out


def paint_points(frames, fmt, sizes, points, D, limbs, limb_colours, joint_colours, thickness=3, diameter=7, alpha=None,
                 rows=None):
    """vali_pose_paint_points: the skeletons of caller-made `points` onto `frames` (flat host images), rows ascending,
    limbs then joints -- pose_model's shapes, coverage and blend on the sanitised points.  Returns how many shapes it
    drew."""
    import mask_model as mm
    import pose_model as po

    pts = sanitise(points, sizes, D).astype(np.int64)
    L, drawn = len(limbs), 0
    for r in range(pts.shape[0]):
        i = r // D
        w, h = sizes[i]
        for j, A, B, width in po.shapes_of(pts[r], limbs, thickness, diameter):
            cover = po.limb_cover(A, B, width, np.arange(w), np.arange(h))
            colour = mm.colour_of(j, limb_colours, alpha) if j < L else mm.colour_of(j - L, joint_colours, alpha)
            mm.blend(frames[i], fmt, w, h, (0, 0, w, h), cover, colour, rows)
            drawn += 1
    return drawn


def matrix_rows(frames, mats):
    """(M, 8) int32 rows from frame indices and (M, 6) float32 coefficients"""
    mats = np.ascontiguousarray(mats, F32)
    rows = np.zeros((len(frames), 8), np.int32)
    rows[:, 0] = frames
    rows[:, 1:7] = mats.view(np.int32)
    return rows
