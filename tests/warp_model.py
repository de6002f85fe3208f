"""Model of vali_warp_tensor / vali_warp_fit / PySurfaceWarper (include/vali_hip.h, "aligned crops"): numpy float32 with
one rounding per operation, written from the definition.

A frame is its flat, tightly packed host image (annotate_model.channels gives the views); `rows` are the (M, 8) int32
matrices rows (frame, a, b, c, d, e, f, status) with the six middle values as float32 bits; `kpts`, `dets`, `rects` as in
tests/pose_model.py, whose mapping and visibility rule the fit shares.  The YUV444 -> RGB arithmetic of an NV12 pixel is the
oracle's (oracle.convert).
"""
import numpy as np

import annotate_model as am
import mask_cases as mc
import mask_model as mm
import pose_model as po

F32 = np.float32
HALF = F32(0.5)

# the published ArcFace points (pixel centres are integers there) in this project's convention
ARCFACE_112 = tuple((u + 0.5, v + 0.5) for u, v in ((38.2946, 51.6963), (73.5318, 51.5014), (56.0252, 71.7366),
                                                    (41.5493, 92.3655), (70.7299, 92.2041)))


def pack_rows(frames, coeffs, status=0):
    """(M, 8) int32 rows from M frame indices and an (M, 6) array of coefficients (rounded to float32 here)"""
    coeffs = np.asarray(coeffs, F32).reshape(-1, 6)
    rows = np.zeros((len(coeffs), 8), np.int32)
    rows[:, 0] = np.asarray(frames, np.int64).astype(np.int32)
    rows[:, 1:7] = coeffs.view(np.int32)
    rows[:, 7] = status
    return rows


def coeffs_of(rows):
    return np.ascontiguousarray(np.asarray(rows, np.int32)[:, 1:7]).view(F32)


def positions(co, w, h):
    """step 2: (sx, sy), float32 (h, w), from each pixel's own (x, y)"""
    a, b, c, d, e, f = (F32(v) for v in co)
    u = (np.arange(w).astype(F32) + HALF)[None, :]
    v = (np.arange(h).astype(F32) + HALF)[:, None]
    with np.errstate(all="ignore"):
        sx = ((a * u).astype(F32) + (b * v).astype(F32)).astype(F32) + c
        sy = ((d * u).astype(F32) + (e * v).astype(F32)).astype(F32) + f
    return sx.astype(F32), sy.astype(F32)


def inside_of(sx, sy, W, H):
    with np.errstate(all="ignore"):
        return (sx >= 0) & (sx < F32(W)) & (sy >= 0) & (sy < F32(H))


def taps(s, n):
    """step 3 along one axis for positions inside [0, n): (i0, i1, t)"""
    g = (s - HALF).astype(F32)
    x0 = np.floor(g)
    t = (g - x0).astype(F32)
    i = x0.astype(np.int64)
    return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), t


def bilinear(plane, sx, sy):
    """step 3 for one 8-bit channel: q, uint8; sx, sy hold positions inside the plane"""
    H, W = plane.shape
    x0, x1, tx = taps(sx, W)
    y0, y1, ty = taps(sy, H)
    p = plane.astype(F32)
    p00, p01, p10, p11 = p[y0, x0], p[y0, x1], p[y1, x0], p[y1, x1]
    top = (p00 + (tx * (p01 - p00).astype(F32)).astype(F32)).astype(F32)
    bot = (p10 + (tx * (p11 - p10).astype(F32)).astype(F32)).astype(F32)
    val = (top + (ty * (bot - top).astype(F32)).astype(F32)).astype(F32)
    return np.clip(np.rint(val), 0, 255).astype(np.uint8)


def sample_q(frame, fmt, W, H, co, w, h, csc=None):
    """steps 2 to 4 for one slot: (q (3, h, w) uint8 named R, G, B, inside (h, w) bool); q is 0 where not inside.
    `csc`: the (y0, cy, crv, cgu, cgv, cbu) of an NV12 frame's matrix."""
    sx, sy = positions(co, w, h)
    inside = inside_of(sx, sy, W, H)
    px = np.where(inside, sx, HALF).astype(F32)
    py = np.where(inside, sy, HALF).astype(F32)
    ch = am.channels(fmt, frame, W, H)
    q = np.zeros((3, h, w), np.uint8)
    if fmt == "NV12":
        yuv = np.zeros((3, h, w), np.uint8)
        yuv[0] = bilinear(ch[0][0], px, py)
        cx, cy = (px * HALF).astype(F32), (py * HALF).astype(F32)
        yuv[1], yuv[2] = bilinear(ch[1][0], cx, cy), bilinear(ch[2][0], cx, cy)
        from oracle import oracle as o

        rgb = o.convert(yuv.reshape(-1), "YUV444", "RGB", w, h, o.cvt_params(csc_tuple=csc))
        q[:] = np.asarray(rgb, np.uint8).reshape(h, w, 3).transpose(2, 0, 1)
    else:
        for view, _, colour in ch:
            q[colour] = bilinear(view, px, py)
    q[:, ~inside] = 0
    return q, inside


def step5(q, c, norm):
    """((q / 255) / div - mean[c]) / std[c] in float32"""
    div, mean, std = norm
    v = (np.asarray(q).astype(F32) / F32(255.0)).astype(F32)
    v = (v / F32(div)).astype(F32)
    return ((v - F32(mean[c])).astype(F32) / F32(std[c])).astype(F32)


IDENTITY = (1.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def warp(frames, fmt, sizes, rows, canvas, norm=IDENTITY, pad=(0, 0, 0), csc=None, dtype="float32", init=None):
    """vali_warp_tensor: the (M, 3, h, w) tensor as float32 values exact in `dtype`; `init` holds what the tensor held
    before (pad = None leaves it where nothing is sampled).  Returns (out, inside (M, h, w))."""
    w, h = canvas
    rows = np.asarray(rows, np.int32)
    M = len(rows)
    out = np.zeros((M, 3, h, w), F32) if init is None else np.array(init, F32)
    ins = np.zeros((M, h, w), bool)
    co = coeffs_of(rows)
    for m in range(M):
        f = int(rows[m, 0])
        if pad is not None:
            for c in range(3):
                out[m, c] = mc.quantise(step5(pad[c], c, norm), dtype)
        if not 0 <= f < len(frames):
            continue
        q, inside = sample_q(frames[f], fmt, sizes[f][0], sizes[f][1], co[m], w, h, csc)
        for c in range(3):
            out[m, c][inside] = mc.quantise(step5(q[c], c, norm), dtype)[inside]
        ins[m] = inside
    return out, ins


SKIP_ROW = (-1, 0, 0, 0, 0, 0, 0, 0)


def used_points(kp, rect, template, thr):
    """steps 2 of the fit for the (P, 3) or (P, 2) keypoints of one row: (used (P,) bool, fx, fy float32)"""
    kp = np.asarray(kp, F32)
    sx, sy, sw, sh, dx, dy, dw, dh = (int(v) for v in rect)
    kx, ky = kp[:, 0], kp[:, 1]
    conf = kp[:, 2] if kp.shape[1] == 3 else np.ones(len(kp), F32)
    fx, fy = po.map_axis(kx, dx, sw, dw, sx), po.map_axis(ky, dy, sh, dh, sy)
    t = np.asarray(template, F32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        vis = ((conf > F32(thr)) & np.isfinite(kx) & np.isfinite(ky) & (fx >= po.LO) & (fx < po.HI) & (fy >= po.LO) &
               (fy < po.HI))
    return vis & ~np.isnan(t[:, 0]) & ~np.isnan(t[:, 1]), fx, fy


def fit_row(i, kp, rect, template, thr, min_points):
    """steps 2 to 4 of the fit for one row that is not skipped by step 1: 8 integers"""
    used, fx, fy = used_points(kp, rect, template, thr)
    t = np.asarray(template, F32).reshape(-1, 2)
    idx = np.flatnonzero(used)
    n = len(idx)
    if n < min_points:
        return SKIP_ROW
    su = sv = sx = sy = F32(0)
    for j in idx:
        su, sv, sx, sy = F32(su + t[j, 0]), F32(sv + t[j, 1]), F32(sx + fx[j]), F32(sy + fy[j])
    fn = F32(n)
    mu, mv, mx, my = F32(su / fn), F32(sv / fn), F32(sx / fn), F32(sy / fn)
    A = B = Dn = F32(0)
    for j in idx:
        du, dv, dx, dy = F32(t[j, 0] - mu), F32(t[j, 1] - mv), F32(fx[j] - mx), F32(fy[j] - my)
        A = F32(A + F32(F32(du * dx) + F32(dv * dy)))
        B = F32(B + F32(F32(du * dy) - F32(dv * dx)))
        Dn = F32(Dn + F32(F32(du * du) + F32(dv * dv)))
    if Dn == 0:
        return SKIP_ROW
    with np.errstate(all="ignore"):
        al, be = F32(A / Dn), F32(B / Dn)
    if not (np.isfinite(al) and np.isfinite(be)):
        return SKIP_ROW
    c = F32(mx - F32(F32(al * mu) - F32(be * mv)))
    f = F32(my - F32(F32(be * mu) + F32(al * mv)))
    co = np.array([al, -be, c, be, al, f], F32).view(np.int32)
    return (i, *(int(v) for v in co), n)


def fit(sizes, dets, D, kpts, rects, template, thr=0.5, min_points=2):
    """vali_warp_fit: the (N * D, 8) int32 rows"""
    n, K = kpts.shape[0], kpts.shape[1]
    out = np.zeros((n * D, 8), np.int32)
    with np.errstate(all="ignore"):
        for i in range(n):
            for r in range(D):
                row = dets[i * D + r]
                if mm.resolve(row, i, sizes[i], K, rects[i]) is None:
                    out[i * D + r] = SKIP_ROW
                else:
                    out[i * D + r] = fit_row(i, kpts[i, int(row[7])], rects[i], template, thr, min_points)
    return out
