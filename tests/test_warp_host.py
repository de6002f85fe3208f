"""Aligned crops without a GPU: the numpy model (tests/warp_model.py) pinned to independent implementations -- its sampler
to torch's grid_sample and to exact texel properties, its fit to the float64 closed form and to numpy's least squares --
the Python checks, and what the C entry points refuse before any device is touched."""
import ctypes
import math
import types
from pathlib import Path

import numpy as np
import pytest

import warp_model as wm

ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32


def similarity(rng, W, H, w, h):
    """a random similarity (scale 0.2..3, any angle) that takes the canvas centre to a point of the frame"""
    s, th = rng.uniform(0.2, 3.0), rng.uniform(0, 2 * np.pi)
    a, d = s * np.cos(th), s * np.sin(th)
    cx, cy = rng.uniform(0.1 * W, 0.9 * W), rng.uniform(0.1 * H, 0.9 * H)
    return np.array([a, -d, cx - (a * w / 2 - d * h / 2), d, a, cy - (d * w / 2 + a * h / 2)], F32)


# ---- the sampler against grid_sample ---------------------------------------------------------------------------------------
def test_the_sampler_is_grid_sample_with_border_padding():
    """|q - g| <= 0.55 at every compared pixel: 0.5 is the rounding to 8 bits, the rest covers the float32 position error,
    at most about 256 * 2^-22 pixels x 255 levels = 0.02.  Pixels whose float64 position lies within 2^-10 of a frame edge may
    differ in `inside` and are left out, at most 1 % of any case."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(11)
    worst, compared = 0.0, 0
    for case in range(40):
        W, H = int(rng.integers(9, 257)), int(rng.integers(9, 257))
        w, h = int(rng.integers(8, 49)), int(rng.integers(8, 41))
        frame = rng.integers(0, 256, W * H * 3, dtype=np.uint8)
        co = similarity(rng, W, H, w, h)
        q, inside = wm.sample_q(frame, "RGB", W, H, co, w, h)
        a, b, c, d, e, f = (float(v) for v in co)
        u, v = np.arange(w) + 0.5, (np.arange(h) + 0.5)[:, None]
        sx, sy = a * u + b * v + c, d * u + e * v + f
        near = ((np.abs(sx) < 2.0 ** -10) | (np.abs(sx - W) < 2.0 ** -10) | (np.abs(sy) < 2.0 ** -10) |
                (np.abs(sy - H) < 2.0 ** -10))
        assert near.mean() <= 0.01, case
        inside64 = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
        assert np.array_equal(inside[~near], inside64[~near]), case
        grid = torch.from_numpy(np.stack([sx * 2 / W - 1, sy * 2 / H - 1], -1)[None])
        img = torch.from_numpy(frame.reshape(H, W, 3).transpose(2, 0, 1).astype(np.float64)[None])
        g = torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=False)[0].numpy()
        use = inside & ~near
        err = np.abs(q.astype(np.float64) - g)[:, use]
        if err.size:
            worst = max(worst, float(err.max()))
            compared += err.size
    print(f"sampler against grid_sample: worst |q - g| = {worst:.4f} over {compared} values")
    assert compared > 40 * 3 * 100
    assert worst <= 0.55


# ---- exact properties ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["RGB", "BGR", "RGB_PLANAR"])
def test_integer_shifts_return_the_texels(fmt):
    import annotate_model as am

    W, H, w, h = 50, 38, 16, 16
    frame = am.noise_frame(fmt, W, H, 5)
    planes = {colour: view for view, _, colour in am.channels(fmt, frame, W, H)}
    for cx, cy in ((0, 0), (7, 11), (34, 22), (-5, -3), (40, 30)):
        q, inside = wm.sample_q(frame, fmt, W, H, (1, 0, cx, 0, 1, cy), w, h)
        y, x = np.mgrid[0:h, 0:w]
        want_in = (x + cx >= 0) & (x + cx < W) & (y + cy >= 0) & (y + cy < H)
        assert np.array_equal(inside, want_in)
        for c in range(3):
            assert np.array_equal(q[c][inside], planes[c][(y + cy)[inside], (x + cx)[inside]])


def test_the_quarter_turn_is_rot90_of_the_crop():
    import annotate_model as am

    W, H, w, h = 64, 48, 16, 12
    frame = am.noise_frame("RGB_PLANAR", W, H, 6)
    c, f = 40, 9                               # sx = c - v, sy = u + f
    q, inside = wm.sample_q(frame, "RGB_PLANAR", W, H, (0, -1, c, 1, 0, f), w, h)
    assert inside.all()
    for k, (view, _, colour) in enumerate(am.channels("RGB_PLANAR", frame, W, H)):
        crop = view[f:f + w, c - h:c]
        assert np.array_equal(q[colour], np.rot90(crop))


def test_nv12_with_flat_chroma_is_the_luma_through_the_matrix(oracle):
    """an identity view of an NV12 frame whose chroma is flat equals the oracle's NV12 -> RGB"""
    from vali_amd import tasks

    W, H = 34, 26
    rng = np.random.default_rng(8)
    frame = np.concatenate([rng.integers(0, 256, W * H, dtype=np.uint8), np.tile(np.array([90, 170], np.uint8), W * H // 4)])
    q, inside = wm.sample_q(frame, "NV12", W, H, (1, 0, 0, 0, 1, 0), W, H, tasks.CSC_NPP_709CSC)
    want = oracle.nv12_to_rgb(frame.reshape(H * 3 // 2, W), W, H, oracle.csc_from_tuple(tasks.CSC_NPP_709CSC), "RGB")
    assert inside.all() and np.array_equal(q.transpose(1, 2, 0), np.asarray(want).reshape(H, W, 3))


def test_pad_skipped_slots_and_the_element_types():
    import annotate_model as am
    import mask_cases as mc

    W, H = 50, 38
    frame = am.noise_frame("RGB", W, H, 9)
    rows = wm.pack_rows([0, -1, 1, 0], [(1, 0, 45, 0, 1, 30)] * 3 + [(np.nan, 0, 0, 0, 1, 0)])
    norm = (2.0, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    canary = np.full((4, 3, 5, 7), -7.0, F32)
    out, ins = wm.warp([frame], "RGB", [(W, H)], rows, (7, 5), norm, None, dtype="float16", init=canary)
    assert ins[0].sum() == 5 * 5 and not ins[1:].any()                       # 5 columns of slot 0 are inside
    assert (out[1:] == -7).all() and (out[0][:, ~ins[0]] == -7).all() and (out[0][:, ins[0]] != -7).all()
    assert np.array_equal(out, mc.quantise(out, "float16"))
    out, _ = wm.warp([frame], "RGB", [(W, H)], rows, (7, 5), norm, (255, 0, 128), dtype="bfloat16", init=canary)
    pad = [mc.quantise(wm.step5(v, c, norm), "bfloat16") for c, v in enumerate((255, 0, 128))]
    for c in range(3):
        assert (out[1:, c] == pad[c]).all() and (out[0, c][~ins[0]] == pad[c]).all()
    assert np.array_equal(out, mc.quantise(out, "bfloat16"))


# ---- the fit against float64 ---------------------------------------------------------------------------------------------------
IDENTITY_RECT = (0, 0, 4096, 4096, 0, 0, 4096, 4096)        # the mapping of a keypoint is exact: fx = kx


def closed_form64(t, p):
    """the least-squares similarity template -> points in float64: (a, b, c, d, e, f)"""
    t, p = np.asarray(t, np.float64), np.asarray(p, np.float64)
    mt, mp = t.mean(0), p.mean(0)
    dt, dp = t - mt, p - mp
    den = (dt ** 2).sum()
    al = (dt[:, 0] * dp[:, 0] + dt[:, 1] * dp[:, 1]).sum() / den
    be = (dt[:, 0] * dp[:, 1] - dt[:, 1] * dp[:, 0]).sum() / den
    return np.array([al, -be, mp[0] - (al * mt[0] - be * mt[1]), be, al, mp[1] - (be * mt[0] + al * mt[1])])


def lstsq64(t, p):
    t, p = np.asarray(t, np.float64), np.asarray(p, np.float64)
    rows, rhs = [], []
    for (u, v), (x, y) in zip(t, p):
        rows += [[u, -v, 1, 0], [v, u, 0, 1]]
        rhs += [x, y]
    al, be, c, f = np.linalg.lstsq(np.array(rows), np.array(rhs), rcond=None)[0]
    return np.array([al, -be, c, be, al, f])


def apply64(co, pts):
    pts = np.asarray(pts, np.float64)
    return np.stack([co[0] * pts[:, 0] + co[1] * pts[:, 1] + co[2], co[3] * pts[:, 0] + co[4] * pts[:, 1] + co[5]], 1)


CORNERS = [(0, 0), (112, 0), (0, 112), (112, 112)]


def planted(rng, noise=1.5):
    """five landmarks: the ArcFace template under a random similarity (scale 0.3..8) into frame coordinates below 4096,
    with noise, as float32"""
    s, th = rng.uniform(0.3, 8.0), rng.uniform(0, 2 * np.pi)
    al, be = s * np.cos(th), s * np.sin(th)
    centre = rng.uniform(900, 3100, 2)
    t = np.asarray(wm.ARCFACE_112)
    x = al * (t[:, 0] - 56) - be * (t[:, 1] - 56) + centre[0]
    y = be * (t[:, 0] - 56) + al * (t[:, 1] - 56) + centre[1]
    pts = np.stack([x, y], 1) + rng.normal(0, noise, (5, 2)) * s / 4
    assert pts.min() > 0 and pts.max() < 4096
    return pts.astype(F32)


def test_the_fit_is_the_float64_least_squares_similarity():
    """the four corners of the 112 x 112 canvas map within 2^-8 pixels of where the float64 closed form puts them"""
    rng = np.random.default_rng(21)
    tmpl32 = np.asarray(wm.ARCFACE_112, F32)
    worst, worst_ls = 0.0, 0.0
    for case in range(3000):
        pts = planted(rng)
        kp = np.concatenate([pts, np.ones((5, 1), F32)], 1)
        row = wm.fit_row(0, kp, IDENTITY_RECT, wm.ARCFACE_112, 0.5, 2)
        assert row[0] == 0 and row[7] == 5
        co = np.array(row[1:7], np.int32).view(F32).astype(np.float64)
        ref = closed_form64(tmpl32, pts)
        worst = max(worst, float(np.abs(apply64(co, CORNERS) - apply64(ref, CORNERS)).max()))
        if case % 10 == 0:
            worst_ls = max(worst_ls, float(np.abs(apply64(lstsq64(tmpl32, pts), CORNERS) - apply64(ref, CORNERS)).max()))
    print(f"fit against float64: worst corner error {worst:.3e} pixels; closed form against lstsq {worst_ls:.3e}")
    assert worst_ls < 1e-6
    assert worst <= 2.0 ** -8


def test_two_points_are_reproduced():
    rng = np.random.default_rng(22)
    nan = float("nan")
    tmpl = [wm.ARCFACE_112[0], wm.ARCFACE_112[1], (nan, 60.0), (nan, nan), (50.0, nan)]
    t32 = np.asarray(tmpl[:2], F32).astype(np.float64)
    for _ in range(300):
        pts = planted(rng)
        kp = np.concatenate([pts, np.ones((5, 1), F32)], 1)
        row = wm.fit_row(3, kp, IDENTITY_RECT, tmpl, 0.5, 2)
        assert row[0] == 3 and row[7] == 2
        co = np.array(row[1:7], np.int32).view(F32).astype(np.float64)
        assert np.abs(apply64(co, t32) - pts[:2].astype(np.float64)).max() <= 2.0 ** -8


def test_the_rows_the_fit_skips():
    kp = np.array([[100, 100, 0.9], [140, 100, 0.9], [120, 130, 0.4], [np.nan, 5, 0.9], [130, np.inf, 0.9]], F32)
    fit = lambda kp, tmpl=wm.ARCFACE_112, thr=0.5, mp=2: wm.fit_row(0, kp, IDENTITY_RECT, tmpl, thr, mp)
    assert fit(kp)[7] == 2 and fit(kp, mp=3) == wm.SKIP_ROW
    assert fit(kp, thr=0.3)[7] == 3 and fit(kp, thr=0.95) == wm.SKIP_ROW
    same = kp.copy()
    same[1, :2] = same[0, :2]
    assert fit(same)[7] == 2 and fit(same)[1] == 0 and fit(same)[4] == 0   # coincident keypoints: al = be = 0 is a fit ...
    tsame = [wm.ARCFACE_112[0]] * 5
    assert fit(kp, tmpl=tsame) == wm.SKIP_ROW                              # ... coincident template points are none: Dn == 0
    two = fit(kp[:, :2], mp=2)                                             # kdim = 2: every confidence is 1.0
    assert two[7] == 3
    # the rows of the selector that PyPoseDrawer skips
    import mask_cases as mc
    import pose_cases as pc

    rows = wm.fit(pc.SIZES, pc.SKIPS, pc.D, pc.kpts(), pc.RECTS, wm.ARCFACE_112)
    assert {i for i in range(8) if tuple(rows[i]) != wm.SKIP_ROW} == mc.SKIPS_PAINTED


def test_coincident_keypoints_give_the_zero_matrix_and_every_pixel_samples_one_point():
    """Dn is the template's spread: with a good template and coincident keypoints the fit is al = be = 0, the all-zero
    a..e of the sampler's hostile rows"""
    kp = np.array([[100.25, 90.5, 0.9]] * 5, F32)
    row = wm.fit_row(0, kp, IDENTITY_RECT, wm.ARCFACE_112, 0.5, 2)
    co = np.array(row[1:7], np.int32).view(F32)
    assert row[7] == 5 and co[0] == 0 and co[1] == 0 and co[3] == 0 and co[4] == 0
    assert abs(co[2] - 100.25) < 1e-3 and abs(co[5] - 90.5) < 1e-3


# ---- the Python checks ---------------------------------------------------------------------------------------------------------
F32_, F16_ = (2, 32), (2, 16)


def test_the_spec_functions_say_what_is_wrong(vali):
    from vali_amd.pose import kpts_layout
    from vali_amd.warp import ARCFACE_112, fit_spec, frames_spec, keypoints_spec, matrices_spec

    assert frames_spec([(vali.NV12, 64, 48), (vali.NV12, 34, 26)]) == vali.NV12
    assert frames_spec([(vali.BGR, 50, 37)]) == vali.BGR
    for frames, text in [([], "0 surfaces"), ([(vali.RGB, 4, 4)] * 1025, "1025 surfaces"),
                         ([(vali.YUV420, 64, 48)], "supported: NV12, RGB, BGR, RGB_PLANAR"), ([(vali.Y, 64, 48)], "supported"),
                         ([(vali.NV12, 63, 48)], "even width and height"), ([(vali.NV12, 64, 47)], "even width and height"),
                         ([(vali.RGB, 64, 48), (vali.BGR, 64, 48)], "one format per batch")]:
        with pytest.raises(ValueError, match=text):
            frames_spec(frames)
    assert matrices_spec(6, (6, 8)) == 6 and matrices_spec(65535) == 65535
    for args, text in [((0,), "M = 0"), ((65536,), "M = 65536"), ((6, (5, 8)), r"shape \(6, 8\)"), ((6, (6, 6)), r"shape \(6, 8\)")]:
        with pytest.raises(ValueError, match=text):
            matrices_spec(*args)
    good = kpts_layout((2, 40, 5, 3), None, *F16_)
    n, k, p, kdim, D, flat = keypoints_spec(2, good, 6, 3, ARCFACE_112)
    assert (n, k, p, kdim, D) == (2, 40, 5, 3, 3) and len(flat) == 10 and flat[0] == 38.2946 + 0.5
    nan = float("nan")
    assert math.isnan(keypoints_spec(2, good, 6, 3, [(nan, nan)] * 3 + [(1, 2), (3, 4)])[5][0])
    for kw, text in [(dict(n_frames=3), "3 surfaces"), (dict(max_det=0), "max_det = 0"), (dict(max_det=1025), "max_det = 1025"),
                     (dict(m_out=5), r"M = 5 slots for N \* max_det = 2 \* 3 = 6"), (dict(template=ARCFACE_112[:4]), "4 pairs for keypoints of P = 5"),
                     (dict(template=[(1, 2, 3)] * 5), "pairs"), (dict(template=7), "pairs"),
                     (dict(template=[(float("inf"), 2)] * 5), "finite")]:
        a = dict(n_frames=2, m_out=6, max_det=3, template=ARCFACE_112)
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            keypoints_spec(a["n_frames"], good, a["m_out"], a["max_det"], a["template"])
    with pytest.raises(ValueError, match="exceeds 65535"):
        keypoints_spec(1024, kpts_layout((1024, 1, 5, 3), None, *F32_), 65536, 64, ARCFACE_112)
    with pytest.raises(ValueError, match="at least 2 keypoints"):
        keypoints_spec(2, kpts_layout((2, 40, 1, 3), None, *F32_), 6, 3, [(1, 2)])
    assert fit_spec(0.5, 2, 5) == (0.5, 2) and fit_spec(-np.inf, 17, 17) == (-np.inf, 17)
    for args, text in [((np.nan, 2, 5), "kpt_thr"), ((0.5, 1, 5), "min_points = 1"), ((0.5, 6, 5), "min_points = 6")]:
        with pytest.raises(ValueError, match=text):
            fit_spec(*args)


class Cai:
    """a device array seen through __cuda_array_interface__ (never dereferenced)"""

    def __init__(self, shape, typestr, ptr=4096, strides=None):
        self.shape = tuple(shape)
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 3,
                                         "strides": strides}
        self.device = types.SimpleNamespace(type="cuda", index=0)


def test_prepare_refuses_before_any_device_is_touched(vali):
    """stand-ins for the frames and tensors: every refusal comes before the first device call"""
    from vali_amd.warp import WarpBatch

    def frames(fmt=None, sizes=((64, 48), (34, 26))):
        return [types.SimpleNamespace(IsEmpty=False, Format=fmt or vali.NV12, Width=w, Height=h, DeviceId=0) for w, h in sizes]

    out = Cai((6, 3, 16, 16), "<f2")
    mats = Cai((6, 8), "<i4")
    kpts, dets = Cai((2, 40, 5, 3), "<f4"), Cai((6, 8), "<i4")
    cases = [
        (dict(matrices=None), "matrices: an int32 .6, 8. device tensor is required"),
        (dict(matrices=Cai((6, 8), "<f4")), "matrices: need an int32 tensor of shape .6x8."),
        (dict(matrices=Cai((5, 8), "<i4")), "matrices: need an int32 tensor of shape .6x8."),
        (dict(matrices=Cai((6, 8), "<i4", ptr=4104)), "matrices: the tensor must be 16-byte aligned"),
        (dict(matrices=Cai((6, 8), "<i4", strides=(64, 4))), "matrices: the tensor must be contiguous"),
        (dict(out=Cai((6, 4, 16, 16), "<f2")), "out: need 3 channels"),
        (dict(out=Cai((6, 3, 16, 16), "|u1")), "out: the dtype must be"),
        (dict(out=Cai((6, 3, 16, 16), "<f4", strides=(3072, 4, 192, 8))), "neither planar"),
        (dict(frames=frames(vali.YUV444)), "supported: NV12, RGB, BGR, RGB_PLANAR"),
        (dict(frames=frames(sizes=((64, 48), (33, 26)))), "even width and height"),
        (dict(frames=frames() + frames(vali.RGB)), "one format per batch"),
        (dict(frames=[]), "0 surfaces"),
        (dict(kpts=kpts, dets=dets, max_det=3, template=vali.ARCFACE_112, matrices=None, out=Cai((5, 3, 16, 16), "<f2")), "M = 5 slots"),
        (dict(kpts=kpts, dets=None, max_det=3, template=vali.ARCFACE_112, matrices=None), "dets: an int32 .6, 8. device tensor"),
        (dict(kpts=kpts, dets=Cai((6, 7), "<i4"), max_det=3, template=vali.ARCFACE_112, matrices=None), "dets: need an int32"),
        (dict(kpts=Cai((2, 40, 5, 4), "<f4"), dets=dets, max_det=3, template=vali.ARCFACE_112), "last dimension"),
        (dict(kpts=kpts, dets=dets, max_det=3, template=vali.ARCFACE_112[:3]), "3 pairs for keypoints of P = 5"),
        (dict(kpts=kpts, dets=dets, max_det=3, template=vali.ARCFACE_112, matrices=Cai((6, 8), "<i4", ptr=4100)), "16-byte aligned"),
    ]
    for kw, text in cases:
        a = dict(frames=frames(), out=out, matrices=mats)
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            WarpBatch(0, 0, a.pop("frames"), a.pop("out"), **a)


def test_the_names_are_exported():
    import python_vali
    import vali_amd

    for name in ("PySurfaceWarper", "WarpBatch", "ARCFACE_112"):
        assert getattr(python_vali, name) is getattr(vali_amd, name)
    assert np.allclose(np.asarray(vali_amd.ARCFACE_112), np.asarray(wm.ARCFACE_112), rtol=0, atol=0)
    assert vali_amd.ARCFACE_112[2] == (56.0252 + 0.5, 71.7366 + 0.5)


# ---- the C entry points without a device ---------------------------------------------------------------------------------------
def test_the_entry_points_refuse_null_arguments_through_ctypes():
    lib = ctypes.CDLL(str(ROOT / "vali_amd" / "libvali_hip.so"))
    lib.vali_last_error.restype = ctypes.c_char_p
    assert lib.vali_warp_fit(None, 2, None, None, None, None, None) == -1
    assert b"vali_warp_fit: null argument" in lib.vali_last_error()
    assert lib.vali_warp_tensor(None, None, 2, 3, None, None, None, 0, None, None) == -1
    assert b"vali_warp_tensor: null argument" in lib.vali_last_error()


def test_warp_fit_refuses_before_any_device_is_touched(vali):
    """the pointers below are dummies that are never read"""
    from vali_amd._native import shim

    def call(d_frames=0x1000, n=2, kpts=(0x2000, 1, 1000, 15, 3, 1), kdim=3, k=40, p=5, D=3, mp=2, tmpl=0x3000, thr=0.5,
             dets=0x4000, rects=0x5000, mats=0x6000):
        rc = shim.warp_fit(d_frames, n, kpts, kdim, k, p, D, mp, tmpl, thr, dets, rects, mats, 0)
        return rc, shim.last_error()

    cases = [
        (dict(d_frames=0), "null argument"), (dict(dets=0), "null argument"), (dict(rects=0), "null argument"),
        (dict(mats=0), "null argument"), (dict(n=0), "n outside"), (dict(n=1025), "n outside"),
        (dict(k=0), "k outside"), (dict(k=2**20 + 1), "k outside"), (dict(p=1), "p outside"), (dict(p=65), "p outside"),
        (dict(kdim=1), "kdim"), (dict(kdim=4), "kdim"), (dict(D=0), "max_det outside"), (dict(D=1025), "max_det outside"),
        (dict(n=1024, D=64), "exceeds 65535"), (dict(mp=1), "min_points outside"), (dict(mp=6), "min_points outside"),
        (dict(kpts=(0, 1, 1000, 15, 3, 1)), "kpts has a null pointer"), (dict(tmpl=0), "template has a null pointer"),
        (dict(kpts=(0x2000, 3, 1000, 15, 3, 1)), "dtype 3"), (dict(kpts=(0x2001, 1, 1000, 15, 3, 1)), "not aligned to its element"),
        (dict(kpts=(0x2002, 0, 1000, 15, 3, 1)), "not aligned to its element"), (dict(kpts=(0x2000, 1, -1, 15, 3, 1)), "strides"),
        (dict(kpts=(0x2000, 1, 1000, 15, 3, 2**41)), "strides"), (dict(thr=float("nan")), "kpt_thr"),
        (dict(dets=0x4002), "not 4-byte aligned"), (dict(rects=0x5001), "not 4-byte aligned"), (dict(tmpl=0x3002), "not 4-byte aligned"),
        (dict(mats=0x6008), "matrices is not 16-byte aligned"),
    ]
    for kw, text in cases:
        rc, err = call(**kw)
        assert rc == -1 and rc == shim.ERR_INVALID_ARG and text in err and "vali_warp_fit" in err, (kw, rc, err)


def test_warp_tensor_refuses_before_any_device_is_touched(vali):
    from vali_amd import tasks
    from vali_amd._native import shim

    prm = shim.PreprocParams(shim.Csc(*tasks.CSC_NPP_709CSC), 1.0, [0.0] * 3, [1.0] * 3)

    def call(fmt="NV12", sizes=((64, 48), (34, 26)), descs=None, d_frames=0x1000, mats=0x6000, dst=True, params=True,
             pad=True, plane=0x7000, pitch=None, data=0x8000, dtype=1, packed=0, m=6, w=16, h=16, sn=768, sc=256, sy=16):
        f = int(getattr(vali, fmt)) if isinstance(fmt, str) else fmt
        if descs is None:
            descs = [shim.SurfaceDesc([plane] * 3, [pitch or 3 * sw] * 3, sw, sh, f) for sw, sh in sizes]
        t = shim.TensorDst(data, dtype, packed, m, w, h, sn, sc, sy) if dst else None
        rc = shim.warp_tensor(descs, d_frames, f, mats, t, prm if params else None, pad, (1, 2, 3), 0)
        return rc, shim.last_error()

    cases = [
        (dict(d_frames=0), "null argument"), (dict(mats=0), "null argument"), (dict(dst=False), "null argument"),
        (dict(params=False), "null argument"), (dict(descs=[]), "null argument"),
        (dict(sizes=[(2, 2)] * 1025), "n outside"),
        (dict(sizes=((64, 48), (33, 26))), "even width and height"), (dict(sizes=((64, 48), (0, 2))), "outside 1..65535"),
        (dict(sizes=((64, 48), (65536, 2)), fmt="RGB"), "outside 1..65535"), (dict(plane=0), "plane 0 is null"),
        (dict(pitch=63), "shorter than a row"),
        (dict(data=0), "null tensor data"), (dict(dtype=3), "dtype must be"), (dict(dtype=-1), "dtype must be"),
        (dict(packed=2), "packed must be"), (dict(m=0), "batch size"), (dict(m=65536), "batch size"),
        (dict(w=0), "bad geometry"), (dict(h=0), "bad geometry"), (dict(sn=0), "strides must be positive"),
        (dict(sc=0), "strides must be positive"), (dict(sy=15), "shorter than a row"), (dict(packed=1, sy=47), "shorter than a row"),
        (dict(data=0x8001), "not aligned to its element"), (dict(dtype=0, data=0x8002), "not aligned to its element"),
        (dict(sy=2**30), "row pitch"), (dict(mats=0x6002), "not 4-byte aligned"), (dict(d_frames=0x1001), "not 4-byte aligned"),
        (dict(m=65535, w=4096, h=65536, sy=4096, sc=2**28, sn=2**30), "too large"),
    ]
    for kw, text in cases:
        rc, err = call(**kw)
        assert rc == -1 and rc == shim.ERR_INVALID_ARG and text in err and "vali_warp_tensor" in err, (kw, rc, err)
    mixed = [shim.SurfaceDesc([0x7000] * 3, [192] * 3, 64, 48, int(vali.NV12)),
             shim.SurfaceDesc([0x7000] * 3, [192] * 3, 64, 48, int(vali.RGB))]
    rc, err = call(descs=mixed)
    assert rc == shim.ERR_INVALID_ARG and "one format per batch" in err
    for fmt in ("YUV420", "YUV444", "Y"):
        rc, err = call(fmt=fmt)
        assert rc == shim.ERR_UNSUPPORTED and "NV12, RGB, BGR, RGB_PLANAR" in err
