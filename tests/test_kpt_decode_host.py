"""PyKeypointDecoder without a GPU: the numpy model (tests/kpt_decode_model.py) against torch's flattened max, against
planted Gaussians whose true centres are known, and on the edges of the definition in include/vali_hip.h; every ValueError
of Prepare / Run and every VALI_ERR_INVALID_ARG of vali_kpt_decode and vali_pose_paint_points, which are decided before
any device is touched."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

import kpt_decode_model as kd

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
IDENTITY = kd.matrix_rows([0], [[1, 0, 0, 0, 1, 0]])


def bits(v):
    return int(np.asarray(v, F).view(np.int32))


# ---- (i) the model against torch ----------------------------------------------------------------------------------------
def test_peak_equals_torchs_flattened_max_on_unique_maxima():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(0)
    for hh, wh in ((1, 1), (5, 3), (17, 13), (64, 48)):
        heat = rng.permutation(4 * 3 * hh * wh).astype(F).reshape(4, 3, hh, wh)      # every value once
        val, idx = torch.from_numpy(heat).flatten(2).max(2)
        pts, kp = kd.decode([(9999, 9999)], np.repeat(IDENTITY, 4, 0), 0, (wh, hh), heat=heat, thr=-1.0, refine="none")
        # canvas = the map and the identity: fx = xp + 0.5, fy = yp + 0.5
        assert np.array_equal(pts[..., 0], idx.numpy() % wh) and np.array_equal(pts[..., 1], idx.numpy() // wh)
        assert np.array_equal(kp[..., 2], val.numpy()) and np.array_equal(pts[..., 2], val.numpy().view(np.int32))
        assert np.array_equal(kp[..., 0], idx.numpy() % wh + F(0.5))
        assert (pts[..., 3] == 3).all()


# ---- (ii) planted Gaussians ---------------------------------------------------------------------------------------------
HH, WH, CANVAS, SIGMA = 64, 48, (192, 256), 2.0


def gaussians(rng, count, dtype):
    """(count, 1, HH, WH) maps, each a Gaussian of sigma 2 cells whose peak cell is at least one cell from the border and
    whose centre lies up to 0.45 cells from that cell's centre; the centres in continuous heat coordinates"""
    cx = rng.integers(1, WH - 1, count) + 0.5 + rng.uniform(-0.45, 0.45, count)
    cy = rng.integers(1, HH - 1, count) + 0.5 + rng.uniform(-0.45, 0.45, count)
    x, y = np.arange(WH) + 0.5, np.arange(HH) + 0.5
    g = np.exp(-((x[None, None, :] - cx[:, None, None]) ** 2 + (y[None, :, None] - cy[:, None, None]) ** 2)
               / (2 * SIGMA ** 2))
    return g.astype(dtype).astype(F)[:, None], cx, cy


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_planted_gaussians_come_back_within_a_quarter_cell(dtype):
    """The quarter-cell refinement is within 0.25 cells of the centre along each heat axis.  A heat cell is w / Wh by
    h / Hh canvas pixels, and a canvas step (du, dv) moves the frame point by (a du + b dv, d du + e dv): each frame axis
    may be off by 0.25 (|a| w / Wh + |b| h / Hh), the 0.25 cells scaled by the mapping, plus 2^-6 for the float32
    arithmetic of steps 4 and 5 at coordinates below 2^12 (an ulp is 2^-12 there; a handful of roundings)."""
    rng = np.random.default_rng(7 if dtype == "float32" else 8)
    count = 300
    heat, cx, cy = gaussians(rng, count, dtype)
    w, h = CANVAS
    cell = (w / WH, h / HH)
    # a random similarity per slot: scale 0.5 .. 3, any angle, a shift into a 2000 x 1500 frame
    s, th = rng.uniform(0.5, 3.0, count), rng.uniform(0, 2 * np.pi, count)
    mats = np.stack([s * np.cos(th), -s * np.sin(th), rng.uniform(0, 2000, count), s * np.sin(th), s * np.cos(th),
                     rng.uniform(0, 1500, count)], 1).astype(F)
    _, kp = kd.decode([(2000, 1500)], kd.matrix_rows([0] * count, mats), 0, CANVAS, heat=heat)
    m64 = mats.astype(np.float64)
    cu, cv = cx * cell[0], cy * cell[1]
    tx, ty = m64[:, 0] * cu + m64[:, 1] * cv + m64[:, 2], m64[:, 3] * cu + m64[:, 4] * cv + m64[:, 5]
    bx = 0.25 * (abs(m64[:, 0]) * cell[0] + abs(m64[:, 1]) * cell[1]) + 2.0 ** -6
    by = 0.25 * (abs(m64[:, 3]) * cell[0] + abs(m64[:, 4]) * cell[1]) + 2.0 ** -6
    assert (abs(kp[:, 0, 0] - tx) <= bx).all() and (abs(kp[:, 0, 1] - ty) <= by).all()
    assert np.array_equal(kp[:, 0, 2], heat.reshape(count, -1).max(1))

    # the same maps through roi records: placement (dst) = the whole canvas, sources of any size in the frame
    rois = np.zeros((count, 8), np.int32)
    rois[:, 0], rois[:, 1] = rng.integers(0, 1500, count), rng.integers(0, 1000, count)
    rois[:, 2], rois[:, 3] = rng.integers(20, 500, count), rng.integers(20, 500, count)
    rois[:, 6], rois[:, 7] = w, h
    _, kp = kd.decode([(2000, 1500)] * count, rois, 1, CANVAS, heat=heat)
    sx, sy = rois[:, 2] / w, rois[:, 3] / h
    assert (abs(kp[:, 0, 0] - (cu * sx + rois[:, 0])) <= 0.25 * sx * cell[0] + 2.0 ** -6).all()
    assert (abs(kp[:, 0, 1] - (cv * sy + rois[:, 1])) <= 0.25 * sy * cell[1] + 2.0 ** -6).all()


# ---- (iii) the edges of the definition ----------------------------------------------------------------------------------
def one(heat, **kw):
    heat = np.asarray(heat, F)
    kw.setdefault("thr", -np.inf)
    pts, kp = kd.decode([(100, 100)], IDENTITY, 0, heat.shape[::-1], heat=heat[None, None], **kw)
    return tuple(int(v) for v in pts[0, 0]), tuple(kp[0, 0])


def test_ties_go_to_the_lowest_index_and_zeros_are_equal():
    pts, _ = one([[1, 5, 5], [5, 0, 5]], refine="none")
    assert pts[:2] == (1, 0)
    pts, kp = one([[-1, -0.0, 0.0], [0.0, -2, -0.0]], refine="none", thr=-1.0)
    assert pts == (1, 0, bits(-0.0), 3) and np.signbit(kp[2])
    pts, _ = one([[-1, 0.0, -0.0]], refine="none", thr=-1.0)
    assert pts == (1, 0, bits(0.0), 3)


def test_a_nan_never_wins_and_infinities_are_values():
    nan, inf = np.nan, np.inf
    pts, _ = one([[nan, -7, nan], [nan, -9, nan]], refine="none")
    assert pts == (1, 0, bits(-7), 3)
    pts, _ = one([[3, inf, nan, inf]], refine="none")
    assert pts == (1, 0, bits(inf), 3)


def test_minus_infinity_is_a_peak_but_not_above_a_threshold_of_minus_infinity():
    pts, kp = kd.decode([(100, 100)], IDENTITY, 0, (2, 1), heat=np.asarray([[[[-np.inf, np.nan]]]], F), thr=-np.inf,
                        refine="none")
    assert tuple(pts[0, 0]) == (0, 0, bits(-np.inf), 0) and kp[0, 0, 0] == F(0.5) and kp[0, 0, 2] == -np.inf


def test_a_map_of_nans_has_no_peak():
    pts, kp = one([[np.nan, np.nan], [np.nan, np.nan]])
    assert pts == (0, 0, kd.NAN_BITS, 0)
    assert kp[0] == 0 and kp[1] == 0 and np.isnan(kp[2])
    # SimCC: no peak in either vector
    x, y = np.asarray([[[1, 2, 3]]], F), np.full((1, 1, 4), np.nan, F)
    for sim in ((x, y), (y, x)):
        pts, kp = kd.decode([(100, 100)], IDENTITY, 0, (3, 4), simcc=sim, refine="none")
        assert tuple(pts[0, 0]) == (0, 0, kd.NAN_BITS, 0) and np.isnan(kp[0, 0, 2])


def test_simcc_takes_the_smaller_confidence():
    x, y = np.asarray([[[0.1, 0.9, 0.9]]], F), np.asarray([[[0.2, 0.1, 0.7, 0.3]]], F)
    pts, kp = kd.decode([(100, 100)], IDENTITY, 0, (3, 4), simcc=(x, y), refine="none")
    assert tuple(pts[0, 0]) == (1, 2, bits(0.7), 3) and tuple(kp[0, 0]) == (F(1.5), F(2.5), F(0.7))


def test_refinement_on_borders_corners_ties_and_nans():
    q = F(0.25)
    base = np.zeros((4, 5), F)
    for (yp, xp), want in {(0, 0): (0, 0), (0, 4): (0, 0), (3, 0): (0, 0), (3, 4): (0, 0), (0, 2): (q, 0), (3, 2): (q, 0),
                           (1, 0): (0, q), (2, 4): (0, -q), (1, 2): (q, q)}.items():
        h = base.copy()
        h[yp, xp] = 9
        if 0 < xp < 4:
            h[yp, xp + 1], h[yp, xp - 1] = 2, 1
        if 0 < yp < 3:
            sign = 1 if want[1] > 0 else -1
            h[yp + sign, xp], h[yp - sign, xp] = 2, 1
        _, kp = one(h)
        assert (kp[0] - (xp + F(0.5)), kp[1] - (yp + F(0.5))) == want, (yp, xp)
    h = base.copy()
    h[1, 2], h[1, 1], h[1, 3], h[0, 2], h[2, 2] = 9, 3, 3, np.nan, 1          # equal neighbours; a NaN neighbour
    _, kp = one(h)
    assert (kp[0], kp[1]) == (F(2.5), F(1.5))
    _, kp = one(h, refine="none")
    assert (kp[0], kp[1]) == (F(2.5), F(1.5))


def test_alignments():
    h = np.zeros((4, 8), F)
    h[2, 5], h[2, 6] = 1, 0.5
    pts, kp = kd.decode([(100, 100)], IDENTITY, 0, (32, 12), heat=h[None, None], align="centre")
    assert (kp[0, 0, 0], kp[0, 0, 1]) == (F(23.0), F(7.5))               # (5 + 0.5 + 0.25) * 4, (2 + 0.5) * 3
    pts, kp = kd.decode([(100, 100)], IDENTITY, 0, (32, 12), heat=h[None, None], align="index")
    assert (kp[0, 0, 0], kp[0, 0, 1]) == (F(21.5), F(6.5))               # (5 + 0.25) * 4 + 0.5, 2 * 3 + 0.5


def test_skipped_slots_and_flags():
    h = np.zeros((6, 1, 2, 2), F)
    h[:, 0, 1, 1] = 1
    rows = kd.matrix_rows([0, 1, -1, 2, 0, 0], [[1, 0, 0, 0, 1, 0]] * 3 + [[1, 0, 0, 0, 1, 0], [1, 0, 50, 0, 1, 0],
                                                                           [np.nan, 0, 0, 0, np.inf, 0]])
    pts, kp = kd.decode([(10, 10), (1, 1)], rows, 0, (2, 2), heat=h, refine="none")
    assert tuple(pts[0, 0]) == (1, 1, bits(1), 3)
    assert tuple(pts[1, 0]) == (1, 1, bits(1), 1)                        # frame 1 is 1 x 1: visible, outside
    assert not pts[2].any() and not pts[3].any() and not kp[2].any() and not kp[3].any()       # frames -1 and 2 of 2
    assert tuple(pts[4, 0]) == (51, 1, bits(1), 1)
    assert tuple(pts[5, 0]) == (0, 0, bits(1), 0) and np.isnan(kp[5, 0, 0]) and kp[5, 0, 1] == np.inf
    rois = np.asarray([[4, 6, 20, 30, 0, 0, 2, 2], [0, 0, 0, 0, 0, 0, 0, 0], [4, 6, 20, 30, 0, 0, 0, 2],
                       [4, 6, -1, 30, 0, 0, 2, 2]], np.int32)
    pts, kp = kd.decode([(100, 100), (100, 100)], rois, 2, (2, 2), heat=h[:4], refine="none")
    assert tuple(pts[0, 0]) == (19, 28, bits(1), 3) and tuple(kp[0, 0]) == (F(19), F(28.5), F(1))
    assert not pts[1:].any() and not kp[1:].any()


def test_sanitise_is_the_drawers_rule():
    pts = np.asarray([[[5, 5, 7, 1], [5, 5, 7, 2], [5, 5, 7, 7], [-65536, 131071, 0, 1], [-65537, 0, 0, 1],
                       [0, 131072, 0, 3], [200, 5, 9, 3], [5, 5, 7, -1]]], np.int32)
    got = kd.sanitise(pts, [(100, 100)], 1)[0].tolist()
    assert got == [[5, 5, 7, 3], [0] * 4, [5, 5, 7, 3], [-65536, 131071, 0, 1], [0] * 4, [0] * 4, [200, 5, 9, 1],
                   [5, 5, 7, 3]]


# ---- (iv) the errors, without a device ----------------------------------------------------------------------------------
def test_layout_errors():
    from vali_amd import keypoints as kp

    f32, f16, bf16, i32 = (2, 32), (2, 16), (4, 16), (0, 32)
    assert kp.heat_layout((2, 17, 64, 48), None, *f16) == (1, (2, 17, 64, 48), (17 * 3072, 3072, 48, 1))
    assert kp.heat_layout((2, 17, 64, 48), (0, 4000, 50, 1), *bf16)[2] == (0, 4000, 50, 1)
    assert kp.heat_layout((2, 17, 64, 1), (0, 64, 1, 7), *f32)[2] == (0, 64, 1, 7)           # one column: any x stride
    for shape, strides, dt, word in (((2, 17, 64), None, f32, "4-D"), ((2, 17, 64, 48), None, i32, "dtype"),
                                     ((0, 17, 64, 48), None, f32, "M = 0"), ((65536, 1, 1, 1), None, f32, "M = 65536"),
                                     ((1, 65, 4, 4), None, f32, "P = 65"), ((1, 1, 4097, 1), None, f32, "4097"),
                                     ((1, 1, 1024, 1025), None, f32, "exceeds 2.20"),
                                     ((2, 17, 64, 48), (1, 2, 96, 2), f32, "stride 1"),
                                     ((2, 17, 64, 48), (1, 2, -48, 1), f32, "negative")):
        with pytest.raises(ValueError, match=word):
            kp.heat_layout(shape, strides, *dt)
    lay = kp.simcc_layout("simcc_x")
    assert lay((3, 17, 384), None, *f32) == (0, (3, 17, 384), (17 * 384, 384, 1))
    for shape, strides, word in (((3, 17), None, "3-D"), ((3, 17, 4097), None, "W = 4097"),
                                 ((3, 17, 8), (136, 16, 2), "stride 1")):
        with pytest.raises(ValueError, match="simcc_x.*" + word):
            lay(shape, strides, *f32)
    with pytest.raises(ValueError, match="one dtype"):
        kp.simcc_pair((0, (3, 17, 8), None), (1, (3, 17, 8), None))
    with pytest.raises(ValueError, match="simcc_y"):
        kp.simcc_pair((0, (3, 17, 8), None), (0, (3, 16, 8), None))


def test_mapping_and_run_errors():
    from vali_amd import keypoints as kp

    t = object()
    assert kp.mapping_spec(3, 12, (192, 256), t, None, None) == (192, 256, 0)
    assert kp.mapping_spec(3, 12, (192, 256), None, t, 4) == (192, 256, 4)
    for args, word in (((3, 12, (192, 256), t, t, 4), "both"), ((3, 12, (192, 256), None, None, None), "neither"),
                       ((3, 12, (192, 256), None, t, None), "max_det is required"),
                       ((3, 12, (192, 256), None, t, 5), r"M = 12 slots for N \* max_det = 3 \* 5"),
                       ((3, 12, (192, 256), None, t, 0), "max_det = 0"), ((3, 12, (192, 256), t, None, 4), "max_det goes"),
                       ((3, 12, (0, 256), t, None, None), "canvas"), ((3, 12, 192, t, None, None), "canvas"),
                       ((0, 12, (192, 256), t, None, None), "frames")):
        with pytest.raises(ValueError, match=word):
            kp.mapping_spec(*args)
    assert kp.run_spec(0.3, "quarter", "centre", False) == (0.3, 1, 0)
    assert kp.run_spec(0.3, "none", "index", True) == (0.3, 0, 1)
    for args, word in (((float("nan"), "none", "centre", False), "NaN"), ((0.3, "dark", "centre", False), "refine"),
                       ((0.3, "none", "center", False), "align"), ((0.3, "quarter", "centre", True), "SimCC")):
        with pytest.raises(ValueError, match=word):
            kp.run_spec(*args)


def test_points_spec_errors():
    from vali_amd import pose

    assert pose.points_spec(3, (12, 17, 4), 4)[:3] == (3, 17, 4)
    for args, word in (((3, (12, 17, 4), None), "max_det is required"), ((3, (12, 17, 3), 4), "shape"),
                       ((3, (12, 17), 4), "shape"), ((3, (12, 65, 4), 4), "P = 65"), ((3, (13, 17, 4), 4), "13 rows"),
                       ((3, (12, 17, 4), 4, ((0, 17),)), "limbs"), ((0, (12, 17, 4), 4), "frames")):
        with pytest.raises(ValueError, match=word):
            pose.points_spec(*args)


class DecodeIn(ctypes.Structure):
    _fields_ = [("heat", ctypes.c_void_p), ("simcc_x", ctypes.c_void_p), ("simcc_y", ctypes.c_void_p),
                ("dtype", ctypes.c_int32), ("refine", ctypes.c_int32), ("align", ctypes.c_int32), ("max_det", ctypes.c_int32),
                ("stride_m", ctypes.c_int64), ("stride_p", ctypes.c_int64), ("stride_y", ctypes.c_int64),
                ("x_stride_m", ctypes.c_int64), ("x_stride_p", ctypes.c_int64), ("y_stride_m", ctypes.c_int64),
                ("y_stride_p", ctypes.c_int64), ("m", ctypes.c_int32), ("p", ctypes.c_int32), ("hh", ctypes.c_int32),
                ("wh", ctypes.c_int32), ("canvas_w", ctypes.c_int32), ("canvas_h", ctypes.c_int32),
                ("kpt_thr", ctypes.c_float), ("reserved", ctypes.c_int32)]


def test_c_abi_refuses_invalid_arguments_before_any_device():
    """pointers are never followed by the checks: made-up aligned addresses stand in for device memory"""
    assert ctypes.sizeof(DecodeIn) == 128
    lib = ctypes.CDLL(str(ROOT / "vali_amd" / "libvali_hip.so"))
    lib.vali_last_error.restype = ctypes.c_char_p
    fn = lib.vali_kpt_decode
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(DecodeIn)] + [ctypes.c_void_p] * 5
    A = 0x10000

    def good(**kw):
        d = dict(heat=A, dtype=1, refine=1, align=0, stride_m=17 * 3072, stride_p=3072, stride_y=48, m=12, p=17, hh=64,
                 wh=48, canvas_w=192, canvas_h=256, kpt_thr=0.3, max_det=4)
        d.update(kw)
        return DecodeIn(**d)

    def call(inp, frames=A, n=3, mats=A, rois=None, points=A, kpts=None):
        return fn(frames, n, ctypes.byref(inp) if inp is not None else None, mats, rois, points, kpts, None)

    simcc = dict(heat=None, simcc_x=A, simcc_y=A, refine=0, x_stride_m=17 * 48, x_stride_p=48, y_stride_m=17 * 64, y_stride_p=64)
    cases = [(dict(), dict(frames=None), "null"), (dict(), dict(points=None), "null"), (None, dict(), "null"),
             (dict(), dict(mats=None), "exactly one"), (dict(), dict(rois=A), "exactly one"),
             (dict(), dict(n=0), "n outside"), (dict(), dict(n=1025), "n outside"),
             (dict(simcc_x=A), dict(), "at once"), (dict(heat=None), dict(), "neither heat"),
             (dict(heat=None, simcc_x=A), dict(), "neither heat"),
             (dict(dtype=3), dict(), "dtype"), (dict(m=0), dict(), "m outside"), (dict(m=65536), dict(), "m outside"),
             (dict(p=65), dict(), "p outside"), (dict(hh=0), dict(), "hh or wh"), (dict(wh=4097), dict(), "hh or wh"),
             (dict(hh=1024, wh=1025), dict(), "2\\^20"), (dict(canvas_w=0), dict(), "canvas"),
             (dict(canvas_h=65536), dict(), "canvas"), (dict(refine=2), dict(), "refine"), (dict(align=2), dict(), "align"),
             (dict(kpt_thr=float("nan")), dict(), "NaN"), (dict(heat=A + 1), dict(), "aligned to its element"),
             (dict(dtype=0, heat=A + 2), dict(), "aligned to its element"), (dict(stride_y=-1), dict(), "stride"),
             (dict(stride_m=(1 << 40) + 1), dict(), "stride"),
             (dict(simcc, refine=1), dict(), "SimCC"), (dict(simcc, simcc_y=A + 1), dict(), "aligned to its element"),
             (dict(simcc, x_stride_p=-1), dict(), "stride"),
             (dict(max_det=5), dict(mats=None, rois=A), "n \\* max_det"), (dict(max_det=0), dict(mats=None, rois=A), "max_det"),
             (dict(), dict(mats=A + 2), "4-byte"), (dict(), dict(kpts=A + 2), "4-byte"), (dict(), dict(points=A + 8), "16-byte")]
    import re
    for fields, args, word in cases:
        inp = None if fields is None else good(**fields)
        assert call(inp, **args) == -1, (fields, args)
        assert re.search(word, lib.vali_last_error().decode()), (fields, args, lib.vali_last_error())

    pp = lib.vali_pose_paint_points
    pp.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                   ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                   ctypes.c_void_p]
    assert pp(None, A, 1, 0, A, 17, 4, A, 19, A, None, A, 1 << 20, None) == -1 and b"null" in lib.vali_last_error()
    assert pp(A, A, 1, 0, None, 17, 4, A, 19, A, None, A, 1 << 20, None) == -1 and b"null" in lib.vali_last_error()
