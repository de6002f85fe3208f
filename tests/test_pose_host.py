"""Pose skeletons without a GPU: the numpy model (tests/pose_model.py) against Python integers and against the stamp
model, the float32 mapping against the selector's, the conditions the shared fixtures (tests/pose_cases.py) must hold, the
Python checks, and what the C entry point refuses before any device is touched."""
import numpy as np
import pytest

import annotate_model as am
import annotate_stamp_model as sm
import detect_model as dm
import pose_cases as pc
import pose_model as po
import postproc_model as pm

ROWS_601 = "601_JPEG"


# ---- coverage: the model against Python integers -------------------------------------------------------------------------
def random_segments(rng, count):
    """segments near a 96 x 80 window, of every slope, some with an end at the limits of a visible keypoint"""
    ends = [-65536, 131071]
    for _ in range(count):
        A = [int(rng.integers(-20, 116)), int(rng.integers(-20, 100))]
        B = [int(rng.integers(-20, 116)), int(rng.integers(-20, 100))]
        kind = int(rng.integers(0, 6))
        if kind == 0:
            B[0] = ends[int(rng.integers(0, 2))]
        elif kind == 1:
            B[1] = ends[int(rng.integers(0, 2))]
        elif kind == 2:
            B = [ends[int(rng.integers(0, 2))], ends[int(rng.integers(0, 2))]]
        yield A, B, int(rng.choice([1, 2, 3, 4, 7, 33, 64]))


def test_a_limb_is_the_exact_integer_rule_pixel_by_pixel():
    rng = np.random.default_rng(1)
    xs, ys = np.arange(96), np.arange(80)
    far = 0
    for A, B, t in random_segments(rng, 60):
        got = po.limb_cover(A, B, t, xs, ys)
        want = np.array([[po.covers_exact(A, B, t, (x, y)) for x in xs] for y in ys])
        assert np.array_equal(got, want), (A, B, t)
        far += max(abs(B[0]), abs(B[1])) > 60000
    assert far >= 10


def dist2_rational(A, B, P):
    """the squared distance of P from the segment AB as a fraction (numerator, denominator) of Python integers"""
    ex, ey, qx, qy = B[0] - A[0], B[1] - A[1], P[0] - A[0], P[1] - A[1]
    L2, s = ex * ex + ey * ey, qx * ex + qy * ey
    if L2 == 0 or s <= 0:
        return qx * qx + qy * qy, 1
    if s >= L2:
        return (P[0] - B[0]) ** 2 + (P[1] - B[1]) ** 2, 1
    c = qx * ey - qy * ex
    return c * c, L2                    # |q|^2 - s^2 / L2 = c^2 / L2


def test_a_limb_is_every_pixel_within_half_the_thickness_of_the_segment():
    """the union over the segment's points of the discs of diameter t, as an exact rational distance test"""
    rng = np.random.default_rng(2)
    xs, ys = np.arange(96), np.arange(80)
    for A, B, t in random_segments(rng, 40):
        got = po.limb_cover(A, B, t, xs, ys)
        for y in range(0, 80, 3):
            for x in range(0, 96, 3):
                num, den = dist2_rational(A, B, (x, y))
                assert bool(got[y, x]) == (4 * num <= t * t * den), (A, B, t, x, y)


def test_thickness_1_leaves_no_gap_along_a_line_at_any_slope():
    """every pixel column (or row, for steep lines) between the ends holds a pixel, and neighbours touch (8-connected)"""
    rng = np.random.default_rng(3)
    xs, ys = np.arange(96), np.arange(80)
    lines = [((3, 3), (90, 3)), ((3, 3), (3, 70)), ((3, 3), (73, 73)), ((5, 70), (90, 4)), ((2, 2), (93, 3)), ((2, 2), (3, 77))]
    lines += [((int(a), int(b)), (int(c), int(d))) for a, b, c, d in
              zip(rng.integers(0, 96, 40), rng.integers(0, 80, 40), rng.integers(0, 96, 40), rng.integers(0, 80, 40))]
    for A, B in lines:
        cover = po.limb_cover(A, B, 1, xs, ys)
        assert cover[A[1], A[0]] and cover[B[1], B[0]]
        wide = abs(B[0] - A[0]) >= abs(B[1] - A[1])
        along = cover.any(0) if wide else cover.any(1)
        lo, hi = sorted((A[0], B[0]) if wide else (A[1], B[1]))
        assert along[lo:hi + 1].all(), (A, B)
        # one component: grow from A through 8-neighbours
        seen, todo = {tuple(A)}, [tuple(A)]
        while todo:
            x, y = todo.pop()
            for dx in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    n = (x + dx, y + dy)
                    if 0 <= n[0] < 96 and 0 <= n[1] < 80 and cover[n[1], n[0]] and n not in seen:
                        seen.add(n)
                        todo.append(n)
        assert len(seen) == int(cover.sum()), (A, B)


def test_a_limb_of_no_length_is_the_disc_of_its_thickness():
    xs, ys = np.arange(96), np.arange(80)
    for t in (1, 2, 3, 7, 8, 64):
        disc = po.joint_cover((40, 33), t, xs, ys)
        assert np.array_equal(po.limb_cover((40, 33), (40, 33), t, xs, ys), disc)
        yy, xx = np.mgrid[0:80, 0:96]
        assert np.array_equal(disc, 4 * ((xx - 40) ** 2 + (yy - 33) ** 2) <= t * t)
        assert disc[33, 40] and disc.sum() >= 1
    assert po.joint_cover((40, 33), 1, xs, ys).sum() == 1 and po.joint_cover((40, 33), 2, xs, ys).sum() == 5


def test_skipping_the_square_of_a_large_c_never_changes_a_result():
    """t^2 L2 <= 64^2 * 2 * 196607^2 < 2^49, so 4 c^2 <= t^2 L2 fails wherever |c| >= 2^24: k_pose_paint never forms the
    square of such a c (it compares |c| with isqrt(t^2 L2 / 4) < 2^24), the model none of a |c| >= 2^30.  A bound of 2^23
    would not do: the longest limb at thickness 64 lets |c| up to 8897417 > 2^23 in."""
    assert 64 * 64 * 2 * 196607 ** 2 < 1 << 49
    rng = np.random.default_rng(4)
    for A, B, t in list(random_segments(rng, 300)) + [((-65536, -65536), (131071, 131071), 64)]:
        ex, ey = B[0] - A[0], B[1] - A[1]
        L2 = ex * ex + ey * ey
        for _ in range(20):
            P = (int(rng.integers(0, 65536)), int(rng.integers(0, 65536)))
            c = (P[0] - A[0]) * ey - (P[1] - A[1]) * ex
            if abs(c) >= 1 << 24:
                assert 4 * c * c > t * t * L2
    import math
    A, B, t = (-65536, -65536), (131071, 131071), 64
    L2 = 2 * 196607 ** 2
    cmax = math.isqrt(t * t * L2 // 4)
    assert cmax == 8897417 and 1 << 23 < cmax < 1 << 24
    # pixels beside the diagonal: c = (x - y) * 196607
    assert po.covers_exact(A, B, t, (145, 100)) and (145 - 100) * 196607 > 1 << 23
    assert not po.covers_exact(A, B, t, (146, 100))
    assert po.limb_cover(A, B, t, np.arange(100, 200), np.array([100]))[0].tolist() == [x - 100 <= 45 for x in range(100, 200)]


# ---- the mapping ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rect", pc.RECTS + [(3, 7, 1919, 1073, 0, 140, 640, 360)])
def test_the_mapping_is_the_selectors(rect):
    """detect_model.to_pixels floors (x1 - dst_x) * sx + src_x for a box's first corner; away from its clamp to the source
    rectangle that is X and Y"""
    rng = np.random.default_rng(5)
    sx, sy, sw, sh, dx, dy, dw, dh = rect
    kx = rng.uniform(dx, dx + dw, 500).astype(np.float32)
    ky = rng.uniform(dy, dy + dh, 500).astype(np.float32)
    box = np.stack([kx, ky, kx + 1, ky + 1], 1).astype(np.float32)
    x, y, _, _ = dm.to_pixels(box, rect)
    kp = np.stack([kx, ky, np.ones(500, np.float32)], 1)
    pts = po.row_points(kp, rect, (1 << 20, 1 << 20), 0.5)
    inner = (x > sx) & (x < sx + sw) & (y > sy) & (y < sy + sh)
    assert inner.sum() > 400
    assert np.array_equal(pts[inner, 0], x[inner]) and np.array_equal(pts[inner, 1], y[inner])
    assert (pts[:, 3] == 3).all()


def test_visibility_and_the_points_row():
    rect, size = pc.RECTS[0], pc.SIZES[0]
    inf, nan = np.inf, np.nan
    kp = np.array([[10, 20, 0.9], [10, 20, 0.5], [10, 20, nan], [nan, 20, 0.9], [10, inf, 0.9], [-inf, 20, 0.9],
                   [-65535.5 / 1.5, 20, 0.9], [-65536.5 / 1.5, 20, 0.9], [131071.5 / 1.5, 20, 0.9], [131072 / 1.5, 20, 0.9],
                   [70, 20, 0.9], [10, 4, 0.9], [3e38, 20, 0.9]], np.float32)
    pts = po.row_points(kp, rect, size, 0.5)
    assert pts[:, 3].tolist() == [3, 0, 0, 0, 0, 0, 1, 0, 1, 0, 1, 1, 0]
    assert pts[0, :2].tolist() == [15, 22] and pts[6, 0] == -65536 and pts[8, 0] == 131071
    assert pts[10, :2].tolist() == [105, 22] and pts[11, :2].tolist() == [15, -2]          # visible, outside the frame
    assert (pts[pts[:, 3] == 0, :2] == 0).all()
    assert pts[:, 2].astype(np.int32).view(np.float32)[0] == np.float32(0.9) and np.isnan(pts[2, 2].astype(np.int32).view(np.float32))
    two = po.row_points(kp[:, :2], rect, size, 0.5)
    assert (two[:, 2] == 0x3F800000).all() and two[1, 3] == 3 and two[2, 3] == 3
    assert (po.row_points(kp, rect, size, np.inf)[:, 3] == 0).all()


# ---- conditions on the fixtures ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_every_fixture_row_has_3_visible_keypoints_and_paints_1_to_60_percent(dtype):
    """no GPU test passes on an empty drawing"""
    kpts = pc.kpts(pc.P, dtype)
    for rows, painted in ((pc.PLACEMENTS, set(range(8))), (pc.SKIPS, pc.SKIPS_PAINTED)):
        frames = pc.noise_frames("RGB")
        points, drawn = po.apply(frames, "RGB", pc.SIZES, rows, pc.D, kpts, pc.RECTS, pc.LIMBS, pc.LIMB_COLOURS,
                                 pc.JOINT_COLOURS, pc.THR)
        assert {d[0] for d in drawn} == painted
        for idx in painted:
            assert (points[idx, :, 3] != 0).sum() >= 3, idx
            w, h = pc.SIZES[idx // pc.D]
            union = np.zeros((h, w), bool)
            for d in drawn:
                if d[0] == idx:
                    union |= d[3]
            assert 0.01 <= union.mean() <= 0.60, (idx, union.mean())
        for idx in set(range(8)) - painted:
            assert not points[idx].any()


def test_the_fixtures_are_what_their_names_say():
    kpts = pc.kpts()
    pts = po.points_of(pc.SIZES, pc.PLACEMENTS, pc.D, kpts, pc.RECTS, pc.THR)
    assert pts[0, :2, :2].tolist() == [[50, 50], [78, 78]]                 # PLACEMENTS[0] has k = 3: through (64, 64)
    assert pts[4, :2, :2].tolist() == [[58, 10], [68, 40]]                 # PLACEMENTS[4] has k = 5: across x = 64
    assert (pts[:, :, 3] == 3).sum() >= 30 and ((pts[:, 4, 3] == 0) == (np.asarray(pc.PLACEMENTS)[:, 7] % 2 == 1)).all()
    far = po.points_of(pc.SIZES, pc.PLACEMENTS, pc.D, pc.far_kpts(), pc.RECTS, pc.THR)
    assert far[0, 0, 0] == -65536 and far[1, 1, 0] == 131071 and far[2, 0, 1] == -65536 and far[3, 1, 1] == 131071
    assert (far[:4, 2, 3] == 0).all() and (far[:4, 2, :2] == 0).all()
    assert far[0, 0, 3] == 1 and far[1, 1, 3] == 1 and far[2, 0, 3] == 1 and far[3, 1, 3] == 1
    odd = po.points_of(pc.SIZES, pc.PLACEMENTS, pc.D, pc.odd_kpts(), pc.RECTS, pc.THR)
    for idx, row in enumerate(pc.PLACEMENTS):
        assert (odd[idx, :, 3] != 0).tolist() == ([True, False, True, False, False] if row[7] % 2 else
                                                    [False, True, False, False, True]), idx


# ---- the model's frames against the stamp model ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", am.FORMATS)
def test_drawing_is_stamping_the_shapes_from_an_atlas(fmt):
    kpts = pc.kpts()
    rows = pm.matrices()[ROWS_601]
    for dets, alpha, t, d in ((pc.PLACEMENTS, None, 3, 7), (pc.SKIPS, 128, 2, 4), (pc.PLACEMENTS, 255, 1, 64)):
        a, b = pc.noise_frames(fmt), pc.noise_frames(fmt)
        _, drawn = po.apply(a, fmt, pc.SIZES, dets, pc.D, kpts, pc.RECTS, pc.LIMBS, pc.LIMB_COLOURS, pc.JOINT_COLOURS,
                            pc.THR, t, d, alpha, rows)
        assert len({d[0] for d in drawn}) == (8 if dets is pc.PLACEMENTS else 2)
        atlas, marks = po.stamp_atlas(drawn)
        assert len(marks) >= 0.9 * len(drawn)
        assert sm.apply(b, fmt, pc.SIZES, marks, rows, atlas) == list(range(len(marks)))
        for i in range(2):
            assert np.array_equal(a[i], b[i]), (fmt, alpha, i)
            assert not np.array_equal(a[i], pc.noise_frames(fmt)[i])


def test_the_order_of_overlapping_shapes_is_visible():
    kpts = pc.kpts()
    a, b, c = pc.noise_frames("RGB"), pc.noise_frames("RGB"), pc.noise_frames("RGB")
    swapped = list(pc.PLACEMENTS)
    swapped[0], swapped[1] = swapped[1], swapped[0]
    args = (pc.D, kpts, pc.RECTS)
    po.apply(a, "RGB", pc.SIZES, pc.PLACEMENTS, *args, pc.LIMBS, pc.LIMB_COLOURS, pc.JOINT_COLOURS, pc.THR)
    po.apply(b, "RGB", pc.SIZES, swapped, *args, pc.LIMBS, pc.LIMB_COLOURS, pc.JOINT_COLOURS, pc.THR)
    po.apply(c, "RGB", pc.SIZES, pc.PLACEMENTS, *args, tuple(reversed(pc.LIMBS)), pc.LIMB_COLOURS, pc.JOINT_COLOURS, pc.THR)
    assert not np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0], c[0])


# ---- the Python checks -------------------------------------------------------------------------------------------------------------
F32, F16, BF16 = (2, 32), (2, 16), (4, 16)


def test_layouts_say_what_is_wrong():
    from vali_amd.pose import COCO_SKELETON, draw_spec, kpts_layout, pose_spec

    good = kpts_layout((2, 8400, 17, 3), None, *F16)
    assert good == (1, (2, 8400, 17, 3), (8400 * 51, 51, 3, 1))
    # a YOLOv8-pose head (N, 5 + 3 P, K): pred[:, 5:].transpose(1, 2).unflatten(2, (P, 3)); a broadcast
    head = kpts_layout((2, 8400, 17, 3), (56 * 8400, 1, 3 * 8400, 8400), *F32)
    assert head[2] == (56 * 8400, 1, 3 * 8400, 8400)
    assert kpts_layout((16, 8400, 17, 2), (0, 34, 2, 1), *BF16)[2][0] == 0
    for args, text in [(((2, 8400, 51), None, *F32), "4-D"), (((2, 8400, 17, 3), None, 0, 32), "dtype"),
                       (((0, 8400, 17, 3), None, *F32), "N = 0"), (((1025, 1, 1, 3), None, *F32), "N = 1025"),
                       (((2, 0, 17, 3), None, *F32), "K = 0"), (((2, 2**20 + 1, 17, 3), None, *F32), "K ="),
                       (((2, 8400, 0, 3), None, *F32), "P = 0"), (((2, 8400, 65, 3), None, *F32), "P = 65"),
                       (((2, 8400, 17, 4), None, *F32), "last dimension"), (((2, 8400, 17, 1), None, *F32), "last dimension"),
                       (((2, 8400, 17, 3), (1, 2, -3, 1), *F32), "negative strides"),
                       (((2, 8400, 17, 3), (2**41, 2, 3, 1), *F32), "beyond 2.40")]:
        with pytest.raises(ValueError, match=text):
            kpts_layout(*args)
    assert pose_spec(2, good, 100, COCO_SKELETON)[:5] == (2, 8400, 17, 3, 100)
    assert pose_spec(2, good, 100, COCO_SKELETON)[5][:4] == [15, 13, 13, 11] and len(COCO_SKELETON) == 19
    assert pose_spec(2, good, 1, ())[5] == []
    for kw, text in [(dict(n_frames=3), "3 surfaces"), (dict(max_det=0), "max_det = 0"), (dict(max_det=1025), "max_det = 1025"),
                     (dict(limbs=[(0, 17)]), r"pair 0 = \(0, 17\)"), (dict(limbs=[(0, 1), (-1, 2)]), "pair 1"),
                     (dict(limbs=[(0, 1, 2)]), "pairs"), (dict(limbs=5), "pairs"), (dict(limbs=[(0, 1)] * 129), "129 pairs")]:
        a = dict(n_frames=2, max_det=100, limbs=COCO_SKELETON)
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            pose_spec(a["n_frames"], good, a["max_det"], a["limbs"])
    with pytest.raises(ValueError, match="exceeds 65535"):
        pose_spec(1024, kpts_layout((1024, 1, 1, 3), None, *F32), 64, ())
    assert draw_spec([1, -2], (7,), 0.5, 3, 7, None) == ([1, -2], [7], 0.5, 3, 7, -1)
    assert draw_spec([1], [2], -np.inf, 1, 64, 255)[2:] == (-np.inf, 1, 64, 255)
    for args, text in [(([], [1], 0.5, 3, 7, None), "limb_colours: at least one"), (([1], [], 0.5, 3, 7, None), "joint_colours: at least one"),
                       (([1], [2**31], 0.5, 3, 7, None), "joint_colours: every colour"), ((5, [1], 0.5, 3, 7, None), "limb_colours"),
                       (([1], [1], np.nan, 3, 7, None), "kpt_thr"), (([1], [1], 0.5, 0, 7, None), "thickness = 0"),
                       (([1], [1], 0.5, 65, 7, None), "thickness = 65"), (([1], [1], 0.5, 3, 0, None), "diameter = 0"),
                       (([1], [1], 0.5, 3, 65, None), "diameter = 65"), (([1], [1], 0.5, 3, 7, 256), "alpha"),
                       (([1], [1], 0.5, 3, 7, -1), "alpha")]:
        with pytest.raises(ValueError, match=text):
            draw_spec(*args)


def test_the_names_are_exported():
    import python_vali
    import vali_amd

    for name in ("PyPoseDrawer", "PoseBatch", "COCO_SKELETON"):
        assert getattr(python_vali, name) is getattr(vali_amd, name)
    assert tuple(vali_amd.COCO_SKELETON) == po.COCO_SKELETON


# ---- the C entry points without a device ---------------------------------------------------------------------------------------------
def test_workspace_size():
    from vali_amd._native import shim

    assert shim.pose_workspace_size(16, 100, 17) == 16 * 100 * 18 * 16
    assert shim.pose_workspace_size(1, 1, 1) == 32
    assert shim.pose_workspace_size(63, 1024, 64) == 63 * 1024 * 65 * 16
    for bad in [(0, 1, 1), (1025, 1, 1), (1, 0, 1), (1, 1025, 1), (64, 1024, 1), (1, 1, 0), (1, 1, 65)]:
        assert shim.pose_workspace_size(*bad) == 0, bad


def test_the_entry_point_refuses_before_any_device_is_touched(vali):
    """the pointers below are dummies that are never read"""
    from vali_amd._native import shim

    def call(fmt="NV12", sizes=((64, 48), (2, 2)), descs=None, d_frames=0x1000, kpts=(0x2000, 1, 1000, 15, 3, 1), kdim=3,
             k=12, p=5, D=4, limbs=0x3000, nl=6, dets=0x4000, rects=0x5000, lc=0x6000, nlc=3, jc=0x6100, njc=2, thr=0.5,
             t=3, dia=7, alpha=-1, points=0x8000, params=True, ws=0x10000, ws_bytes=None, plane=0x7000, pitch=None):
        f = int(getattr(vali, fmt)) if isinstance(fmt, str) else fmt
        if descs is None:
            descs = [shim.SurfaceDesc([plane] * 3, [pitch or 3 * w] * 3, w, h, f) for w, h in sizes]
        if ws_bytes is None:
            ws_bytes = len(descs) * D * (1 + p) * 16
        prm = shim.CvtParams(None, [[0.25, 0.5, 0.25, 0.0]] * 3) if params else None
        rc = shim.pose_paint(descs, d_frames, f, kpts, kdim, k, p, D, limbs, nl, dets, rects, lc, nlc, jc, njc, thr, t, dia,
                             alpha, points, prm, ws, ws_bytes, 0)
        return rc, shim.last_error()

    cases = [
        (dict(d_frames=0), "null argument"), (dict(dets=0), "null argument"), (dict(rects=0), "null argument"),
        (dict(ws=0), "null argument"), (dict(descs=[]), "null argument"),
        (dict(sizes=[(2, 2)] * 1025), "n outside"), (dict(k=0), "k outside"), (dict(k=2**20 + 1), "k outside"),
        (dict(p=0), "p outside"), (dict(p=65), "p outside"), (dict(kdim=1), "kdim"), (dict(kdim=4), "kdim"),
        (dict(D=0), "max_det outside"), (dict(D=1025), "max_det outside"),
        (dict(sizes=[(2, 2)] * 1024, D=64, ws_bytes=2**40), "exceeds 65535"),
        (dict(nl=-1), "n_limbs outside"), (dict(nl=129), "n_limbs outside"), (dict(limbs=0), "limbs has a null pointer"),
        (dict(kpts=(0, 1, 1000, 15, 3, 1)), "kpts has a null pointer"), (dict(kpts=(0x2000, 3, 1000, 15, 3, 1)), "dtype 3"),
        (dict(kpts=(0x2000, -1, 1000, 15, 3, 1)), "dtype -1"), (dict(kpts=(0x2001, 1, 1000, 15, 3, 1)), "not aligned to its element"),
        (dict(kpts=(0x2002, 0, 1000, 15, 3, 1)), "not aligned to its element"),
        (dict(kpts=(0x2000, 1, -1, 15, 3, 1)), "strides"), (dict(kpts=(0x2000, 1, 1000, 15, 3, 2**41)), "strides"),
        (dict(lc=0), "limb_colours or joint_colours"), (dict(jc=0), "limb_colours or joint_colours"),
        (dict(nlc=0), "below 1"), (dict(njc=0), "below 1"), (dict(thr=float("nan")), "kpt_thr"),
        (dict(t=0), "thickness outside"), (dict(t=65), "thickness outside"), (dict(dia=0), "diameter outside"),
        (dict(dia=65), "diameter outside"), (dict(alpha=256), "alpha outside"), (dict(alpha=-2), "alpha outside"),
        (dict(dets=0x4002), "not 4-byte aligned"), (dict(rects=0x5001), "not 4-byte aligned"),
        (dict(lc=0x6002), "not 4-byte aligned"), (dict(jc=0x6101), "not 4-byte aligned"), (dict(limbs=0x3002), "not 4-byte aligned"),
        (dict(points=0x8008), "points is not 16-byte aligned"),
        (dict(sizes=((64, 48), (3, 2))), "even width and height"), (dict(sizes=((64, 48), (0, 2))), "outside 1..65535"),
        (dict(sizes=((64, 48), (65536, 2)), fmt="RGB"), "outside 1..65535"), (dict(plane=0), "plane 0 is null"),
        (dict(pitch=63), "shorter than a row"), (dict(params=False), "needs params"),
        (dict(ws=0x10008), "not 16-byte aligned"), (dict(ws_bytes=2 * 4 * 6 * 16 - 1), "workspace is smaller"),
    ]
    for kw, text in cases:
        rc, err = call(**kw)
        assert rc == -1 and rc == shim.ERR_INVALID_ARG and text in err and "vali_pose_paint" in err, (kw, rc, err)
    mixed = [shim.SurfaceDesc([0x7000] * 3, [192] * 3, 64, 48, int(vali.NV12)),
             shim.SurfaceDesc([0x7000] * 3, [192] * 3, 64, 48, int(vali.YUV420))]
    rc, err = call(descs=mixed)
    assert rc == shim.ERR_INVALID_ARG and "one format per batch" in err
    rc, err = call(fmt=int(vali.Y))
    assert rc == shim.ERR_UNSUPPORTED and "format" in err
