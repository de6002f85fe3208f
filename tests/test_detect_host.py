"""PyDetectionSelector without a GPU: the numpy model (tests/detect_model.py) against a second, scalar implementation of the
definition in include/vali_hip.h; hand-made cases checked by value; every ValueError of Prepare / Run and every
VALI_ERR_INVALID_ARG of vali_detect_select, which are decided before any device is touched."""
import ctypes
import math
from pathlib import Path

import numpy as np
import pytest

import detect_model as dm

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
LETTERBOX = (0, 0, 1920, 1080, 0, 140, 640, 360)     # letterbox_rect(1920, 1080, 640, 640) = (0, 140, 640, 360)


# ---- a second implementation: Python loops over np.float32 scalars ------------------------------------------------------
def naive_select(boxes, scores, rects, score_thr, iou_thr, agnostic, box_format, T, D):
    n, K, C = scores.shape
    dets = [[-1, 0, 0, 0, 0, 0, 0, 0] for _ in range(n * D)]
    counts = [0] * n
    thr, ithr = F(score_thr), F(iou_thr)
    for i in range(n):
        sx_, sy_, sw, sh, dx_, dy_, dw, dh = (int(v) for v in rects[i])
        if min(sw, sh, dw, dh) < 1:
            continue
        cands = []
        for k in range(K):
            s, cls = F(-np.inf), 0
            for c in range(C):
                v = scores[i, k, c]
                if v > s:
                    s, cls = v, c
            if not s > thr:
                continue
            b = [F(v) for v in boxes[i, k]]
            if box_format == "cxcywh":
                hw, hh = F(b[2] * F(0.5)), F(b[3] * F(0.5))
                x1, x2, y1, y2 = F(b[0] - hw), F(b[0] + hw), F(b[1] - hh), F(b[1] + hh)
            else:
                x1, y1, x2, y2 = b
            ex1, ey1, ex2, ey2 = F(dx_), F(dy_), F(dx_ + dw), F(dy_ + dh)
            x1 = ex1 if ex1 > x1 else x1
            y1 = ey1 if ey1 > y1 else y1
            x2 = ex2 if ex2 < x2 else x2
            y2 = ey2 if ey2 < y2 else y2
            if not all(math.isfinite(float(v)) for v in (x1, y1, x2, y2)) or not (x2 > x1 and y2 > y1):
                continue
            cands.append((s, k, cls, (x1, y1, x2, y2)))
        cands = sorted(cands, key=lambda t: (-float(t[0]), t[1]))[:T]      # -(-0.0) == -(0.0) as floats
        kept = []
        for s, k, cls, bj in cands:
            gone = False
            for _, _, ci, bi in kept:
                if not (agnostic or ci == cls):
                    continue
                iw = max(F(min(bi[2], bj[2]) - max(bi[0], bj[0])), F(0))
                ih = max(F(min(bi[3], bj[3]) - max(bi[1], bj[1])), F(0))
                inter = F(iw * ih)
                ai, aj = F(F(bi[2] - bi[0]) * F(bi[3] - bi[1])), F(F(bj[2] - bj[0]) * F(bj[3] - bj[1]))
                uni = F(F(ai + aj) - inter)
                if inter > F(ithr * uni):
                    gone = True
                    break
            if not gone and len(kept) < D:
                kept.append((s, k, cls, bj))
            if len(kept) == D:
                break
        fx, fy = F(F(sw) / F(dw)), F(F(sh) / F(dh))
        for r, (s, k, cls, b) in enumerate(kept):
            X1 = math.floor(float(F(F(F(b[0] - F(dx_)) * fx) + F(sx_))))
            X2 = math.ceil(float(F(F(F(b[2] - F(dx_)) * fx) + F(sx_))))
            Y1 = math.floor(float(F(F(F(b[1] - F(dy_)) * fy) + F(sy_))))
            Y2 = math.ceil(float(F(F(F(b[3] - F(dy_)) * fy) + F(sy_))))
            hx, hy = int(F(sx_ + sw)), int(F(sy_ + sh))
            lx, ly = int(F(sx_)), int(F(sy_))
            X1, X2 = min(max(X1, lx), hx), min(max(X2, lx), hx)
            Y1, Y2 = min(max(Y1, ly), hy), min(max(Y2, ly), hy)
            sv = F(0.0) if s == 0 else s
            dets[i * D + r] = [i, X1, Y1, max(X2 - X1, 1), max(Y2 - Y1, 1), cls, int(np.asarray(sv, F).view(np.int32)), k]
        counts[i] = len(kept)
    return np.asarray(dets, np.int32), np.asarray(counts, np.int32)


def random_head(seed, n=2, K=90, C=5, box_format="xyxy", rect=(4, 6, 320, 200, 10, 20, 160, 100)):
    """seeded, with ties, NaN and +-inf scores, NaN and inverted boxes, boxes on and outside the placement; values on a
    coarse grid so that equal scores and touching boxes are common"""
    rng = np.random.default_rng(seed)
    dx, dy, dw, dh = rect[4:]
    scores = (rng.integers(0, 33, (n, K, C)) / 32).astype(F)              # many equal scores
    scores[rng.random((n, K, C)) < 0.03] = np.nan
    scores[rng.random((n, K, C)) < 0.01] = np.inf
    scores[rng.random((n, K, C)) < 0.02] = -np.inf
    scores[rng.random((n, K, C)) < 0.02] = -0.0
    cx = rng.integers(dx - 20, dx + dw + 20, (n, K)).astype(F)
    cy = rng.integers(dy - 20, dy + dh + 20, (n, K)).astype(F)
    w = rng.integers(0, 60, (n, K)).astype(F) * F(0.5)
    h = rng.integers(0, 60, (n, K)).astype(F) * F(0.5)
    for arr in (cx, cy, w, h):
        arr[:, 0:K - 1:7] = arr[:, 1:K:7]                                   # identical boxes
    if box_format == "cxcywh":
        boxes = np.stack([cx, cy, w, h], 2)
    else:
        boxes = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 2)
    boxes = boxes.astype(F)
    bad = rng.random((n, K)) < 0.05
    boxes[bad, rng.integers(0, 4, int(bad.sum()))] = np.nan
    inv = rng.random((n, K)) < 0.05
    if box_format == "xyxy":
        boxes[inv] = boxes[inv][:, [2, 3, 0, 1]]                            # inverted
    else:
        boxes[inv, 2] = -boxes[inv, 2]
    big = rng.random((n, K)) < 0.03
    boxes[big, 2] = np.inf
    boxes[0, 0] = (dx, dy, dx + dw, dy + dh) if box_format == "xyxy" else (dx + dw / 2, dy + dh / 2, dw, dh)   # the placement itself
    rects = np.asarray([rect] * n, np.int32)
    return boxes, scores, rects


@pytest.mark.parametrize("box_format", ["xyxy", "cxcywh"])
@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("iou_thr", [0.0, 0.45, 1.0])
def test_the_model_equals_the_scalar_implementation(box_format, agnostic, iou_thr):
    total = 0
    for seed, (T, D, thr) in enumerate([(1024, 100, 0.25), (16, 16, 0.5), (40, 7, -1.0)]):
        boxes, scores, rects = random_head(10 * seed + 1, box_format=box_format)
        with np.errstate(all="ignore"):
            want = naive_select(boxes, scores, rects, thr, iou_thr, agnostic, box_format, T, D)
        got = dm.select(boxes, scores, rects, thr, iou_thr, agnostic, box_format, T, D)
        assert np.array_equal(got[1], want[1]), (seed, got[1], want[1])
        assert np.array_equal(got[0], want[0]), (seed, np.flatnonzero((got[0] != want[0]).any(1))[:5])
        total += int(want[1].sum())
    assert total >= 12       # a condition on the inputs: something is detected


def test_the_random_heads_hold_what_they_promise():
    boxes, scores, rects = random_head(1)
    assert np.isnan(scores).any() and np.isposinf(scores).any() and np.isneginf(scores).any()
    assert np.isnan(boxes).any() and (boxes[..., 2] < boxes[..., 0]).any()
    s = np.where(np.isnan(scores), -np.inf, scores).max(2)
    assert len(np.unique(s[0])) < s.shape[1] // 2           # ties
    assert (boxes[..., 0] < rects[0, 4]).any() and (boxes[..., 2] > rects[0, 4] + rects[0, 6]).any()


def chain_head():
    """A (0.9) overlaps B (0.8) with IoU 0.6, B overlaps C (0.7) with IoU 0.6, A and C with 1 / 3: at 0.45 A suppresses
    B, B is gone and suppresses nothing, C is kept"""
    boxes = np.asarray([[[10, 10, 50, 50], [20, 10, 60, 50], [30, 10, 70, 50]]], F)
    scores = np.asarray([[[0.9], [0.8], [0.7]]], F)
    rects = np.asarray([[0, 0, 100, 100, 0, 0, 100, 100]], np.int32)
    return boxes, scores, rects


def test_a_suppressed_candidate_suppresses_nothing():
    boxes, scores, rects = chain_head()
    sup = dm.suppression(boxes[0], np.zeros(3, np.int64), 0.45, False)
    assert sup[0, 1] and sup[1, 2] and not sup[0, 2]
    dets, counts = dm.select(boxes, scores, rects, 0.25, 0.45, D=3)
    assert counts.tolist() == [2]
    assert dets[0].tolist() == [0, 10, 10, 40, 40, 0, int(F(0.9).view(np.int32)), 0]
    assert dets[1].tolist() == [0, 30, 10, 40, 40, 0, int(F(0.7).view(np.int32)), 2]
    assert dets[2].tolist() == [-1, 0, 0, 0, 0, 0, 0, 0]


def test_a_box_goes_back_through_the_letterbox():
    from vali_amd.tasks import letterbox_rect

    assert letterbox_rect(1920, 1080, 640, 640) == LETTERBOX[4:]
    # network (100.5, 200.25) .. (300, 400.5): x * 3, (y - 140) * 3: 301.5 .. 900, 180.75 .. 781.5 -> floor / ceil
    boxes = np.asarray([[[100.5, 200.25, 300.0, 400.5]]], F)
    dets, counts = dm.select(boxes, np.asarray([[[0.5, 0.75]]], F), np.asarray([LETTERBOX], np.int32))
    assert counts.tolist() == [1]
    assert dets[0].tolist() == [0, 301, 180, 900 - 301, 782 - 180, 1, int(F(0.75).view(np.int32)), 0]
    # a box that reaches into the bars is clipped to the picture: y from 140, to 500
    boxes = np.asarray([[[-50.0, 0.0, 700.0, 640.0]]], F)
    dets, _ = dm.select(boxes, np.asarray([[[0.5, 0.75]]], F), np.asarray([LETTERBOX], np.int32))
    assert dets[0, :5].tolist() == [0, 0, 0, 1920, 1080]
    # a crop record: src_x, src_y move the result
    rec = (100, 50, 960, 540, 0, 140, 640, 360)
    dets, _ = dm.select(np.asarray([[[64.0, 204.0, 128.0, 268.0]]], F), np.asarray([[[0.9]]], F), np.asarray([rec], np.int32))
    assert dets[0, :5].tolist() == [0, 100 + 96, 50 + 96, 96, 96]


def test_ties_nan_and_signed_zero():
    rects = np.asarray([[0, 0, 64, 64, 0, 0, 64, 64]], np.int32)
    boxes = np.asarray([[[i * 10, 0, i * 10 + 8, 8] for i in range(6)]], F)
    scores = np.asarray([[[0.0, np.nan], [np.nan, -0.0], [np.nan, np.nan], [0.5, 0.5], [0.0, -0.0], [np.inf, 1.0]]], F)
    dets, counts = dm.select(boxes, scores, rects, score_thr=-1.0, D=6, T=6)
    # inf first; 0.5 (lowest class wins the tie); the zeros, whatever their sign, by k; all-NaN never passes
    assert counts.tolist() == [5]
    assert dets[:5, 7].tolist() == [5, 3, 0, 1, 4]
    assert dets[:5, 5].tolist() == [0, 0, 0, 1, 0]
    assert dets[2:5, 6].tolist() == [0, 0, 0]               # -0.0 is reported as 0.0
    # exactly the first T under the order
    dets, counts = dm.select(boxes, scores, rects, score_thr=-1.0, D=3, T=3)
    assert dets[:3, 7].tolist() == [5, 3, 0]


def test_marks_are_what_the_example_builds():
    """examples/label_detections.py::marks_of, restated in numpy on fixed detections"""
    green = dm.pack_colour(40, 255, 80)
    dets = np.asarray([[0, 10, 40, 100, 80, 1, 0, 5], [0, 300, 5, 60, 60, 0, 0, 9], [-1, 0, 0, 0, 0, 0, 0, 0],
                       [1, 7, 9, 30, 20, 2, 0, 1], [1, 50, 60, 70, 80, 3, 0, 2], [-1, 0, 0, 0, 0, 0, 0, 0]], np.int32)
    rects = np.asarray([[0, 0, 40, 12], [0, 12, 52, 12], [0, 24, 33, 13]], np.int32)        # three labels: class 3 has none
    got = dm.marks_of(dets, [green], 2, rects, 200, dm.pack_colour(0, 0, 0))
    live = dets[[0, 1, 3]]                       # used, with a label
    r = rects[live[:, 5]]
    k = len(live)

    def rows(x, y, w, h, kind, arg, colour):
        cols = [live[:, 0], x, y, w, h] + [v if isinstance(v, np.ndarray) else np.full(k, v, np.int32) for v in (kind, arg, colour)]
        return np.stack(cols, 1)

    lx, ly = live[:, 1], live[:, 2] - r[:, 3]
    outline = rows(live[:, 1], live[:, 2], live[:, 3], live[:, 4], 1, 2, green)
    background = rows(lx, ly, r[:, 2], r[:, 3], 2, 0, dm.pack_colour(40, 255, 80, 200))
    text = rows(lx, ly, r[:, 2], r[:, 3], 4, r[:, 0] | r[:, 1] << 16, dm.pack_colour(0, 0, 0))
    assert np.array_equal(got[[0, 1, 3]], outline)
    assert np.array_equal(got[[6, 7, 9]], background)
    assert np.array_equal(got[[12, 13, 15]], text)
    assert got[4].tolist() == [1, 50, 60, 70, 80, 1, 2, green]           # class 3: an outline ...
    assert not got[[2, 5, 8, 10, 11, 14, 16, 17]].any()                     # ... no label; unused rows are MARK_NONE
    assert np.array_equal(dm.marks_of(dets, [green, 7], 3)[:, 7], [7, green, 0, green, 7, 0])
    rois = dm.rois_of(dets, (0, 0, 224, 224))
    assert rois[0].tolist() == [10, 40, 100, 80, 0, 0, 224, 224] and not rois[2].any()


# ---- ValueErrors of Prepare / Run ------------------------------------------------------------------------------------------
class FakeDevice:
    type, index = "cuda", 0


class FakeTensor:
    """what Prepare reads of a device tensor, without a device"""
    device = FakeDevice()

    def __init__(self, shape, typestr="<f4", strides=None, device_type="cuda", index=0):
        self.shape = tuple(shape)
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (4096, False), "version": 3,
                                         "strides": strides}
        self.device = FakeDevice()
        self.device.type, self.device.index = device_type, index


def i32(*shape, **kw):
    return FakeTensor(shape, "<i4", **kw)


def test_prepare_says_what_is_wrong():
    import vali_amd as vali

    ok_b, ok_s = FakeTensor((2, 100, 4)), FakeTensor((2, 100, 3))
    dets = i32(200, 8)

    def prepare(boxes=ok_b, scores=ok_s, dets=dets, **kw):
        return vali.SelectBatch(0, 0, boxes, scores, dets, **kw)

    for match, kw in [
        ("boxes: need a 3-D tensor", dict(boxes=FakeTensor((100, 4)))),
        ("boxes: the last dimension must be 4", dict(boxes=FakeTensor((2, 100, 5)))),
        ("scores: need a 3-D tensor", dict(scores=FakeTensor((2, 100, 3, 1)))),
        ("scores: the dtype must be float32 or float16", dict(scores=FakeTensor((2, 100, 3), "<f8"))),
        ("boxes: the dtype must be", dict(boxes=FakeTensor((2, 100, 4), "<i4"))),
        ("scores: negative strides", dict(scores=FakeTensor((2, 100, 3), strides=(1200, -12, 4)))),
        ("boxes: strides that are no multiple", dict(boxes=FakeTensor((2, 100, 4), strides=(1600, 16, 3)))),
        ("boxes and scores disagree", dict(scores=FakeTensor((2, 101, 3)))),
        ("boxes and scores disagree", dict(scores=FakeTensor((3, 100, 3)))),
        ("scores: the tensor is on device 1", dict(scores=FakeTensor((2, 100, 3), index=1))),
        ("boxes: the tensor must live on the GPU", dict(boxes=FakeTensor((2, 100, 4), device_type="cpu"))),
        ("scores: a device tensor with", dict(scores=[[[0.5]]])),
        ("N = 1025 is outside", dict(boxes=FakeTensor((1025, 1, 4)), scores=FakeTensor((1025, 1, 3)))),
        (r"K = 1048577 is outside", dict(boxes=FakeTensor((1, 2**20 + 1, 4)), scores=FakeTensor((1, 2**20 + 1, 3)))),
        ("C = 4097 is outside", dict(scores=FakeTensor((2, 100, 4097)))),
        ("C = 0 is outside", dict(scores=FakeTensor((2, 100, 0)))),
        ("box_format", dict(box_format="xywh")),
        ("max_candidates = 1025", dict(max_candidates=1025)),
        ("max_candidates = 0", dict(max_candidates=0)),
        ("max_det = 65 is outside", dict(max_candidates=64, max_det=65)),
        ("max_det = 0 is outside", dict(max_det=0)),
        ("exceeds 65535", dict(boxes=FakeTensor((1024, 1, 4)), scores=FakeTensor((1024, 1, 3)), max_det=64)),
        (r"dets: need an int32 tensor of shape \(200x8\)", dict(dets=i32(199, 8))),
        ("dets: need an int32 tensor", dict(dets=FakeTensor((200, 8), "<f4"))),
        ("dets: the tensor must be contiguous", dict(dets=i32(200, 8, strides=(64, 4)))),
        ("dets: the tensor is on device 1", dict(dets=i32(200, 8, index=1))),
        ("dets: an int32", dict(dets=None)),
        (r"counts: need an int32 tensor of shape \(2\)", dict(counts=i32(3))),
        (r"rois: need an int32 tensor of shape \(200x8\)", dict(rois=i32(200, 4))),
        ("marks: need", dict(marks=i32(400, 8))),
        ("marks: 6000 rows", dict(marks=i32(6000, 8), max_det=1000)),
        ("marks: the tensor must live on the GPU", dict(marks=i32(600, 8, device_type="cpu"))),
    ]:
        with pytest.raises(ValueError, match=match):
            prepare(**kw)


def test_layout_rules_accept_what_the_issue_lists():
    from vali_amd.detect import head_layout

    # a YOLOv8 head (N, 4 + C, K) as two transposed slices, a broadcast, dimensions of size 1
    assert head_layout("scores", (16, 8400, 80), (84 * 8400, 1, 8400), 2, 16) == (1, (16, 8400, 80), (84 * 8400, 1, 8400))
    assert head_layout("boxes", (16, 8400, 4), (84 * 8400, 1, 8400), 4, 16, 4)[0] == 2
    assert head_layout("scores", (2, 100, 3), (0, 0, 1), 2, 32)[2] == (0, 0, 1)
    assert head_layout("scores", (1, 1, 1), None, 2, 32)[2] == (1, 1, 1)
    with pytest.raises(ValueError, match="beyond 2\\^40"):
        head_layout("scores", (2, 100, 3), (2**41, 3, 1), 2, 32)


def test_run_says_what_is_wrong():
    from vali_amd.detect import DetectionStyle, _host_rects, run_spec

    plain, labelled = DetectionStyle(), DetectionStyle(label_rects=[(0, 0, 10, 5)])
    assert run_spec(0, False, 0.25, 0.45, None, None) == (0.25, 0.45, (0, 0, 0, 0))
    assert run_spec(1, True, 0.25, 0.45, (0, 0, 224, 224), plain)[2] == (0, 0, 224, 224)
    assert run_spec(3, False, 0.25, 0.45, None, labelled)
    for match, args in [
        ("score_thr must be finite", (0, False, float("nan"), 0.45, None, None)),
        ("score_thr must be finite", (0, False, float("-inf"), 0.45, None, None)),
        ("iou_thr must be finite", (0, False, 0.25, float("inf"), None, None)),
        ("crop_placement: four integers", (0, True, 0.25, 0.45, None, None)),
        ("crop_placement: four int32", (0, True, 0.25, 0.45, (0, 0, 224), None)),
        ("crop_placement: four int32", (0, True, 0.25, 0.45, (0, 0, 224, 2**31), None)),
        ("style: a DetectionStyle is required", (1, False, 0.25, 0.45, None, None)),
        ("style: marks of 3", (3, False, 0.25, 0.45, None, plain)),
        ("style: marks of 3", (1, False, 0.25, 0.45, None, labelled)),
    ]:
        with pytest.raises(ValueError, match=match):
            run_spec(*args)
    with pytest.raises(TypeError):
        run_spec(0, True, 0.25, 0.45, (0, 0, 2.5, 2), None)
    for match, rects in [("rects: need 2 rows", [(0,) * 8]), ("rects: need 2 rows", [(0,) * 8, (0,) * 7]),
                         ("rects: every value must fit", [(0,) * 8, (2**31,) * 8]), ("rects: a device tensor", 5)]:
        with pytest.raises(ValueError, match=match):
            _host_rects(rects, 2)
    for match, kw in [("thickness", dict(thickness=0)), ("label_alpha", dict(label_alpha=256)), ("at least one colour", dict(colours=[])),
                      ("every colour", dict(colours=[2**31])), ("label_rects must be", dict(label_rects=[(0, 0, 1)])),
                      ("text_colour", dict(text_colour=2**32))]:
        with pytest.raises(ValueError, match=match):
            DetectionStyle(**kw)


def test_the_names_are_exported():
    import python_vali
    import vali_amd

    for name in ("PyDetectionSelector", "SelectBatch", "DetectionStyle"):
        assert getattr(python_vali, name) is getattr(vali_amd, name)


# ---- VALI_ERR_INVALID_ARG of the C entry point, decided before any device is touched --------------------------------------
class Tensor(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("dtype", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("stride_n", ctypes.c_int64), ("stride_k", ctypes.c_int64), ("stride_c", ctypes.c_int64)]


class In(ctypes.Structure):
    _fields_ = [("boxes", Tensor), ("scores", Tensor), ("n", ctypes.c_int32), ("k", ctypes.c_int32), ("c", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class Params(ctypes.Structure):
    _fields_ = [("max_candidates", ctypes.c_int32), ("max_det", ctypes.c_int32), ("score_thr", ctypes.c_float),
                ("iou_thr", ctypes.c_float), ("class_agnostic", ctypes.c_int32), ("box_format", ctypes.c_int32),
                ("crop", ctypes.c_int32 * 4), ("thickness", ctypes.c_int32), ("label_alpha", ctypes.c_int32),
                ("text_colour", ctypes.c_int32), ("n_colours", ctypes.c_int32), ("n_labels", ctypes.c_int32)]


class Out(ctypes.Structure):
    _fields_ = [("dets", ctypes.c_void_p), ("counts", ctypes.c_void_p), ("rois", ctypes.c_void_p), ("marks", ctypes.c_void_p),
                ("colours", ctypes.c_void_p), ("label_rects", ctypes.c_void_p)]


def test_struct_sizes_match_the_header():
    assert (ctypes.sizeof(Tensor), ctypes.sizeof(In), ctypes.sizeof(Params), ctypes.sizeof(Out)) == (40, 96, 60, 48)


def test_the_c_entry_point_refuses_before_any_device_is_touched():
    lib = ctypes.CDLL(str(ROOT / "vali_amd" / "libvali_hip.so"))
    lib.vali_last_error.restype = ctypes.c_char_p
    lib.vali_detect_workspace_size.restype = ctypes.c_size_t
    lib.vali_detect_select.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_void_p]
    size = lib.vali_detect_workspace_size(2, 100, 64)
    assert size >= 2 * 100 * 6 + 2 * 64 * 32 + 2 * 64 * 8
    for bad in [(0, 100, 64), (1025, 100, 64), (2, 0, 64), (2, 2**20 + 1, 64), (2, 100, 0), (2, 100, 1025)]:
        assert lib.vali_detect_workspace_size(*bad) == 0, bad
    assert lib.vali_detect_workspace_size(1024, 2**20, 1024) > 2**32

    def call(edit=None, null=None, ws_bytes=size, ws=0x10000):
        t = lambda last: Tensor(0x1000, 0, 0, 100 * last, last, 1)         # noqa: E731  (never dereferenced)
        i = In(t(4), t(3), 2, 100, 3, 0)
        p = Params(64, 10, 0.25, 0.45, 0, 0, (ctypes.c_int32 * 4)(), 2, 200, 0, 1, 0)
        o = Out(0x2000, 0, 0, 0, 0, 0)
        if edit:
            edit(i, p, o)
        args = [ctypes.addressof(i), ctypes.addressof(p), 0x3000, ctypes.addressof(o), ws]
        if null is not None:
            args[null] = None
        rc = lib.vali_detect_select(*args, ws_bytes, None)
        return rc, lib.vali_last_error().decode()

    def setter(path, value):
        def edit(i, p, o):
            obj = {"i": i, "p": p, "o": o}[path[0]]
            for name in path[1:-1]:
                obj = getattr(obj, name)
            setattr(obj, path[-1], value)
        return edit

    for k in range(5):
        assert call(null=k) == (-1, "vali_detect_select: null argument"), k
    cases = [
        (("i", "n"), 0, "n outside"), (("i", "n"), 1025, "n outside"), (("i", "k"), 0, "k outside"),
        (("i", "k"), 2**20 + 1, "k outside"), (("i", "c"), 0, "c outside"), (("i", "c"), 4097, "c outside"),
        (("i", "boxes", "data"), None, "boxes has a null pointer"), (("i", "scores", "data"), None, "scores has a null pointer"),
        (("i", "scores", "dtype"), 3, "dtype 3"), (("i", "boxes", "dtype"), -1, "dtype -1"),
        (("i", "scores", "data"), 0x1002, "not aligned to its element"), (("i", "scores", "stride_k"), -1, "strides"),
        (("i", "boxes", "stride_n"), 2**41, "strides"),
        (("p", "max_candidates"), 0, "max_candidates outside"), (("p", "max_candidates"), 1025, "max_candidates outside"),
        (("p", "max_det"), 0, "max_det outside"), (("p", "max_det"), 65, "max_det outside"),
        (("p", "score_thr"), float("nan"), "score_thr is not finite"), (("p", "score_thr"), float("inf"), "score_thr is not finite"),
        (("p", "iou_thr"), float("-inf"), "iou_thr is not finite"), (("p", "iou_thr"), float("nan"), "iou_thr is not finite"),
        (("p", "box_format"), 2, "box_format"),
        (("o", "dets"), 0x2002, "not 4-byte aligned"),
    ]
    for path, value, text in cases:
        rc, err = call(setter(path, value))
        assert rc == -1 and text in err, (path, value, rc, err)
    rc, err = call(ws_bytes=size - 1)
    assert rc == -1 and "workspace is smaller" in err
    rc, err = call(ws=0x10008)
    assert rc == -1 and "not 16-byte aligned" in err

    def many(i, p, o):
        i.n, p.max_det, p.max_candidates = 1024, 64, 64
    rc, err = call(many, ws_bytes=2**40)
    assert rc == -1 and "exceeds 65535" in err

    def marks(**kw):
        def edit(i, p, o):
            o.marks, o.colours = 0x4000, 0x5000
            for name, v in kw.items():
                setattr(o if name in ("colours", "label_rects") else p, name, v)
        return edit
    for kw, text in [(dict(colours=None), "marks without colours"), (dict(n_colours=0), "marks without colours"),
                     (dict(thickness=0), "thickness below 1"), (dict(label_alpha=256), "label_alpha outside"),
                     (dict(label_rects=0x6000, n_labels=0), "label_rects without n_labels"),
                     (dict(max_candidates=1024, max_det=1000, label_rects=0x6000, n_labels=1), "more than 4096 mark rows")]:
        rc, err = call(marks(**kw), ws_bytes=2**40)
        assert rc == -1 and text in err, (kw, rc, err)
