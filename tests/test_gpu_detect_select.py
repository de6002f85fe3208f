"""PyDetectionSelector on the GPU against tests/detect_model.py, bit for bit: every output row of every call, on outputs
that were filled with garbage first.

Shapes are the smallest at which the kernels can still go wrong: K around the 64-lane and 512-candidate blocks of the
score kernels and the 1024-thread stride of the select kernel, C around the 16-byte loads (80 float16 classes are ten of
them, 81 leave a tail and break the rows' alignment), one frame and three."""
import numpy as np
import pytest

import detect_model as dm
from test_detect_host import chain_head, random_head

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

F = np.float32
GARBAGE = 0x5A5A5A5A
DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
RECT = (4, 6, 320, 200, 10, 20, 160, 100)


@pytest.fixture(scope="module")
def sel(vali, gpu):
    return vali.PyDetectionSelector(gpu)


def lay_out(boxes, scores, layout, dtype, gpu):
    """numpy (N, K, 4) and (N, K, C) -> two device views in `layout`, and whatever they are views of"""
    dev = f"cuda:{gpu}"
    b, s = torch.from_numpy(boxes).to(dev).to(dtype), torch.from_numpy(scores).to(dev).to(dtype)
    n, k, c = scores.shape
    if layout == "c":                       # (N, K, C) as it is
        return b.contiguous(), s.contiguous(), None
    if layout == "k":                       # a YOLOv8 head (N, 4 + C, K), as two transposed slices
        pred = torch.cat([b, s], 2).transpose(1, 2).contiguous()
        return pred[:, :4].transpose(1, 2), pred[:, 4:].transpose(1, 2), pred
    if layout == "mis":                     # a misaligned base: the slice [..., 1:] of a wider tensor
        wide_s = torch.full((n, k, c + 1), 9.0, dtype=dtype, device=dev)
        wide_s[..., 1:] = s
        wide_b = torch.full((n, k, 5), 9.0, dtype=dtype, device=dev)
        wide_b[..., 1:] = b
        return wide_b[..., 1:], wide_s[..., 1:], (wide_b, wide_s)
    if layout == "mis_k":                   # the same for a transposed head: candidates from 1
        pred = torch.full((n, 4 + c, k + 1), 9.0, dtype=dtype, device=dev)
        pred[:, :, 1:] = torch.cat([b, s], 2).transpose(1, 2)
        return pred[:, :4, 1:].transpose(1, 2), pred[:, 4:, 1:].transpose(1, 2), pred
    if layout == "bcast_k":                 # one row of scores for every candidate: stride 0
        return b.contiguous(), s[:, :1, :].contiguous().expand(n, k, c), None
    if layout == "bcast_c":                 # one score for every class
        return b.contiguous(), s[:, :, :1].contiguous().expand(n, k, c), None
    raise AssertionError(layout)


def outputs(n, D, gpu, rois=False, R=0):
    dev = f"cuda:{gpu}"
    full = lambda *shape: torch.full(shape, GARBAGE, dtype=torch.int32, device=dev)      # noqa: E731
    return full(n * D, 8), full(n), full(n * D, 8) if rois else None, full(R * n * D, 8) if R else None


def check(vali, gpu, sel, b, s, rects, T=1024, D=100, thr=0.25, iou=0.45, agnostic=False, fmt="xyxy", device_rects=False,
          crop=None, style=None, colours=None, label_rects=None):
    """one Run on garbage-filled outputs against the model; returns (dets, counts) of the model"""
    n = s.shape[0]
    R = 0 if style is None else (3 if label_rects is not None else 1)
    dets, counts, rois, marks = outputs(n, D, gpu, crop is not None, R)
    rects = np.asarray(rects, np.int32).reshape(n, 8)
    rects_arg = torch.from_numpy(rects).to(f"cuda:{gpu}") if device_rects else [tuple(int(v) for v in r) for r in rects]
    torch.cuda.synchronize()
    sb = sel.Prepare(b, s, dets, counts, rois, marks, box_format=fmt, max_candidates=T, max_det=D)
    ok, info = sel.Run(sb, rects_arg, thr, iou, agnostic, crop_placement=crop, style=style)
    assert ok and info == vali.TaskExecInfo.SUCCESS, info
    want_d, want_c = dm.select(b.float().cpu().numpy(), s.float().cpu().numpy(), rects, thr, iou, agnostic, fmt, T, D)
    got_d, got_c = dets.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(got_c, want_c), (got_c, want_c)
    if not np.array_equal(got_d, want_d):
        bad = np.flatnonzero((got_d != want_d).any(1))
        raise AssertionError(f"{bad.size} rows differ, first {bad[:4]}: got {got_d[bad[:4]]}, want {want_d[bad[:4]]}")
    if rois is not None:
        assert np.array_equal(rois.cpu().numpy(), dm.rois_of(want_d, crop))
    if marks is not None:
        want_m = dm.marks_of(want_d, colours, style.thickness, label_rects, style.label_alpha, style.text_colour)
        assert np.array_equal(marks.cpu().numpy(), want_m)
    return want_d, want_c


def head(seed, n, K, C, fmt="xyxy"):
    boxes, scores, _ = random_head(seed, n, K, C, fmt, RECT)
    return boxes, scores, [RECT] * n


# ---- shapes, layouts, dtypes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["k", "c"])
@pytest.mark.parametrize("C", [1, 3, 80, 81])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 257, 1000])
def test_shapes(vali, gpu, sel, K, C, layout):
    n = 3 if (K + C) % 2 else 1
    dtype = list(DTYPES)[(K + C + len(layout)) % 3]
    boxes, scores, rects = head(K * 100 + C, n, K, C)
    b, s, _keep = lay_out(boxes, scores, layout, DTYPES[dtype], gpu)
    _, counts = check(vali, gpu, sel, b, s, rects, D=20, thr=0.5)
    if K >= 63:
        assert counts.sum() >= 5           # a condition on the inputs


@pytest.mark.parametrize("layout", ["k", "c", "mis", "mis_k", "bcast_k", "bcast_c"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("K,C", [(257, 80), (65, 3), (1000, 81), (1024, 16)])
def test_layouts_and_dtypes(vali, gpu, sel, K, C, dtype, layout):
    boxes, scores, rects = head(K + C, 3, K, C, "cxcywh")
    b, s, _keep = lay_out(boxes, scores, layout, DTYPES[dtype], gpu)
    if layout == "k":
        assert s.stride(1) == 1 and b.stride(1) == 1
    if layout.startswith("mis"):
        assert s.data_ptr() % 16 != 0
    if layout.startswith("bcast"):
        assert 0 in s.stride()
    check(vali, gpu, sel, b, s, rects, D=30, thr=0.6, fmt="cxcywh", agnostic=layout == "bcast_c")


# ---- order and limits -----------------------------------------------------------------------------------------------------------
def spread_boxes(n, K, step=3.0, size=2.0):
    """K boxes that do not touch, on a grid inside RECT's placement"""
    dx, dy, dw, _ = RECT[4:]
    per_row = int(dw // step)
    k = np.arange(K)
    x, y = dx + (k % per_row) * step, dy + (k // per_row) * step
    assert y.max() + size <= dy + RECT[7]
    return np.broadcast_to(np.stack([x, y, x + size, y + size], 1).astype(F), (n, K, 4)).copy()


@pytest.mark.parametrize("layout", ["k", "c"])
def test_more_than_T_candidates_with_equal_scores_across_the_cut(vali, gpu, sel, layout):
    n, K, C, T = 2, 1000, 3, 64
    rng = np.random.default_rng(5)
    scores = (rng.random((n, K, C)) * 0.2).astype(F)                     # below the threshold
    for i in range(n):
        order = rng.permutation(K)
        scores[i, order[:40], rng.integers(0, C, 40)] = (0.6 + 0.3 * rng.random(40)).astype(F)       # 40 above the block
        scores[i, order[40:140], rng.integers(0, C, 100)] = 0.5          # 100 equal scores: 24 of them go on, by k
        scores[i, order[140:300], rng.integers(0, C, 160)] = (0.3 + 0.19 * rng.random(160)).astype(F)
    boxes = spread_boxes(n, K)
    b, s, _keep = lay_out(boxes, scores, layout, torch.float32, gpu)
    dets, counts = check(vali, gpu, sel, b, s, [RECT] * n, T=T, D=T, thr=0.25)
    assert counts.tolist() == [T, T]
    for i in range(n):
        bits = dets[i * T:(i + 1) * T, 6].view(F)
        assert (bits[:40] > 0.5).all() and (bits[40:] == 0.5).all()
        ks = dets[i * T + 40:(i + 1) * T, 7]
        equal = np.flatnonzero(scores[i].max(1) == F(0.5))
        assert np.array_equal(ks, equal[:24])                           # the first of the block by k, exactly


def test_more_than_D_kept_every_candidate_passing_and_none(vali, gpu, sel):
    n, K, C = 3, 257, 3
    boxes, scores, rects = head(9, n, K, C)
    scores = np.nan_to_num(scores, nan=0.5, posinf=1.0, neginf=0.0)
    boxes = spread_boxes(n, K)
    b, s, _keep = lay_out(boxes, scores, "c", torch.float32, gpu)
    _, counts = check(vali, gpu, sel, b, s, rects, D=5, thr=0.1)
    assert counts.tolist() == [5, 5, 5]
    _, counts = check(vali, gpu, sel, b, s, rects, T=1024, D=300, thr=-1.0)      # every candidate passes and is kept
    assert counts.tolist() == [K, K, K]
    _, counts = check(vali, gpu, sel, b, s, rects, thr=2.0)                         # none passes
    assert counts.tolist() == [0, 0, 0]


@pytest.mark.parametrize("device_rects", [False, True])
def test_the_suppression_chain(vali, gpu, sel, device_rects):
    boxes, scores, rects = chain_head()
    b, s, _keep = lay_out(boxes, scores, "c", torch.float32, gpu)
    dets, counts = check(vali, gpu, sel, b, s, rects, D=3, device_rects=device_rects)
    assert counts.tolist() == [2] and dets[:2, 7].tolist() == [0, 2]


@pytest.mark.parametrize("agnostic", [False, True])
def test_identical_boxes_of_two_classes(vali, gpu, sel, agnostic):
    boxes = np.asarray([[[20, 30, 60, 70], [20, 30, 60, 70], [100, 40, 120, 60]]], F)
    scores = np.asarray([[[0.9, 0.1], [0.2, 0.8], [0.3, 0.7]]], F)
    b, s, _keep = lay_out(boxes, scores, "c", torch.float16, gpu)
    dets, counts = check(vali, gpu, sel, b, s, [RECT], D=3, agnostic=agnostic)
    assert counts.tolist() == [2 if agnostic else 3]
    assert dets[:counts[0], 7].tolist() == ([0, 2] if agnostic else [0, 1, 2])


@pytest.mark.parametrize("layout", ["k", "c"])
def test_1024_candidates_at_T_1024(vali, gpu, sel, layout):
    n, K, C = 2, 1024, 4
    rng = np.random.default_rng(8)
    scores = (0.3 + 0.6 * rng.random((n, K, C))).astype(F)
    dx, dy, dw, dh = RECT[4:]
    x, y = dx + rng.random((n, K)) * (dw - 12), dy + rng.random((n, K)) * (dh - 12)
    w, h = 4 + rng.random((n, K)) * 8, 4 + rng.random((n, K)) * 8
    boxes = np.stack([x, y, x + w, y + h], 2).astype(F)
    b, s, _keep = lay_out(boxes, scores, layout, torch.float32, gpu)
    dets, counts = check(vali, gpu, sel, b, s, [RECT] * n, T=1024, D=1024 // 16, iou=0.3)
    assert (counts == 64).all()
    dets, counts = check(vali, gpu, sel, b, s, [RECT] * n, T=1024, D=1024, iou=0.1, agnostic=True)
    assert (counts > 64).all() and (counts < 1024).all()        # the walk goes through all sixteen blocks of candidates


def test_nan_and_inf_scores_and_boxes(vali, gpu, sel):
    boxes, scores, rects = head(21, 3, 257, 5)
    assert np.isnan(scores).any() and np.isinf(scores).any() and np.isnan(boxes).any() and np.isinf(boxes).any()
    for layout in ("k", "c"):
        b, s, _keep = lay_out(boxes, scores, layout, torch.float32, gpu)
        dets, counts = check(vali, gpu, sel, b, s, rects, thr=-1.0, D=40)
        assert (dets[:, 6].view(F) == np.inf).any()


# ---- records ----------------------------------------------------------------------------------------------------------------------
def test_device_rects_that_empty_one_frame_of_three(vali, gpu, sel):
    boxes, scores, _ = head(31, 3, 257, 3)
    rects = [RECT, (4, 6, 320, 200, 10, 20, 0, 100), RECT]
    b, s, _keep = lay_out(boxes, scores, "k", torch.float16, gpu)
    _, counts = check(vali, gpu, sel, b, s, rects, D=10, device_rects=True)
    assert counts[1] == 0 and counts[0] > 0 and counts[2] > 0
    rects = [(0, 0, -5, 200, 10, 20, 160, 100), RECT, (0, 0, 320, 200, 10, 20, 160, -2**31)]
    _, counts = check(vali, gpu, sel, b, s, rects, D=10, device_rects=True)
    assert counts[0] == 0 and counts[1] > 0 and counts[2] == 0


def test_a_crop_source_record_and_a_letterbox(vali, gpu, sel):
    boxes, scores, _ = head(41, 2, 257, 3)
    rects = [(100, 50, 960, 540, 10, 20, 160, 100), (0, 0, 77, 33, 10, 20, 160, 100)]     # growing and shrinking, odd ratios
    b, s, _keep = lay_out(boxes, scores, "c", torch.bfloat16, gpu)
    dets, counts = check(vali, gpu, sel, b, s, rects, D=50)
    used = dets[:counts[0]]
    assert (used[:, 1] >= 100).all() and (used[:, 1] + used[:, 3] <= 1060).all() and (used[:, 2] >= 50).all()


# ---- rois and marks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", [False, True])
def test_rois_and_marks(vali, gpu, sel, labels):
    n, K, C, D = 3, 257, 5, 12
    boxes, scores, rects = head(51, n, K, C)
    rects = [RECT, (0, 0, 320, 200, 10, 20, 160, 0), RECT]             # frame 1 has no detections: unused rows
    b, s, _keep = lay_out(boxes, scores, "k", torch.float32, gpu)
    colours = [vali.pack_colour(40, 255, 80), vali.pack_colour(255, 0, 0, 128), vali.pack_colour(1, 2, 3, 0)]
    label_rects = np.asarray([[0, 0, 40, 12], [0, 12, 52, 12], [3, 24, 33, 13]], np.int32) if labels else None    # classes 3, 4: none
    style = vali.DetectionStyle(thickness=3, colours=colours, label_rects=label_rects, label_alpha=77,
                                text_colour=vali.pack_colour(250, 250, 250))
    dets, counts = check(vali, gpu, sel, b, s, rects, D=D, thr=0.5, crop=(0, 0, 224, 224), style=style, colours=colours,
                         label_rects=label_rects)
    classes = dets[dets[:, 0] >= 0, 5]
    assert (classes >= 3).any() and (classes < 3).any() and (counts < D).any()
    # the style's arrays as device tensors give the same rows
    dev = f"cuda:{gpu}"
    style_d = vali.DetectionStyle(thickness=3, colours=torch.tensor(colours, dtype=torch.int32, device=dev),
                                  label_rects=None if label_rects is None else torch.from_numpy(label_rects).to(dev),
                                  label_alpha=77, text_colour=vali.pack_colour(250, 250, 250))
    check(vali, gpu, sel, b, s, rects, D=D, thr=0.5, style=style_d, colours=colours, label_rects=label_rects)


def test_run_refuses_what_prepare_could_not_see(vali, gpu, sel):
    boxes, scores, rects = head(61, 2, 65, 3)
    b, s, _keep = lay_out(boxes, scores, "c", torch.float32, gpu)
    dets, counts, rois, marks = outputs(2, 10, gpu, True, 1)
    sb = sel.Prepare(b, s, dets, counts, rois, marks, max_det=10)
    style = vali.DetectionStyle()
    with pytest.raises(ValueError, match="crop_placement"):
        sel.Run(sb, rects, style=style)
    with pytest.raises(ValueError, match="style"):
        sel.Run(sb, rects, crop_placement=(0, 0, 8, 8))
    with pytest.raises(ValueError, match="rects: need an int32 tensor of shape"):
        sel.Run(sb, torch.zeros((3, 8), dtype=torch.int32, device=f"cuda:{gpu}"), crop_placement=(0, 0, 8, 8), style=style)
    with pytest.raises(ValueError, match="score_thr"):
        sel.Run(sb, rects, score_thr=float("nan"), crop_placement=(0, 0, 8, 8), style=style)
    with pytest.raises(ValueError, match="dets: the tensor must be contiguous"):
        sel.Prepare(b, s, torch.zeros((20, 16), dtype=torch.int32, device=f"cuda:{gpu}")[:, :8], max_det=10)
    assert sel.Run(sb, rects, crop_placement=(0, 0, 8, 8), style=style)[0]


# ---- capture ----------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay_after_the_inputs_were_rewritten(vali, gpu):
    from vali_amd._native import shim

    n, K, C, D = 3, 257, 80, 25
    stream = shim.stream_create(gpu)
    task = vali.PyDetectionSelector(gpu, stream)
    sets = [head(70 + j, n, K, C) for j in range(2)]
    recs = [[RECT] * n, [(100, 50, 960, 540, 10, 20, 160, 100), (0, 0, 0, 0, 0, 0, 0, 0), RECT]]
    b, s, pred = lay_out(sets[0][0], sets[0][1], "k", torch.float16, gpu)
    dev = f"cuda:{gpu}"
    rects = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    colours = torch.tensor([vali.pack_colour(0, 255, 0)], dtype=torch.int32, device=dev)
    style = vali.DetectionStyle(colours=colours)
    dets, counts, rois, marks = outputs(n, D, gpu, True, 1)
    torch.cuda.synchronize()
    sb = task.Prepare(b, s, dets, counts, rois, marks, max_det=D)
    cap = vali.StreamCapture(stream, gpu)
    with cap:
        assert task.RunAsync(sb, rects, 0.5, 0.4, crop_placement=(2, 4, 64, 64), style=style)[0]
    cap.Keep(sb)
    for j in (0, 1, 0):
        b2, s2, _keep = lay_out(sets[j][0], sets[j][1], "c", torch.float16, gpu)
        b.copy_(b2), s.copy_(s2)                                      # rewritten in place, through the views
        rects.copy_(torch.tensor(recs[j % 2], dtype=torch.int32))
        for t in (dets, counts, rois, marks):
            t.fill_(GARBAGE)
        torch.cuda.synchronize()
        cap.Launch()
        shim.stream_sync(gpu, stream)
        want_d, want_c = dm.select(b.float().cpu().numpy(), s.float().cpu().numpy(), np.asarray(recs[j % 2], np.int32), 0.5, 0.4,
                                   False, "xyxy", 1024, D)
        assert np.array_equal(counts.cpu().numpy(), want_c) and np.array_equal(dets.cpu().numpy(), want_d), j
        assert np.array_equal(rois.cpu().numpy(), dm.rois_of(want_d, (2, 4, 64, 64)))
        assert np.array_equal(marks.cpu().numpy(), dm.marks_of(want_d, [vali.pack_colour(0, 255, 0)]))
        assert want_c.sum() > 0
    assert pred is not None
