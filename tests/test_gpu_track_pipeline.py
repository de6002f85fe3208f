"""The tracker between its neighbours: PyDetectionSelector's `dets` go straight into PyDetectionTracker, its `marks`
straight into PySurfaceAnnotator.RunBatch (with a coverage atlas for the labels), on three consecutive NV12 frames of a
synthetic head in which one object moves and changes its class on the way.  No host step in between.  The box keeps
one id and so one colour, where the selector's own marks would change theirs with the class, and the frames equal those
of the model's marks (tests/detect_model.py, tests/track_model.py) drawn by the same annotator."""
import numpy as np
import pytest

import detect_model as dm
import track_model as tm
from test_gpu_annotate import download, make_frames

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

W, H = 64, 48
N, K, C, D, T = 3, 33, 3, 4, 8
RECT = (0, 0, W, H, 0, 0, W, H)               # the network saw the frames as they are


def moving_head():
    """one object of 20 x 16 that moves 5 px a frame and is of class 0, 1, 2 in the three frames, a second one that stays
    and is of class 1; everything else scores below the threshold"""
    rng = np.random.default_rng(8)
    boxes = np.zeros((N, K, 4), np.float32)
    scores = (rng.random((N, K, C)) * 0.2).astype(np.float32)
    x = rng.random((N, K)) * 30
    boxes[..., 0], boxes[..., 1], boxes[..., 2], boxes[..., 3] = x, 2, x + 9, 11
    for i in range(N):
        boxes[i, 7] = 6 + 5 * i, 20, 26 + 5 * i, 36
        scores[i, 7, i] = 0.9
        boxes[i, 20] = 40, 4, 58, 18
        scores[i, 20, 1] = 0.8
    return boxes, scores


def test_the_selectors_rows_are_tracked_and_drawn_in_one_colour_per_object(vali, gpu):
    dev = f"cuda:{gpu}"
    boxes, scores = moving_head()
    b, s = torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev)
    atlas_host = np.random.default_rng(2).integers(0, 256, (30, 20), dtype=np.uint8)
    atlas_t = torch.from_numpy(atlas_host).to(dev)
    label_rects = np.asarray([[0, 0, 20, 9], [0, 9, 14, 8], [3, 17, 17, 13]], np.int32)
    colours = [vali.pack_colour(40, 255, 80), vali.pack_colour(250, 20, 20), vali.pack_colour(20, 20, 250),
               vali.pack_colour(240, 240, 0)]
    style = vali.DetectionStyle(thickness=2, colours=colours, label_rects=label_rects, label_alpha=180)
    dets = torch.zeros((N * D, 8), dtype=torch.int32, device=dev)
    tracked, marks = torch.zeros_like(dets), torch.zeros((3 * N * D, 8), dtype=torch.int32, device=dev)
    assoc = torch.zeros((N * D, 4), dtype=torch.int32, device=dev)
    tracks = torch.zeros((T, 16), dtype=torch.int32, device=dev)
    clock = torch.zeros((1, 4), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    atlas = vali.Surface.from_dlpack(atlas_t, vali.Y)

    sel = vali.PyDetectionSelector(gpu)
    sb = sel.Prepare(b, s, dets, max_candidates=32, max_det=D)
    assert sel.Run(sb, [RECT] * N, 0.5, 0.45) == (True, vali.TaskExecInfo.SUCCESS)
    tk = vali.PyDetectionTracker(gpu)
    tb = tk.Prepare(dets, tracks, clock, tracked, assoc, marks, streams=1, max_det=D, max_tracks=T)
    run = dict(iou_thr=0.3, new_thr=0.5, min_hits=1, max_age=5, momentum=0.5, class_agnostic=True)
    assert tk.Run(tb, style=style, **run) == (True, vali.TaskExecInfo.SUCCESS)

    want_d, want_c = dm.select(boxes, scores, np.asarray([RECT] * N, np.int32), 0.5, 0.45, False, "xyxy", 32, D)
    assert want_c.tolist() == [2, 2, 2] and np.array_equal(dets.cpu().numpy(), want_d)
    _, _, want_t, want_a = tm.update(want_d, np.zeros((T, 16), np.int32), np.zeros((1, 4), np.int32), 1, D, T, **run)
    want_m = tm.marks_of(want_t, colours, 2, label_rects, 180)
    got_t, got_m = tracked.cpu().numpy(), marks.cpu().numpy()
    assert np.array_equal(got_t, want_t) and np.array_equal(assoc.cpu().numpy(), want_a) and np.array_equal(got_m, want_m)

    # the moving box is row 0 of every frame (the higher score): three classes in dets, one id and one colour here
    mover = [i * D for i in range(N)]
    assert want_d[mover, 5].tolist() == [0, 1, 2] and want_d[mover, 1].tolist() == [6, 11, 16]
    assert got_t[mover, 5].tolist() == [1, 1, 1] and got_t[[i * D + 1 for i in range(N)], 5].tolist() == [2, 2, 2]
    assert got_m[mover, 7].tolist() == [colours[1]] * 3
    by_class = dm.marks_of(want_d, colours, 2, label_rects, 180)
    assert len(set(by_class[mover, 7].tolist())) == 3

    # marks -> annotator
    ann = vali.PySurfaceAnnotator(gpu)
    a, hosts = make_frames(vali, gpu, "NV12", [(W, H)] * N, seed=3)
    m, _ = make_frames(vali, gpu, "NV12", [(W, H)] * N, seed=3)
    model_marks = torch.from_numpy(want_m).to(dev)
    torch.cuda.synchronize()
    assert ann.RunBatch(ann.PrepareBatch(a), marks, atlas=atlas)[0]
    assert ann.RunBatch(ann.PrepareBatch(m), model_marks, atlas=atlas)[0]
    for i in range(N):
        got = download(vali, gpu, a[i])
        assert np.array_equal(got, download(vali, gpu, m[i])), i
        assert not np.array_equal(got, hosts[i]), i                  # drawn on
