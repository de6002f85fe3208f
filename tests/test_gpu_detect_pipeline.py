"""The selector's rows in the hands of their consumers: `marks` goes straight into PySurfaceAnnotator.RunBatch (with a
coverage atlas for the labels) and `rois` into PySurfacePreprocessor.RunRoiBatch, on three small NV12 frames, with no
host step in between.  The frames and crops equal those of the model's rows (tests/detect_model.py) fed through the same
calls, and something was drawn and cropped."""
import numpy as np
import pytest

import detect_model as dm
from test_detect_host import random_head
from test_gpu_annotate import download, make_frames
from test_gpu_preproc_roi import MEAN, STD, canvas

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

W, H = 64, 48
N, K, C, D = 3, 65, 4, 4
RECT = (0, 0, W, H, 2, 4, 32, 24)             # the frames went into a 36 x 32 network input at (2, 4), halved
CROP = (0, 0, 16, 16)


def test_marks_and_rois_feed_the_annotator_and_the_preprocessor(vali, gpu):
    dev = f"cuda:{gpu}"
    boxes, scores, _ = random_head(5, N, K, C, "xyxy", RECT)
    rects = [RECT, RECT, (0, 0, W, H, 2, 4, 0, 24)]                 # the last frame has no detections
    b, s = torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev)
    atlas_host = np.random.default_rng(2).integers(0, 256, (30, 20), dtype=np.uint8)
    atlas_t = torch.from_numpy(atlas_host).to(dev)
    label_rects = np.asarray([[0, 0, 20, 9], [0, 9, 14, 8], [3, 17, 17, 13]], np.int32)        # class 3 has no label
    colours = [vali.pack_colour(40, 255, 80), vali.pack_colour(250, 20, 20)]
    style = vali.DetectionStyle(thickness=2, colours=colours, label_rects=label_rects, label_alpha=180)
    dets = torch.zeros((N * D, 8), dtype=torch.int32, device=dev)
    counts = torch.zeros((N,), dtype=torch.int32, device=dev)
    rois, marks = torch.zeros_like(dets), torch.zeros((3 * N * D, 8), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    atlas = vali.Surface.from_dlpack(atlas_t, vali.Y)

    sel = vali.PyDetectionSelector(gpu)
    sb = sel.Prepare(b, s, dets, counts, rois, marks, max_candidates=64, max_det=D)
    assert sel.Run(sb, rects, 0.5, 0.3, crop_placement=CROP, style=style) == (True, vali.TaskExecInfo.SUCCESS)

    want_d, want_c = dm.select(boxes, scores, np.asarray(rects, np.int32), 0.5, 0.3, False, "xyxy", 64, D)
    want_m = dm.marks_of(want_d, colours, 2, label_rects, 180)
    want_r = dm.rois_of(want_d, CROP)
    assert want_c.tolist()[2] == 0 and want_c[0] >= 2 and want_c[1] >= 2
    model_marks = torch.from_numpy(want_m).to(dev)
    model_rois = torch.from_numpy(want_r).to(dev)
    torch.cuda.synchronize()

    # marks -> annotator
    ann = vali.PySurfaceAnnotator(gpu)
    a, hosts = make_frames(vali, gpu, "NV12", [(W, H)] * N, seed=3)
    m, _ = make_frames(vali, gpu, "NV12", [(W, H)] * N, seed=3)
    assert ann.RunBatch(ann.PrepareBatch(a), marks, atlas=atlas)[0]
    assert ann.RunBatch(ann.PrepareBatch(m), model_marks, atlas=atlas)[0]
    for i in range(N):
        got = download(vali, gpu, a[i])
        assert np.array_equal(got, download(vali, gpu, m[i])), i
        assert np.array_equal(got, hosts[i]) == (i == 2), i          # drawn on, except the frame without detections

    # rois -> second-stage crops, item i * D + r from frame i
    pp = vali.PySurfacePreprocessor(gpu, mean=MEAN, std=STD, div=255.0)
    srcs = [a[i] for i in range(N) for _ in range(D)]
    crops = []
    for tensor in (rois, model_rois):
        dsts = [canvas(vali, gpu, "RGB_32F_PLANAR", 16, 16) for _ in srcs]
        batch = pp.PrepareRoiBatch(srcs, dsts)
        assert pp.RunRoiBatch(batch, (114, 114, 114), rects=tensor) == (True, vali.TaskExecInfo.SUCCESS)
        crops.append([download(vali, gpu, d) for d in dsts])
    used = want_d[:, 0] >= 0
    for k, (x, y) in enumerate(zip(*crops)):
        assert np.array_equal(x, y), k
    assert len({crops[0][k].tobytes() for k in np.flatnonzero(used)}) >= 3        # different boxes give different crops
