"""Selector -> masker -> annotator on one small batch, with no host read of `dets` in between: the selector's dets tensor
goes straight into PyInstanceMasker.Prepare and its marks into PySurfaceAnnotator.RunBatch.  The final frames equal the
three models chained (tests/detect_model.py, tests/mask_model.py, tests/annotate_model.py)."""
import numpy as np
import pytest

import annotate_model as am
import detect_model as dm
import mask_cases as mc
import mask_model as mm
import postproc_model as pm
from test_detect_host import random_head
from test_gpu_annotate import download, make_frames

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SIZES = [(96, 80), (96, 80), (70, 50)]
N, K, C, D, M = 3, 65, 4, 4, 5
RECT = (0, 0, 96, 80, 0, 5, 64, 53)            # the letterbox of a 96 x 80 frame in the 64 x 64 network input
NET = (64, 64)


@pytest.mark.parametrize("fmt", ["NV12", "RGB"])
def test_selector_masker_annotator(vali, gpu, fmt):
    dev = f"cuda:{gpu}"
    boxes, scores, _ = random_head(7, N, K, C, "xyxy", RECT)
    rects = [RECT, RECT, (0, 0, 70, 50, 0, 9, 0, 46)]              # the last frame has no detections
    rng = np.random.default_rng(5)
    coeffs = rng.standard_normal((N, K, M)).astype(np.float32)
    protos = mc.protos(M, 16, 16, n=N)
    colours = [vali.pack_colour(40, 255, 80), vali.pack_colour(250, 20, 20), vali.pack_colour(20, 40, 250)]
    b, s = torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev)
    pt, ct = torch.from_numpy(protos).to(dev), torch.from_numpy(coeffs).to(dev)
    dets = torch.zeros((N * D, 8), dtype=torch.int32, device=dev)
    marks = torch.zeros((N * D, 8), dtype=torch.int32, device=dev)
    rects_t = torch.tensor(np.asarray(rects, np.int32), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    frames, hosts = make_frames(vali, gpu, fmt, SIZES, seed=21)
    untouched = hosts[2].copy()

    sel, mk, ann = vali.PyDetectionSelector(gpu), vali.PyInstanceMasker(gpu), vali.PySurfaceAnnotator(gpu)
    sb = sel.Prepare(b, s, dets, marks=marks, max_candidates=64, max_det=D)
    mb = mk.Prepare(frames, pt, ct, dets, max_det=D, net_size=NET)
    ab = ann.PrepareBatch(frames)
    style = vali.DetectionStyle(thickness=2, colours=colours)
    assert sel.RunAsync(sb, rects_t, 0.5, 0.3, style=style) == (True, vali.TaskExecInfo.SUCCESS)
    assert mk.RunAsync(mb, rects_t, colours, alpha=120) == (True, vali.TaskExecInfo.SUCCESS)
    assert ann.RunBatch(ab, marks) == (True, vali.TaskExecInfo.SUCCESS)

    want_d, want_c = dm.select(boxes, scores, np.asarray(rects, np.int32), 0.5, 0.3, False, "xyxy", 64, D)
    assert want_c.tolist()[2] == 0 and want_c[0] >= 2 and want_c[1] >= 2
    rows = pm.matrices()["601_JPEG"]
    drawn = mm.apply(hosts, fmt, SIZES, want_d, D, protos, coeffs, rects, colours, 120, NET, rows)
    assert len(drawn) == int(want_c.sum())
    assert sum(0.05 <= d[2].mean() <= 0.95 for d in drawn) >= 3          # the masks are no trivial ones
    am.apply(hosts, fmt, SIZES, dm.marks_of(want_d, colours, 2), rows)
    for i, f in enumerate(frames):
        assert np.array_equal(download(vali, gpu, f), hosts[i]), (fmt, i)
    assert np.array_equal(hosts[2], untouched)
    assert np.array_equal(dets.cpu().numpy(), want_d)                      # read only now, after everything ran
