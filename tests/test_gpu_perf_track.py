"""Speed of PyDetectionTracker.RunAsync next to the call it follows in every pipeline, PyDetectionSelector.RunAsync on the
YOLOv8-sized head tests/test_gpu_perf_detect.py times (16 x 8400 x 80 float16, T = 1024, D = 100, about 300 candidates a
frame passing).  The tracker: 16 streams of one frame, D = 100 rows of which about 30 a frame are detections, 128 slots
a stream, about 30 live tracks a stream that the rows match, with tracked, assoc and marks all written.

Both on one stream in one process, each run between two events, the median of 25 runs after warm-up, the two
alternating.  The aim was that the tracker costs no more than the selector.  Measured on an MI355X: RunAsync 34.2 us
against 42.1 us for the selector, ratio 0.81 (five runs: 0.822, 0.811, 0.806, 0.805, 0.823; profiles/track.md).  The
bound is that ratio times 1.25, the margin tests/test_gpu_perf_pose.py gives for the spread from box to box."""
import numpy as np
import pytest

import track_model as tm
from test_gpu_perf_detect import IOU, LETTERBOX, THR, C, D, K, N, T, _medians, yolo_head

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

STREAMS, SLOTS, OBJECTS = 16, 128, 30
MEASURED_RATIO = 0.81
BOUND = 1.01           # MEASURED_RATIO * 1.25


def street(seed=0):
    """(16 * 100, 8) rows: about 30 boxes a frame on a 1920 x 1080 frame, apart from each other, of 8 classes"""
    rng = np.random.default_rng(seed)
    boxes = {}
    for i in range(STREAMS):
        cells = rng.permutation(8 * 5)[:OBJECTS + int(rng.integers(-3, 4))]
        boxes[i] = [(int(240 * (c % 8) + rng.integers(0, 60)), int(216 * (c // 8) + rng.integers(0, 40)),
                     int(rng.integers(80, 170)), int(rng.integers(80, 170)), int(rng.integers(0, 8)),
                     float(0.5 + 0.45 * rng.random())) for c in cells]
    return tm.det_rows(STREAMS, D, boxes)


def test_run_costs_no_more_than_its_share_of_the_selector(vali, gpu):
    torch.cuda.set_device(gpu)
    stream = torch.cuda.current_stream(gpu).cuda_stream
    dev = f"cuda:{gpu}"
    # the selector, as tests/test_gpu_perf_detect.py sets it up
    pred = yolo_head(gpu)
    boxes, scores = pred[:, :4].transpose(1, 2), pred[:, 4:].transpose(1, 2)
    s_dets = torch.zeros((N * D, 8), dtype=torch.int32, device=dev)
    counts = torch.zeros((N,), dtype=torch.int32, device=dev)
    rois, s_marks = torch.zeros_like(s_dets), torch.zeros_like(s_dets)
    rects = torch.tensor([LETTERBOX] * N, dtype=torch.int32, device=dev)
    colours = torch.tensor([vali.pack_colour(40, 255, 80), vali.pack_colour(250, 20, 20)], dtype=torch.int32, device=dev)
    style = vali.DetectionStyle(colours=colours)
    # the tracker
    rows = street()
    dets = torch.from_numpy(rows).to(dev)
    tracks = torch.zeros((STREAMS * SLOTS, 16), dtype=torch.int32, device=dev)
    clock = torch.zeros((STREAMS, 4), dtype=torch.int32, device=dev)
    tracked, marks = torch.zeros_like(dets), torch.zeros_like(dets)
    assoc = torch.zeros((STREAMS * D, 4), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    sel = vali.PyDetectionSelector(gpu, stream)
    sb = sel.Prepare(boxes, scores, s_dets, counts, rois, s_marks, max_candidates=T, max_det=D)
    tk = vali.PyDetectionTracker(gpu, stream)
    tb = tk.Prepare(dets, tracks, clock, tracked, assoc, marks, streams=STREAMS, max_det=D, max_tracks=SLOTS)

    def select():
        assert sel.RunAsync(sb, rects, THR, IOU, crop_placement=(0, 0, 224, 224), style=style)[0]

    def track():
        assert tk.RunAsync(tb, style=style)[0]

    for _ in range(4):      # the tracks are born, confirmed and matched: the steady state of a street that stands still
        track()
    torch.cuda.synchronize()
    live = (tracks[:, 0] > 0).view(STREAMS, SLOTS).sum(1).cpu().numpy()
    shown = (tracked[:, 0] >= 0).view(STREAMS, D).sum(1).cpu().numpy()
    valid = (rows[:, 0] >= 0).reshape(STREAMS, D).sum(1)
    assert (np.abs(valid - OBJECTS) <= 3).all() and np.array_equal(live, valid), (valid, live)
    assert np.array_equal(shown, live) and (tracks[:, 8].max().item() == 4)
    t_track, t_select = _medians([track, select])
    torch.cuda.synchronize()
    assert tracks[:, 8].min().item() == 0 and tracks[:, 8].max().item() >= 30          # the timed calls went on matching
    ratio = t_track / t_select
    print(f"\ntrack {STREAMS} streams x {D} rows (~{OBJECTS} detections), {SLOTS} slots, ~{int(live.mean())} live tracks: RunAsync "
          f"{t_track * 1e3:.1f} us (1 launch); PyDetectionSelector.RunAsync {N} x {K} x {C} float16 {t_select * 1e3:.1f} us "
          f"(4 launches); ratio {ratio:.3f}")
    assert BOUND is not None, "the bound has not been set from a measurement"
    assert ratio <= BOUND, f"RunAsync {t_track * 1e3:.1f} us vs the selector's {t_select * 1e3:.1f} us: ratio {ratio:.3f} > {BOUND}"
