"""PyDetectionTracker without a GPU: the definition (tests/track_model.py) on planted objects and on hand-made cases with
the expected rows written out, the F = 4 / four F = 1 equivalence, every ValueError of Prepare and Run, and the C entry
point's refusals through ctypes."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

import track_model as tm
from track_model import AGE, CLS, HITS, ID, MISSES, VX, X

ROOT = Path(__file__).resolve().parent.parent
F = np.float32


def bits(v):
    return int(np.array([v], F).view(np.int32)[0])


def empty_state(S, T):
    return np.zeros((S * T, 16), np.int32), np.zeros((S, 4), np.int32)


def run_frames(frames, D, T, **kw):
    """`frames`: a list of [(x, y, w, h, class, score), ...], one stream, one call per frame.  Returns the per-frame
    (tracks, clock, tracked, assoc)."""
    tracks, clock = empty_state(1, T)
    out = []
    for items in frames:
        tracks, clock, tracked, assoc = tm.update(tm.det_rows(1, D, {0: items}), tracks, clock, 1, D, T, **kw)
        out.append((tracks, clock, tracked, assoc))
    return out


# ---- planted objects -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_six_objects_on_lanes_keep_one_id_each(seed):
    """constant velocities up to 12 px / frame, +-2 px of jitter, 15 % of the detections dropped, 90 frames, default
    parameters: every object shows under exactly one id and six ids show in all"""
    rng = np.random.default_rng(seed)
    vel = [-12, -7, -3, 3, 8, 12]
    x0 = [1400, 1000, 600, 300, 200, 100]
    D, T = 8, 16
    frames = []
    for f in range(90):
        items = []
        for o in range(6):
            if rng.random() < 0.15:
                continue
            jx, jy = rng.integers(-2, 3, 2)
            # the lane is told by y; the score decides the order of the rows, not the lane
            items.append((x0[o] + vel[o] * f + int(jx), 150 * o + 10 + int(jy), 60, 100, 0, 0.6 + 0.3 * rng.random()))
        frames.append(items)
    seen = [set() for _ in range(6)]
    shown = 0
    for _, _, tracked, _ in run_frames(frames, D, T):
        for row in tracked[tracked[:, 0] >= 0]:
            seen[(int(row[2]) + 20) // 150].add(int(row[5]))
            shown += 1
    assert all(len(s) == 1 for s in seen), seen
    assert len(set().union(*seen)) == 6
    assert shown > 0.7 * 90 * 6                 # and the objects really were followed, not just never confirmed


@pytest.mark.parametrize("momentum, ids", [(0.5, 1), (0.0, 2)])
def test_the_prediction_is_what_bridges_an_occlusion(momentum, ids):
    """one object at 12 px / frame, 60 x 120, unseen for frames 30..39: with a velocity it is found again where it was
    predicted; without one it has moved 132 px from where it was last seen, more than its width"""
    frames = [[] if 30 <= f <= 39 else [(100 + 12 * f, 50, 60, 120, 2, 0.9)] for f in range(60)]
    seen = set()
    for f, (_, _, tracked, _) in enumerate(run_frames(frames, 2, 4, momentum=momentum)):
        seen |= {int(r[5]) for r in tracked if r[0] >= 0}
        if 30 <= f <= 39:
            assert (tracked[:, 0] == -1).all()
    assert len(seen) == ids, seen


# ---- edge rules ------------------------------------------------------------------------------------------------------
BOX = (100, 50, 40, 80, 1, 0.9)
S9 = bits(F(0.9))


def test_a_one_frame_flicker_never_shows():
    out = run_frames([[BOX], [], [BOX], [BOX], [BOX]], 2, 2, min_hits=3)
    tracks, clock, tracked, assoc = out[0]
    assert tracks[0].tolist() == [1, 1, 100, 50, 40, 80, 0, 0, 1, 0, 1, S9, 0, 0, 0, 0]
    assert assoc.tolist() == [[1, 0, 1, 1], [0, -1, 0, 0]]
    assert tracked.tolist() == [[-1, 0, 0, 0, 0, 0, 0, 0]] * 2
    # its first miss ends a tentative track: nothing is left of id 1
    tracks, clock, tracked, assoc = out[1]
    assert not tracks.any() and clock.tolist() == [[2, 2, 0, 0]]
    # the box returns under id 2 and shows from its third hit
    assert [o[2][0].tolist() for o in out[2:]] == [[-1, 0, 0, 0, 0, 0, 0, 0]] * 2 + [[0, 100, 50, 40, 80, 2, S9, 0]]
    assert out[4][3][0].tolist() == [2, 0, 3, 1]
    assert out[4][0][0].tolist() == [2, 1, 100, 50, 40, 80, 0, 0, 3, 0, 3, S9, 0, 0, 0, 0]


def test_a_track_dies_after_max_age_plus_one_misses():
    out = run_frames([[BOX]] * 3 + [[]] * 4, 1, 2, max_age=2)
    assert out[2][2][0].tolist() == [0, 100, 50, 40, 80, 1, S9, 0]
    for f, misses in ((3, 1), (4, 2)):
        assert out[f][0][0].tolist() == [1, 1, 100, 50, 40, 80, 0, 0, 3, misses, 3 + misses, S9, 0, 0, 0, 0]
    assert not out[5][0].any()                  # the third miss is max_age + 1
    assert out[6][1].tolist() == [[2, 7, 0, 0]]


def test_a_row_below_new_thr_continues_a_track_and_starts_none():
    weak = (100, 50, 40, 80, 1, 0.2)
    out = run_frames([[weak], [BOX], [weak], [weak]], 1, 2)
    assert not out[0][0].any() and out[0][3].tolist() == [[0, -1, 0, 0]]
    assert out[1][3].tolist() == [[1, 0, 1, 1]]
    assert out[2][3].tolist() == [[1, 0, 2, 1]] and out[3][3].tolist() == [[1, 0, 3, 1]]
    assert out[3][2].tolist() == [[0, 100, 50, 40, 80, 1, bits(F(0.2)), 0]]
    assert out[3][0][0, 11] == bits(F(0.2))


def test_a_full_table_means_no_birth():
    items = [(100 * q, 0, 40, 40, 0, 0.9 - 0.1 * q) for q in range(3)]
    (tracks, clock, tracked, assoc), = run_frames([items], 4, 2, min_hits=1)
    assert tracks[:, ID].tolist() == [1, 2] and clock.tolist() == [[3, 1, 0, 0]]
    assert assoc.tolist() == [[1, 0, 1, 0], [2, 1, 1, 0], [0, -1, 0, 0], [0, -1, 0, 0]]
    assert tracked[:, 0].tolist() == [0, 0, -1, -1] and tracked[:, 5].tolist() == [1, 2, 0, 0]


def test_class_gating_and_class_agnostic():
    first, other = [(100, 50, 40, 80, 1, 0.9)], [(100, 50, 40, 80, 2, 0.9)]
    gated = run_frames([first, other], 1, 4, min_hits=1)[1]
    assert gated[3].tolist() == [[2, 1, 1, 2]]              # a new track in slot 1; id 1 counts a miss in slot 0
    assert gated[0][:2, ID].tolist() == [1, 2] and gated[0][:2, MISSES].tolist() == [1, 0]
    assert gated[0][:2, CLS].tolist() == [1, 2]
    agnostic = run_frames([first, other], 1, 4, min_hits=1, class_agnostic=True)[1]
    assert agnostic[3].tolist() == [[1, 0, 2, 2]]
    assert agnostic[0][0].tolist() == [1, 2, 100, 50, 40, 80, 0, 0, 2, 0, 2, S9, 0, 0, 0, 0]


def test_equal_ious_go_to_the_lowest_slot():
    # two tracks side by side, then one box exactly between them: both IoUs are 20 * 80 / (2 * 3200 - 1600)
    out = run_frames([[(100, 50, 40, 80, 0, 0.9), (140, 50, 40, 80, 0, 0.8)], [(120, 50, 40, 80, 0, 0.9)]], 2, 4, min_hits=1)
    assert out[0][3].tolist() == [[1, 0, 1, 0], [2, 1, 1, 0]]
    tracks, _, tracked, assoc = out[1]
    assert assoc.tolist() == [[1, 0, 2, 0], [0, -1, 0, 0]]
    assert tracks[0, X] == 120 and tracks[0, VX] == bits(F(10.0)) and tracks[1, MISSES] == 1
    # the same with the slots' order reversed: the winner is the slot, not the id or the side
    t0, c0 = out[0][0].copy(), out[0][1]
    t0[[0, 1]] = t0[[1, 0]]
    _, _, _, assoc = tm.update(tm.det_rows(1, 2, {0: [(120, 50, 40, 80, 0, 0.9)]}), t0, c0, 1, 2, 4, min_hits=1)
    assert assoc[0].tolist() == [2, 0, 2, 0]


def test_the_id_wraps_after_int32_max():
    tracks, clock = empty_state(1, 4)
    clock[0] = 2**31 - 1, 5, 7, 7
    items = [(100 * q, 0, 40, 40, 0, 0.9 - 0.1 * q) for q in range(2)]
    tracks, clock, tracked, assoc = tm.update(tm.det_rows(1, 2, {0: items}), tracks, clock, 1, 2, 4, min_hits=1)
    assert assoc[:, 0].tolist() == [2**31 - 1, 1] and clock.tolist() == [[2, 6, 0, 0]]
    # a next_id below 1 reads as 1
    t0, c0 = empty_state(1, 4)
    c0[0, 0] = -5
    _, c1, _, assoc = tm.update(tm.det_rows(1, 2, {0: items}), t0, c0, 1, 2, 4)
    assert assoc[:, 0].tolist() == [1, 2] and c1[0, 0] == 3


def test_foreign_track_rows_are_free_and_counters_are_clamped():
    tracks, clock = empty_state(1, 4)
    tracks[0] = [7, 0, 10, 10, 0, 40] + [0] * 10                 # w < 1: free
    tracks[1] = [0, 0, 10, 10, 40, 40] + [0] * 10                # id < 1: free
    tracks[2] = [9, 3, 10, 10, 40, 40, 0, 0, 2**31 - 1, -3, -(2**31), 5, 6, 1, 2, 3]
    tracks, clock, _, _ = tm.update(tm.det_rows(1, 1, {}), tracks, clock, 1, 1, 4)
    assert not tracks[[0, 1, 3]].any()
    assert tracks[2].tolist() == [9, 3, 10, 10, 40, 40, 0, 0, 2**30, 1, 1, 5, 6, 0, 0, 0]


# ---- equivalence -----------------------------------------------------------------------------------------------------
def moving_scene(seed, S, Fr, D, calls):
    """`calls` lists of {frame: items} for S streams of Fr frames per call: objects that move, flicker, appear and leave"""
    rng = np.random.default_rng(seed)
    objs = [[(rng.integers(0, 600), rng.integers(0, 300), rng.integers(20, 80), rng.integers(20, 80), rng.integers(0, 3),
              rng.integers(-9, 10), rng.integers(-5, 6)) for _ in range(min(D, 6))] for _ in range(S)]
    out = []
    for c in range(calls):
        boxes = {}
        for s in range(S):
            for f in range(Fr):
                t = c * Fr + f
                items = []
                for (x, y, w, h, cls, vx, vy) in objs[s]:
                    if rng.random() < 0.25:
                        continue
                    items.append((int(x + vx * t), int(y + vy * t), int(w), int(h), int(cls), float(F(rng.choice([0.3, 0.6, 0.9])))))
                boxes[s * Fr + f] = items[:D]
        out.append(boxes)
    return out


def test_one_call_with_four_frames_equals_four_calls_with_one():
    S, D, T = 2, 5, 3
    calls = moving_scene(4, S, 4, D, 3)
    ta, ca = empty_state(S, T)
    tb, cb = empty_state(S, T)
    births = 0
    for boxes in calls:
        ta, ca, tracked, assoc = tm.update(tm.det_rows(S * 4, D, boxes), ta, ca, S, D, T, min_hits=2, max_age=2)
        for f in range(4):
            one = {s: boxes[s * 4 + f] for s in range(S)}
            tb, cb, tr1, as1 = tm.update(tm.det_rows(S, D, one), tb, cb, S, D, T, min_hits=2, max_age=2)
            for s in range(S):
                big = slice((s * 4 + f) * D, (s * 4 + f + 1) * D)
                want = tr1[s * D:(s + 1) * D].copy()
                want[want[:, 0] >= 0, 0] = s * 4 + f
                assert np.array_equal(tracked[big], want) and np.array_equal(assoc[big], as1[s * D:(s + 1) * D])
        assert np.array_equal(ta, tb) and np.array_equal(ca, cb)
        births += int((assoc[:, 2] == 1).sum())
    assert births > 3 and ca[:, 1].tolist() == [12, 12] and (ta[:, HITS] > 1).any() and (ta[:, AGE] > ta[:, HITS]).any()


def test_marks_follow_the_id():
    tracked = np.asarray([[0, 10, 40, 100, 80, 7, 0, 5], [-1, 0, 0, 0, 0, 0, 0, 0], [1, 7, 9, 30, 20, 102, 0, 1]], np.int32)
    colours = [tm.pack_colour(1, 2, 3), tm.pack_colour(200, 0, 0, 128), tm.pack_colour(0, 0, 9)]
    rects = [[u, 12 * u, 10 + u, 12] for u in range(100)]
    got = tm.marks_of(tracked, colours, 2, rects, 200, 77)
    c7, c102 = colours[7 % 3], colours[102 % 3]
    assert got[:3].tolist() == [[0, 10, 40, 100, 80, 1, 2, c7], [0] * 8, [1, 7, 9, 30, 20, 1, 2, c102]]
    assert got[3].tolist() == [0, 10, 40 - 12, 17, 12, 2, 0, tm.i32((c7 & 0xFFFFFF) | 200 << 24)]
    assert got[6].tolist() == [0, 10, 40 - 12, 17, 12, 4, 7 | (84 << 16), 77]
    assert got[8].tolist() == [1, 7, 9 - 12, 12, 12, 4, 2 | (24 << 16), 77]        # id 102 prints "02"
    assert not got[[4, 7]].any()
    assert tm.marks_of(tracked, colours).shape == (3, 8)


# ---- the Python layer's refusals ---------------------------------------------------------------------------------------
class FakeDevice:
    def __init__(self, kind, index):
        self.type, self.index = kind, index


class FakeTensor:
    """what Prepare reads of a device tensor, without a device"""

    def __init__(self, shape, typestr="<i4", strides=None, device_type="cuda", index=0, ptr=4096):
        self.shape = tuple(shape)
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 3,
                                         "strides": strides}
        self.device = FakeDevice(device_type, index)


def test_prepare_says_what_is_wrong():
    from vali_amd.track import TrackBatch, track_spec

    S, D, T, N = 2, 5, 3, 4
    good = dict(dets=FakeTensor((N * D, 8)), tracks=FakeTensor((S * T, 16)), clock=FakeTensor((S, 4)),
                tracked=FakeTensor((N * D, 8)))

    def prepare(streams=S, max_det=D, max_tracks=T, **kw):
        return TrackBatch(0, 0x5EED, **{**good, **kw}, streams=streams, max_det=max_det, max_tracks=max_tracks)

    tb = prepare(assoc=FakeTensor((N * D, 4)), marks=FakeTensor((3 * N * D, 8)))
    assert (tb.n, tb.S, tb.F, tb.D, tb.T, tb.R, len(tb)) == (N, S, 2, D, T, 3, N)
    assert prepare().R == 0 and prepare(marks=FakeTensor((N * D, 8))).R == 1
    for kw, text in [
        (dict(dets=None), "dets: an int32 device tensor is required"),
        (dict(tracks=None), "tracks: an int32"), (dict(clock=None), "clock: an int32"), (dict(tracked=None), "tracked: an int32"),
        (dict(dets=FakeTensor((N * D + 1, 8))), "dets: need (N * max_det, 8) rows with max_det = 5, got 21"),
        (dict(dets=FakeTensor((N * D, 7))), "dets: need an int32 tensor of shape (20x8)"),
        (dict(dets=FakeTensor((N * D * 8,))), "dets: need (N * max_det, 8) rows"),
        (dict(dets=FakeTensor((N * D, 8), "<f4")), "dets: need an int32"),
        (dict(tracks=FakeTensor((S * T + 1, 16))), "tracks: need an int32 tensor of shape (6x16)"),
        (dict(tracks=FakeTensor((S * T, 8))), "tracks: need an int32 tensor of shape (6x16)"),
        (dict(clock=FakeTensor((S + 1, 4))), "clock: need an int32 tensor of shape (2x4)"),
        (dict(tracked=FakeTensor((N * D, 4))), "tracked: need an int32 tensor of shape (20x8)"),
        (dict(assoc=FakeTensor((N * D, 8))), "assoc: need an int32 tensor of shape (20x4)"),
        (dict(marks=FakeTensor((2 * N * D, 8))), "marks: need (20, 8) rows (outlines) or (60, 8)"),
        (dict(marks=FakeTensor((N * D, 4))), "marks: need an int32 tensor of shape (20x8)"),
        (dict(streams=3), "N = 4 frames is not a multiple of streams = 3"),
        (dict(streams=0), "streams = 0 is outside 1..1024"), (dict(streams=1025), "streams = 1025 is outside"),
        (dict(max_det=0), "max_det = 0 is outside 1..1024"),
        (dict(max_tracks=0), "max_tracks = 0 is outside 1..256"), (dict(max_tracks=257), "max_tracks = 257 is outside 1..256"),
        (dict(tracks=FakeTensor((S * T, 16), strides=(128, 4))), "tracks: the tensor must be contiguous"),
        (dict(dets=FakeTensor((N * D, 8), strides=(4, 80))), "dets: the tensor must be contiguous"),
        (dict(tracks=FakeTensor((S * T, 16), ptr=4096 + 8)), "tracks: the tensor must be 16-byte aligned"),
        (dict(clock=FakeTensor((S, 4), device_type="cpu")), "clock: the tensor must live on the GPU"),
        (dict(tracked=FakeTensor((N * D, 8), index=1)), "tracked: the tensor is on device 1, the task on 0"),
    ]:
        with pytest.raises(ValueError) as e:
            prepare(**kw)
        assert text in str(e.value), (kw, str(e.value))
    # the limits, on sizes alone
    assert track_spec(1024 * 63, 1024, 63, 256) == (1024, 1, 1024, 63, 256, 0)
    assert track_spec(4096, 1, 4, 1, 4096) == (1, 1024, 1024, 4, 1, 1)
    for args, text in [((1025 * 2, 1, 2, 4), "N = 1025 frames; need 1..1024"),
                       ((1024 * 64, 1, 64, 4), "N * max_det = 65536 exceeds 65535"),
                       ((1025, 1, 1025, 4), "max_det = 1025 is outside 1..1024"),
                       ((5000, 1, 5, 4, 5000), "marks: 5000 rows; the annotator takes at most 4096"),
                       ((3, 1, 5, 4), "dets: need (N * max_det, 8) rows")]:
        with pytest.raises(ValueError) as e:
            track_spec(*args)
        assert text in str(e.value), (args, str(e.value))


def test_run_says_what_is_wrong():
    from vali_amd.detect import DetectionStyle
    from vali_amd.track import run_spec

    plain, labelled = DetectionStyle(), DetectionStyle(label_rects=[(0, 0, 10, 5)])
    assert run_spec(0, 0.3, 0.5, 3, 30, 0.5, None) == (0.3, 0.5, 3, 30, 0.5)
    assert run_spec(1, -1.0, 0.0, 1, 0, 0.0, plain) and run_spec(3, 0.3, 0.5, 2**31 - 1, 2**20, 1.0, labelled)
    for args, text in [((0, float("nan"), 0.5, 3, 30, 0.5, None), "iou_thr must be finite"),
                       ((0, float("inf"), 0.5, 3, 30, 0.5, None), "iou_thr must be finite"),
                       ((0, 0.3, float("nan"), 3, 30, 0.5, None), "new_thr must be finite"),
                       ((0, 0.3, -float("inf"), 3, 30, 0.5, None), "new_thr must be finite"),
                       ((0, 0.3, 0.5, 3, 30, 1.5, None), "momentum = 1.5 is outside 0..1"),
                       ((0, 0.3, 0.5, 3, 30, -0.1, None), "momentum = -0.1 is outside 0..1"),
                       ((0, 0.3, 0.5, 3, 30, float("nan"), None), "momentum = nan is outside 0..1"),
                       ((0, 0.3, 0.5, 0, 30, 0.5, None), "min_hits = 0 is below 1"),
                       ((0, 0.3, 0.5, 3, -1, 0.5, None), "max_age = -1 is outside 0..2^20"),
                       ((0, 0.3, 0.5, 3, 2**20 + 1, 0.5, None), "max_age = 1048577 is outside 0..2^20"),
                       ((1, 0.3, 0.5, 3, 30, 0.5, None), "style: a DetectionStyle is required"),
                       ((1, 0.3, 0.5, 3, 30, 0.5, labelled), "style: marks of 3 * N * max_det rows need"),
                       ((3, 0.3, 0.5, 3, 30, 0.5, plain), "style: marks of 3 * N * max_det rows need")]:
        with pytest.raises(ValueError) as e:
            run_spec(*args)
        assert text in str(e.value), (args, str(e.value))
    with pytest.raises(TypeError):
        run_spec(0, 0.3, 0.5, 2.5, 30, 0.5, None)


def test_run_takes_a_track_batch_only():
    import vali_amd as vali

    tk = vali.PyDetectionTracker.__new__(vali.PyDetectionTracker)
    with pytest.raises(ValueError, match="pass a TrackBatch"):
        tk.RunAsync(object())


def test_the_names_are_exported():
    import python_vali
    import vali_amd

    for name in ("PyDetectionTracker", "TrackBatch"):
        assert getattr(python_vali, name) is getattr(vali_amd, name)


# ---- the C entry point -------------------------------------------------------------------------------------------------
class Params(ctypes.Structure):
    """include/vali_hip.h: vali_track_params"""
    _fields_ = [(n, ctypes.c_int32) for n in ("streams", "frames", "max_det", "max_tracks")] + \
               [(n, ctypes.c_float) for n in ("iou_thr", "new_thr", "momentum")] + \
               [(n, ctypes.c_int32) for n in ("min_hits", "max_age", "class_agnostic", "thickness", "label_alpha",
                                              "text_colour", "n_colours", "n_labels", "reserved")]


class Io(ctypes.Structure):
    """include/vali_hip.h: vali_track_io"""
    _fields_ = [(n, ctypes.c_void_p) for n in ("dets", "tracks", "clock", "tracked", "assoc", "marks", "colours",
                                               "label_rects")]


def test_struct_sizes_match_the_header():
    assert (ctypes.sizeof(Params), ctypes.sizeof(Io)) == (64, 64)


def test_the_c_entry_point_refuses_before_any_device_is_touched():
    lib = ctypes.CDLL(str(ROOT / "vali_amd" / "libvali_hip.so"))
    lib.vali_last_error.restype = ctypes.c_char_p
    lib.vali_track_update.argtypes = [ctypes.c_void_p] * 3
    buf = ctypes.create_string_buffer(256)        # never read: every call below is refused first
    base = (ctypes.addressof(buf) + 15) & ~15

    def call(io_changes=(), **changes):
        p = Params(2, 2, 5, 3, 0.3, 0.5, 0.5, 3, 30, 0, 2, 200, 0, 1, 0, 0)
        for k, v in changes.items():
            setattr(p, k, v)
        io = Io(base, base, base, base, None, None, None, None)
        for k, v in dict(io_changes).items():
            setattr(io, k, v)
        return lib.vali_track_update(ctypes.byref(p), ctypes.byref(io), None), lib.vali_last_error()

    assert lib.vali_track_update(None, None, None) == -1 and b"null" in lib.vali_last_error()
    io = Io(base, base, base, base, None, None, None, None)
    assert lib.vali_track_update(None, ctypes.byref(io), None) == -1
    for name in ("dets", "tracks", "clock", "tracked"):
        rc, msg = call({name: None})
        assert rc == -1 and b"null" in msg, name
    for io_changes, text in [({"tracks": base + 4}, b"tracks are not 16-byte aligned"),
                             ({"tracks": base + 8}, b"tracks are not 16-byte aligned"),
                             ({"dets": base + 2}, b"not 4-byte aligned"), ({"clock": base + 1}, b"not 4-byte aligned"),
                             ({"tracked": base + 3}, b"not 4-byte aligned"), ({"assoc": base + 2}, b"not 4-byte aligned"),
                             ({"marks": base + 2, "colours": base}, b"not 4-byte aligned"),
                             ({"marks": base}, b"marks without colours"),
                             ({"marks": base, "colours": base, "label_rects": base}, b"label_rects without n_labels")]:
        rc, msg = call(io_changes)
        assert rc == -1 and text in msg, (io_changes, msg)
    for changes, text in [(dict(streams=0), b"streams"), (dict(streams=1025), b"streams"), (dict(frames=0), b"frames"),
                          (dict(frames=513), b"frames"), (dict(max_det=0), b"max_det"), (dict(max_det=1025), b"max_det"),
                          (dict(streams=1024, frames=1, max_det=64), b"65535"),
                          (dict(max_tracks=0), b"max_tracks"), (dict(max_tracks=257), b"max_tracks"),
                          (dict(iou_thr=float("nan")), b"iou_thr"), (dict(new_thr=float("inf")), b"new_thr"),
                          (dict(momentum=float("nan")), b"momentum"), (dict(momentum=1.5), b"momentum"),
                          (dict(momentum=-0.5), b"momentum"), (dict(min_hits=0), b"min_hits"),
                          (dict(max_age=-1), b"max_age"), (dict(max_age=2**20 + 1), b"max_age")]:
        rc, msg = call(**changes)
        assert rc == -1 and text in msg, (changes, msg)
    marks = {"marks": base, "colours": base}
    for changes, text in [(dict(n_colours=0), b"marks without colours"), (dict(thickness=0), b"thickness"),
                          (dict(label_alpha=256), b"label_alpha"), (dict(streams=64, frames=16, max_det=5), b"4096")]:
        rc, msg = call(marks, **changes)
        assert rc == -1 and text in msg, (changes, msg)
