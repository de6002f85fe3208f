"""PyDetectionTracker on the GPU against tests/track_model.py, bit for bit: tracks, clock, tracked, assoc and marks after
EVERY call of a sequence of 6 to 12 calls on seeded scenes (tests/track_cases.py) in which objects are matched, missed,
born and lost and boxes lie exactly between two tracks.  S in {1, 3}, F in {1, 4}, D in {1, 5, 70} (70: rows in a second
group of 64), T in {1, 3, 64, 65, 256} (a full table, the lane boundary, four tracks a lane), R in {0, 1, 3}; arbitrary
int32 values in dets, tracks and clock, with sentinel rows around everything that is written; F = 4 against four calls
with F = 1; a captured call replayed after dets was rewritten in place."""
import numpy as np
import pytest

import track_cases as tc
import track_model as tm

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GARBAGE = 0x5A5A5A5A
PAD = 3
COLOURS = [tm.pack_colour(40, 255, 80), tm.pack_colour(255, 0, 0, 128), tm.pack_colour(1, 2, 3, 0)]
LABELS = [[7 * (q % 10), 12 * (q // 10), 9 + q % 5, 12] for q in range(100)]


def padded(rows, cols, dev):
    """(whole, view): `rows` rows with PAD sentinel rows before and after"""
    whole = torch.full((rows + 2 * PAD, cols), GARBAGE, dtype=torch.int32, device=dev)
    return whole, whole[PAD:PAD + rows]


def untouched(whole):
    w = whole.cpu().numpy()
    return (w[:PAD] == GARBAGE).all() and (w[-PAD:] == GARBAGE).all()


class Rig:
    """the device tensors of one tracker, the model's state next to them, and the comparison after a call"""

    def __init__(self, vali, gpu, S, Fr, D, T, R, state=None, stream=None):
        self.vali, self.S, self.Fr, self.D, self.T, self.R = vali, S, Fr, D, T, R
        dev = f"cuda:{gpu}"
        n = S * Fr
        self.dets = torch.zeros((n * D, 8), dtype=torch.int32, device=dev)
        self.wholes = {}
        for name, rows, cols in (("tracks", S * T, 16), ("clock", S, 4), ("tracked", n * D, 8), ("assoc", n * D, 4),
                                 ("marks", max(R, 1) * n * D, 8)):
            self.wholes[name], view = padded(rows, cols, dev)
            setattr(self, name, view)
        self.m_tracks, self.m_clock = state if state is not None else (np.zeros((S * T, 16), np.int32), np.zeros((S, 4), np.int32))
        self.tracks.copy_(torch.from_numpy(self.m_tracks))
        self.clock.copy_(torch.from_numpy(self.m_clock))
        self.style = None
        if R:
            self.style = vali.DetectionStyle(thickness=3, colours=COLOURS, label_rects=LABELS if R == 3 else None,
                                             label_alpha=180, text_colour=tm.pack_colour(9, 9, 9))
        torch.cuda.synchronize()
        self.task = vali.PyDetectionTracker(gpu) if stream is None else vali.PyDetectionTracker(gpu, stream)
        self.batch = self.task.Prepare(self.dets, self.tracks, self.clock, self.tracked, self.assoc,
                                       self.marks if R else None, streams=S, max_det=D, max_tracks=T)

    def load(self, rows):
        self.dets.copy_(torch.from_numpy(rows))
        for t in (self.tracked, self.assoc, self.marks):
            t.fill_(GARBAGE)
        torch.cuda.synchronize()

    def step(self, rows, **params):
        self.load(rows)
        assert self.task.Run(self.batch, style=self.style, **params) == (True, self.vali.TaskExecInfo.SUCCESS)
        return self.check(rows, **params)

    def check(self, rows, **params):
        """the model's call on the same rows; everything compared; returns the model's (tracked, assoc)"""
        before = self.m_tracks
        self.m_tracks, self.m_clock, tracked, assoc = tm.update(rows, self.m_tracks, self.m_clock, self.S, self.D, self.T, **params)
        for name, want in (("tracks", self.m_tracks), ("clock", self.m_clock), ("tracked", tracked), ("assoc", assoc)):
            got = getattr(self, name).cpu().numpy()
            bad = np.flatnonzero((got != want).any(1))
            assert not len(bad), f"{name}: {len(bad)} rows differ, first {bad[0]}: got {got[bad[0]].tolist()}, want {want[bad[0]].tolist()}"
        if self.R:
            want = tm.marks_of(tracked, COLOURS, 3, LABELS if self.R == 3 else None, 180, tm.pack_colour(9, 9, 9))
            assert np.array_equal(self.marks.cpu().numpy(), want), "marks"
        else:
            assert (self.marks.cpu().numpy() == GARBAGE).all()
        for name, whole in self.wholes.items():
            assert untouched(whole), f"{name}: a sentinel row was written"
        self.before = before
        return tracked, assoc


# (S, F, D, T, R, objects per stream, calls, a starting state with tracks all over the table)
SHAPES = [(1, 1, 1, 1, 0, None, 12, False), (1, 1, 5, 3, 1, None, 12, False), (3, 1, 5, 64, 3, None, 8, False),
          (1, 4, 5, 65, 1, None, 6, True), (3, 4, 70, 256, 3, 68, 6, True), (1, 1, 70, 65, 0, 68, 8, False),
          (3, 4, 1, 3, 3, None, 6, False), (1, 4, 70, 64, 1, 68, 6, False), (3, 1, 70, 1, 0, 30, 6, False),
          (1, 1, 5, 256, 3, None, 8, True), (3, 4, 5, 256, 0, None, 6, True), (3, 1, 1, 65, 1, None, 8, True)]


@pytest.mark.parametrize("S, Fr, D, T, R, count, calls, spread", SHAPES)
def test_every_call_of_a_sequence_equals_the_model(vali, gpu, S, Fr, D, T, R, count, calls, spread):
    rows = tc.scene(100 * S + 10 * Fr + D + T, S, Fr, D, calls, count)
    state = tc.spread_state(T, rows[0], S, Fr, D, T) if spread else None
    rig = Rig(vali, gpu, S, Fr, D, T, R, state)
    params = dict(iou_thr=0.3, new_thr=0.5, min_hits=2, max_age=3, momentum=0.5)
    seen = dict(births=0, matches=0, shown=0, deaths=0, misses=0)
    for r in rows:
        tracked, assoc = rig.step(r, **params)
        seen["births"] += int((assoc[:, 2] == 1).sum())
        seen["matches"] += int((assoc[:, 2] > 1).sum())
        seen["shown"] += int((tracked[:, 0] >= 0).sum())
        seen["misses"] += int((rig.m_tracks[:, tm.MISSES] > 0).sum())
        ids_before, ids_after = set(rig.before[:, 0].tolist()) - {0}, set(rig.m_tracks[:, 0].tolist())
        seen["deaths"] += len(ids_before - ids_after)
    assert seen["matches"] > 0 and seen["shown"] > 0, seen
    if D >= 5 and T >= 3:
        assert all(v > 0 for v in seen.values()), seen
    if spread and T == 256 and D == 70:
        assert state[0][192:256, 0].any() and state[0][64:128, 0].any()         # every register set holds tracks


@pytest.mark.parametrize("slots", [(0, 1), (63, 64), (5, 200), (64, 129), (191, 255)])
def test_equal_ious_go_to_the_lowest_slot_across_lanes_and_register_sets(vali, gpu, slots):
    """a box exactly between two tracks in the given slots: the lower slot gets it, wherever the two are held"""
    T, D = 256, 2
    tracks, clock = np.zeros((T, 16), np.int32), np.asarray([[9, 4, 0, 0]], np.int32)
    s9 = tm._bits(tm.F(0.9))
    # the higher slot holds the lower id and lies to the LEFT: neither the id nor the side decides
    tracks[slots[1]] = [3, 0, 100, 50, 40, 80, 0, 0, 4, 0, 4, s9, 0, 0, 0, 0]
    tracks[slots[0]] = [7, 0, 140, 50, 40, 80, 0, 0, 4, 0, 4, s9, 0, 0, 0, 0]
    rig = Rig(vali, gpu, 1, 1, D, T, 0, (tracks, clock))
    _, assoc = rig.step(tm.det_rows(1, D, {0: [(120, 50, 40, 80, 0, 0.9)]}), min_hits=1)
    assert assoc[0].tolist() == [7, slots[0], 5, 0]
    assert rig.m_tracks[slots[1], tm.MISSES] == 1 and rig.m_tracks[slots[0], tm.VX] == tm._bits(tm.F(-10.0))


@pytest.mark.parametrize("S, Fr, D, T, R, agnostic", [(1, 1, 70, 256, 3, False), (3, 4, 5, 65, 1, True), (3, 1, 70, 3, 0, False),
                                                      (1, 4, 70, 64, 0, True)])
def test_arbitrary_int32_values_are_handled_as_the_model_handles_them(vali, gpu, S, Fr, D, T, R, agnostic):
    """every value of dets, tracks and clock is the caller's: extreme boxes, NaN and infinite velocities, counters of any
    size.  Three calls, the state of each the foreign outcome of the last; nothing outside the outputs is written."""
    rig = None
    valid = live = cands = 0
    for call in range(3):
        dets, tracks, clock = tc.foreign(1000 * call + S + Fr + D + T, S, Fr, D, T)
        if rig is None:
            rig = Rig(vali, gpu, S, Fr, D, T, R, (tracks, clock))
            live = int(((tracks[:, 0] >= 1) & (tracks[:, 4] >= 1) & (tracks[:, 5] >= 1)).sum())
        frame = np.repeat(np.arange(S * Fr), D)
        valid += int(((dets[:, 0] == frame) & (dets[:, 3] >= 1) & (dets[:, 4] >= 1)).sum())
        _, assoc = rig.step(dets, iou_thr=0.05, new_thr=0.5, min_hits=2, max_age=5, momentum=0.75, class_agnostic=agnostic)
        cands += int((assoc[:, 2] > 1).sum())
    assert valid > 3 and live > 0 and cands > 0        # the arithmetic met real candidates, not only refusals


def test_one_call_with_four_frames_equals_four_calls_with_one(vali, gpu):
    S, D, T = 3, 5, 65
    rows4 = tc.scene(77, S, 4, D, 3)
    big, small = Rig(vali, gpu, S, 4, D, T, 0), Rig(vali, gpu, S, 1, D, T, 0)
    params = dict(min_hits=2, max_age=2)
    for rows in rows4:
        big.step(rows, **params)
        for f in range(4):
            one = np.concatenate([rows[(s * 4 + f) * D:(s * 4 + f + 1) * D] for s in range(S)]).copy()
            for s in range(S):
                part = one[s * D:(s + 1) * D]
                part[part[:, 0] == s * 4 + f, 0] = s
            small.step(one, **params)
        for name in ("tracks", "clock"):
            assert torch.equal(getattr(big, name), getattr(small, name)), name
    assert big.clock.cpu().numpy()[:, 1].tolist() == [12] * S and big.m_tracks.any()


def test_a_captured_call_replayed_after_dets_was_rewritten_advances_the_state(vali, gpu):
    from vali_amd._native import shim

    S, Fr, D, T = 3, 1, 5, 64
    stream = shim.stream_create(gpu)
    rig = Rig(vali, gpu, S, Fr, D, T, 3, stream=stream)
    rig.style.device(gpu, stream)                  # host colours and labels are uploaded before the capture
    params = dict(iou_thr=0.3, new_thr=0.5, min_hits=2, max_age=3, momentum=0.5)
    rows = tc.scene(5, S, Fr, D, 7)
    cap = vali.StreamCapture(stream, gpu)
    rig.load(rows[0])
    state = rig.tracks.clone(), rig.clock.clone()
    with cap:
        assert rig.task.RunAsync(rig.batch, style=rig.style, **params)[0]
    cap.Keep(rig.batch)
    rig.tracks.copy_(state[0]), rig.clock.copy_(state[1])          # whether the capture ran the call or not: start over
    shown = 0
    for r in rows:
        rig.load(r)
        cap.Launch()
        shim.stream_sync(gpu, stream)
        tracked, _ = rig.check(r, **params)
        shown += int((tracked[:, 0] >= 0).sum())
    assert shown > 10 and rig.m_clock[:, 1].tolist() == [7] * S


def test_run_refuses_what_prepare_could_not_see(vali, gpu):
    rig = Rig(vali, gpu, 1, 1, 5, 3, 1)
    with pytest.raises(ValueError, match="momentum"):
        rig.task.Run(rig.batch, momentum=2.0, style=rig.style)
    with pytest.raises(ValueError, match="style"):
        rig.task.Run(rig.batch)
    with pytest.raises(ValueError, match="tracks: the tensor must be 16-byte aligned"):
        flat = torch.zeros((3 * 16 + 2,), dtype=torch.int32, device=f"cuda:{gpu}")
        rig.task.Prepare(rig.dets, flat[2:].view(3, 16), rig.clock, rig.tracked, max_det=5, max_tracks=3)
    assert rig.task.Run(rig.batch, style=rig.style)[0]
