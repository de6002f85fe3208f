"""Seeded scenes for the tracker's tests: sequences of PyDetectionSelector rows in which objects move, are missed for a
frame or several, appear, leave, share classes or not, and in which a box now and then lies exactly between two tracks
(equal IoUs); starting states with tracks in slots all over the table; and rows, states and clocks of arbitrary int32
values.  The GPU tests and the C ABI test read them; nothing here needs a device."""
import numpy as np

import track_model as tm

F = np.float32
SCORES = (0.3, 0.45, 0.6, 0.75, 0.9)       # 0.3 and 0.45 are below the default new_thr


def _objects(rng, count):
    """(x, y, w, h, class, vx, vy, first frame, last frame) per object"""
    objs = []
    for o in range(count):
        x, y = int(rng.integers(0, 1500)), int(rng.integers(0, 800))
        w, h = int(rng.integers(30, 90)), int(rng.integers(30, 90))
        first = 0 if rng.random() < 0.7 else int(rng.integers(1, 12))
        last = 10 ** 6 if rng.random() < 0.7 else first + int(rng.integers(3, 20))
        objs.append([x, y, w, h, int(rng.integers(0, 3)), int(rng.integers(-9, 10)), int(rng.integers(-6, 7)), first, last])
    return objs


def scene(seed, S, Fr, D, calls, count=None):
    """`calls` arrays of (S * Fr * D, 8) int32 rows.  Stream s has min(count or 6, D) objects, `count` of them when
    given.  A few rows are no detections at all (a foreign frame value, w = 0) in the middle of a frame's rows."""
    rng = np.random.default_rng(seed)
    count = min(count or 6, D)
    objs = [_objects(rng, count) for _ in range(S)]
    twin = [(int(rng.integers(0, 1000)), 850, 40, 80, 1) for _ in range(S)]     # two still boxes side by side, below the rest
    out = []
    for c in range(calls):
        boxes = {}
        for s in range(S):
            for f in range(Fr):
                t = c * Fr + f
                items = []
                for (x, y, w, h, cls, vx, vy, first, last) in objs[s]:
                    if not first <= t <= last or rng.random() < 0.2:
                        continue
                    items.append((x + vx * t, y + vy * t, w, h, cls, float(rng.choice(SCORES))))
                if D >= 3:
                    tx, ty, tw, th, tc = twin[s]
                    if t % 4 == 3:      # one box exactly between the two: equal IoUs
                        items.append((tx + tw // 2, ty, tw, th, tc, 0.9))
                    else:
                        items += [(tx, ty, tw, th, tc, 0.9), (tx + tw, ty, tw, th, tc, 0.75)]
                boxes[s * Fr + f] = items[:D]
        rows = tm.det_rows(S * Fr, D, boxes)
        # rows that are no detections, where detections are expected
        for i in range(S * Fr):
            if D >= 4 and rng.random() < 0.5:
                r = i * D + int(rng.integers(0, D))
                if rng.random() < 0.5:
                    rows[r, 0] = i + 1          # another frame's row
                else:
                    rows[r, 3] = 0              # no width
        out.append(rows)
    return out


def spread_state(seed, first_rows, S, Fr, D, T):
    """a starting state whose tracks sit in slots all over the table: one confirmed track under every row of each
    stream's first frame, so that lanes and register sets far from slot 0 take part from the first call on"""
    rng = np.random.default_rng(seed)
    tracks, clock = np.zeros((S * T, 16), np.int32), np.zeros((S, 4), np.int32)
    for s in range(S):
        rows = first_rows[s * Fr * D:s * Fr * D + D]
        rows = rows[rows[:, 0] == s * Fr]
        slots = np.sort(rng.permutation(T)[:min(len(rows), T)])
        for q, (slot, row) in enumerate(zip(slots, rows)):
            vx, vy = F(rng.integers(-8, 9)) * F(0.5), F(rng.integers(-4, 5)) * F(0.25)
            tracks[s * T + slot] = [q + 1, row[5], row[1], row[2], row[3], row[4], tm._bits(vx), tm._bits(vy),
                                    int(rng.integers(1, 6)), int(rng.integers(0, 3)), 9, row[6], row[7], 0, 0, 0]
        clock[s] = len(slots) + 1, 9, 0, 0
    return tracks, clock


_EXTREME = np.asarray([0, 1, -1, 2, 2**31 - 1, -(2**31), 2**30, 2**30 + 1, 2**24 + 1, 65535, -65536, 2**31 - 2], np.int64)
_FLOATS = np.asarray([0x7fc00000, 0x7f800000, 0xff800000, 0x7f7fffff, 0xff7fffff, 0x00000001, 0x80000001, 0x00800000,
                      0x3f800000, 0xbf000000, 0x41400000, 0x7fa00001, 0xffc12345], np.uint32).view(np.int32).astype(np.int64)


def _mixed(rng, shape, small):
    """int32 values: any 32 bits, extremes and values of the size `small`, a third each"""
    pick = rng.integers(0, 3, shape)
    anyv = rng.integers(-(2**31), 2**31, shape)
    ext = _EXTREME[rng.integers(0, len(_EXTREME), shape)]
    sm = rng.integers(-small // 8, small, shape)
    return np.where(pick == 0, anyv, np.where(pick == 1, ext, sm))


def foreign(seed, S, Fr, D, T):
    """(dets, tracks, clock) of arbitrary int32 values, shaped so that a good part of the rows is valid and of the tracks
    live, near each other and of few classes -- the checks are passed and the arithmetic sees the values -- with NaN,
    infinite, huge, tiny and denormal velocity bits and every kind of counter"""
    rng = np.random.default_rng(seed)
    n = S * Fr
    dets = _mixed(rng, (n * D, 8), 300)
    frame = np.repeat(np.arange(n), D)
    dets[:, 0] = np.where(rng.random(n * D) < 0.7, frame, dets[:, 0])
    dets[:, 5] = np.where(rng.random(n * D) < 0.7, rng.integers(0, 2, n * D), dets[:, 5])
    near = lambda rows: np.concatenate([rng.integers(0, 200, (rows, 2)), rng.integers(50, 250, (rows, 2))], 1)
    dets[:, 1:5] = np.where(rng.random((n * D, 4)) < 0.6, near(n * D), dets[:, 1:5])
    score = rng.random(n * D).astype(F).view(np.int32).astype(np.int64)
    dets[:, 6] = np.where(rng.random(n * D) < 0.6, score, np.where(rng.random(n * D) < 0.5, _FLOATS[rng.integers(0, len(_FLOATS), n * D)], dets[:, 6]))
    tracks = _mixed(rng, (S * T, 16), 300)
    tracks[:, 0] = np.where(rng.random(S * T) < 0.7, rng.integers(1, 2**31, S * T), tracks[:, 0])
    tracks[:, 1] = np.where(rng.random(S * T) < 0.7, rng.integers(0, 2, S * T), tracks[:, 1])
    tracks[:, 2:6] = np.where(rng.random((S * T, 4)) < 0.6, near(S * T), tracks[:, 2:6])
    vel = (rng.standard_normal((S * T, 2)) * 6).astype(F).view(np.int32).astype(np.int64)
    odd = _FLOATS[rng.integers(0, len(_FLOATS), (S * T, 2))]
    tracks[:, 6:8] = np.where(rng.random((S * T, 2)) < 0.5, vel, np.where(rng.random((S * T, 2)) < 0.6, odd, tracks[:, 6:8]))
    tracks[:, 8:11] = np.where(rng.random((S * T, 3)) < 0.5, rng.integers(0, 6, (S * T, 3)), tracks[:, 8:11])
    clock = _mixed(rng, (S, 4), 100)
    to32 = lambda a: a.astype(np.uint32).view(np.int32)
    return to32(dets), to32(tracks), to32(clock)
