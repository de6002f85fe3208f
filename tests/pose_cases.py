"""The fixtures the pose tests share (tests/test_pose_host.py checks their conditions on the CPU; the GPU tests and the C
client draw them): the two frames, records and dets rows of tests/mask_cases.py -- 96 x 80 and 70 x 50: more than one tile,
partial tiles, a ragged right edge; D = 4 rows each, K = 12 candidates -- with P = 5 keypoints a candidate and a 6-limb
table.

  frame 0   a letterbox into the 64 x 64 network input: 96 x 80 -> 64 x 53 at (0, 5)
  frame 1   a zoomed crop with a nonzero origin: (10, 6, 18, 15) -> (2, 3, 60, 50); most keypoints lie outside the
            placement in network coordinates, so that the skeletons spread over the whole frame

Keypoints are chosen as frame pixels and taken back through the record, so every candidate of both frames has a skeleton
on its frame.  In every candidate with an odd k keypoint 4 is below the threshold.
"""
import numpy as np

import mask_cases as mc

SIZES, NET, D, K, RECTS, RECTS_DST_W_0 = mc.SIZES, mc.NET, mc.D, mc.K, mc.RECTS, mc.RECTS_DST_W_0
PLACEMENTS, SKIPS, SKIPS_PAINTED = mc.PLACEMENTS, mc.SKIPS, mc.SKIPS_PAINTED
P = 5
LIMBS = ((0, 1), (1, 2), (2, 3), (3, 4), (0, 2), (4, 1))
THR = 0.5
pack_colour, quantise = mc.pack_colour, mc.quantise

LIMB_COLOURS = [pack_colour(230, 40, 40, 200), pack_colour(40, 200, 60, 90), pack_colour(30, 60, 240, 255),
                pack_colour(250, 220, 20, 140)]
JOINT_COLOURS = [pack_colour(255, 255, 255, 230), pack_colour(10, 10, 10, 120), pack_colour(200, 30, 220, 255)]


def to_net(px, py, rect):
    """the network coordinates whose mapping lands in the middle of frame pixel (px, py)"""
    sx, sy, sw, sh, dx, dy, dw, dh = rect
    return (px + 0.5 - sx) * dw / sw + dx, (py + 0.5 - sy) * dh / sh + dy


def kpts(p=P, dtype="float32", seed=0, kdim=3, n=2, k=K, sizes=SIZES, rects=RECTS):
    """(n, k, p, kdim): keypoints at random pixels of their frame, 4 pixels from its edges, confidences in 0.55 .. 1; with
    p = P and seed = 0, candidate 3 of frame 0 and candidate 5 of frame 1 hold limbs that cross a tile corner"""
    rng = np.random.default_rng(3000 * seed + p)
    out = np.zeros((n, k, p, 3), np.float64)
    for i in range(n):
        w, h = sizes[i]
        px = rng.integers(4, w - 4, (k, p))
        py = rng.integers(4, h - 4, (k, p))
        if p == P and seed == 0:
            if i == 0:      # through the corner (64, 64) of four tiles, and along the tile edge y = 64
                px[3], py[3] = (50, 78, 60, 90, 20), (50, 78, 64, 64, 63)
            else:           # through (64, 0) .. (64, 50): the ragged last tile column
                px[5], py[5] = (58, 68, 66, 40, 63), (10, 40, 5, 30, 45)
        out[i, :, :, 0], out[i, :, :, 1] = to_net(px, py, rects[i])
        out[i, :, :, 2] = rng.uniform(0.55, 1.0, (k, p))
        if p >= 5:
            out[i, 1::2, 4, 2] = 0.3
    return quantise(out[..., :kdim].astype(np.float32), dtype)


def odd_kpts(dtype="float32"):
    """... with, in every candidate of both frames: a NaN confidence in keypoint 0, a NaN y in keypoint 2 and a confidence
    of exactly THR in keypoint 3 of even candidates (1 and 4 stay visible: limb (4, 1)); an infinite x in keypoint 1 and
    a -inf y in keypoint 3 of odd ones, whose keypoint 4 is below THR already (0 and 2 stay visible: limb (0, 2))"""
    a = kpts(P, dtype).copy()
    a[:, 0::2, 0, 2] = np.nan
    a[:, 0::2, 2, 1] = np.nan
    a[:, 0::2, 3, 2] = THR
    a[:, 1::2, 1, 0] = np.inf
    a[:, 1::2, 3, 1] = -np.inf
    return a


# frame 0 maps x by exactly 1.5 and y by 80 / 53 from 5: keypoints 0 and 1 of these candidates land at the ends of the
# range a visible keypoint has, keypoint 2 one pixel beyond it (invisible)
FAR_K = (3, 7, 0, 11)       # the candidates of PLACEMENTS[:4]


def far_kpts():
    """float32 only.  Candidate 3: keypoint 0 at X = -65536; 7: keypoint 1 at X = 131071; 0: keypoint 0 at Y = -65536;
    11: keypoint 1 at Y = 131071; keypoint 2 of each is beyond the range on that side and keeps a confidence of 0.9"""
    a = kpts(P, "float32").copy()
    ys = 80.0 / 53.0
    a[0, 3, 0, 0], a[0, 3, 2, 0] = -65535.5 / 1.5, -65537.5 / 1.5
    a[0, 7, 1, 0], a[0, 7, 2, 0] = 131071.5 / 1.5, 131073.5 / 1.5
    a[0, 0, 0, 1], a[0, 0, 2, 1] = 5 - 65535.5 / ys, 5 - 65537.5 / ys
    a[0, 11, 1, 1], a[0, 11, 2, 1] = 5 + 131071.5 / ys, 5 + 131073.5 / ys
    a[0, list(FAR_K), 2, 2] = 0.9
    a[0, list(FAR_K), 4, 2] = 0.9
    return a


def noise_frames(fmt, seed=0):
    return mc.noise_frames(fmt, seed)
