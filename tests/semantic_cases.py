"""The fixtures the semantic-map tests share (tests/test_semantic_host.py checks their conditions on the CPU; the GPU tests
and the C client paint them).  The geometry is that of tests/mask_cases.py: two frames, 96 x 80 and 70 x 50 -- more than
one tile, partial tiles, a ragged right edge -- behind a 64 x 64 network input.

  frame 0   a letterbox: 96 x 80 -> 64 x 53 at (0, 5); the whole frame is the region and is upsampled from the logits
  frame 1   a zoomed crop with a non-zero, non-even origin: (10, 6, 18, 15) -> (2, 3, 60, 50); the region is smaller than
            the frame and is sampled more coarsely than fine logits: 160 x 120 logits put 150 x 94 cells under its 18 x 15
            pixels, more than the kernel's stage holds
"""
import numpy as np

import mask_cases as mc

SIZES = mc.SIZES
NET = mc.NET
RECTS = mc.RECTS
RECTS_DST_W_0 = mc.RECTS_DST_W_0
I32_MIN, I32_MAX = mc.I32_MIN, mc.I32_MAX
# (Ws, Hs): the first two are staged in LDS everywhere, the third is read directly on frame 1; the last two sit either
# side of the switch-over on frame 1 (tests/test_semantic_host.py: 8175 and 8325 cells against a stage of 8192)
LOGIT_SIZES = [(16, 16), (24, 20), (160, 120)]
SWITCH_SIZES = [(120, 100), (122, 100)]
CS = (1, 2, 19, 255)
# frame 0 is reached from -2^31 + 45 (columns 0 .. 43) with a width that overflows int32 past x = 8 on frame 1;
# the second set reaches neither frame: it ends at -1, and it begins at the frame's height
EXTREME_RECTS = [(I32_MIN + 45, 3, I32_MAX, I32_MAX, 0, 5, 64, 53), (8, I32_MIN + 40, I32_MAX, I32_MAX, 2, 3, 60, 50)]
EXTREME_RECTS_MISS = [(I32_MIN, 5, I32_MAX, 30, 0, 5, 64, 53), (10, 50, I32_MAX, I32_MAX, 2, 3, 60, 50)]

pack_colour = mc.pack_colour
quantise = mc.quantise


def palette(n, seed=0):
    """n random colours with an alpha of 60 .. 255"""
    rng = np.random.default_rng(4000 + seed)
    rgb, alpha = rng.integers(0, 256, (n, 3)), rng.integers(60, 256, n)
    return [pack_colour(int(r), int(g), int(b), int(a)) for (r, g, b), a in zip(rgb, alpha)]


# alpha 0, 90 and 255 (alpha=None: class 0 stays untouched)
PALETTE_OWN_ALPHA = [pack_colour(230, 40, 40, 0), pack_colour(40, 200, 60, 90), pack_colour(30, 60, 240, 255)]


def logits(c, ws, hs, dtype="float32", n=2, seed=0):
    """(n, c, hs, ws): per class a sinusoid of amplitude 4 and 0.5 to 2 periods across the plane at a random phase"""
    rng = np.random.default_rng(3000 * seed + 10 * c + ws)
    y, x = np.mgrid[0:hs, 0:ws]
    out = np.zeros((n, c, hs, ws), np.float32)
    for i in range(n):
        for j in range(c):
            fx, fy = rng.uniform(0.5, 2.0, 2) * rng.choice([-1, 1], 2)
            out[i, j] = 4.0 * np.sin(2 * np.pi * (fx * (x + 0.5) / ws + fy * (y + 0.5) / hs) + rng.uniform(0, 2 * np.pi))
    return quantise(out, dtype)


def nonfinite_logits(c, ws, hs, dtype="float32"):
    """... with a NaN plane, a +inf plane and a -inf plane on frame 0 (classes 1, 2 and c - 1), and on frame 1 NaN and
    infinities sprinkled over single cells of every class"""
    assert c >= 4
    out = logits(c, ws, hs, dtype, seed=5).copy()
    out[0, 1], out[0, c - 1] = np.nan, -np.inf
    out[0, 2, : hs // 2] = np.inf
    rng = np.random.default_rng(77)
    for v in (np.nan, np.inf, -np.inf):
        sel = rng.random(out[1].shape) < 0.03
        out[1][sel] = v
    return out


def noise_frames(fmt, seed=0):
    return mc.noise_frames(fmt, seed)
