"""The fixtures the instance-mask tests share (tests/test_mask_host.py checks their conditions on the CPU; the GPU tests
and the C client paint them): two frames, 96 x 80 and 70 x 50 -- more than one tile, partial tiles, a ragged right edge --
with D = 4 rows each and K = 12 candidates.

  frame 0   a letterbox into the 64 x 64 network input: 96 x 80 -> 64 x 53 at (0, 5); with 16 x 16 prototypes a prototype
            pixel spans 6 frame pixels (24 x 20: 4)
  frame 1   a zoomed crop with a nonzero origin: (10, 6, 18, 15) -> (2, 3, 60, 50); the frame is sampled more coarsely than
            the prototypes (16 x 16: 0.83 prototype pixels a frame pixel, 24 x 20: 1.25)
"""
import numpy as np

SIZES = [(96, 80), (70, 50)]
NET = (64, 64)
D, K = 4, 12
RECTS = [(0, 0, 96, 80, 0, 5, 64, 53), (10, 6, 18, 15, 2, 3, 60, 50)]
RECTS_DST_W_0 = [RECTS[0], (10, 6, 18, 15, 2, 3, 0, 50)]
PROTO_SIZES = [(16, 16), (24, 20)]           # (Wp, Hp)
MS = (1, 5, 32, 64)
I32_MIN, I32_MAX = -2**31, 2**31 - 1


def pack_colour(r, g, b, a=255):
    v = a << 24 | r << 16 | g << 8 | b
    return v - (1 << 32) if v >= 1 << 31 else v


COLOURS = [pack_colour(230, 40, 40, 200), pack_colour(40, 200, 60, 90), pack_colour(30, 60, 240, 255)]


def quantise(a, dtype):
    """float32 values that a float16 / bfloat16 tensor holds exactly"""
    a = np.asarray(a, np.float32)
    if dtype == "float16":
        return a.astype(np.float16).astype(np.float32)
    if dtype == "bfloat16":
        b = a.view(np.uint32).astype(np.uint64)
        b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16 << 16).astype(np.uint32)      # round to nearest even
        return b.view(np.float32)
    return a


def protos(m, wp, hp, dtype="float32", n=2, seed=0):
    """(n, m, hp, wp): sinusoids of 1.5 to 4 periods across the plane at random phases"""
    rng = np.random.default_rng(1000 * seed + 10 * m + wp)
    y, x = np.mgrid[0:hp, 0:wp]
    out = np.zeros((n, m, hp, wp), np.float32)
    for i in range(n):
        for j in range(m):
            fx, fy = rng.uniform(1.5, 4.0, 2) * rng.choice([-1, 1], 2)
            out[i, j] = np.sin(2 * np.pi * (fx * (x + 0.5) / wp + fy * (y + 0.5) / hp) + rng.uniform(0, 2 * np.pi))
    return quantise(out, dtype)


def coeffs(m, dtype="float32", n=2, seed=0):
    """(n, K, m) normal coefficients"""
    rng = np.random.default_rng(2000 * seed + m)
    return quantise(rng.standard_normal((n, K, m)).astype(np.float32), dtype)


def nonfinite_coeffs(m, dtype="float32"):
    """... with a NaN, a +inf and a -inf in the candidates 1, 2 and 3 of both frames (and 4: all three, if m allows)"""
    c = coeffs(m, dtype).copy()
    for i in range(c.shape[0]):
        c[i, 1, 0], c[i, 2, m // 2], c[i, 3, m - 1] = np.nan, np.inf, -np.inf
        c[i, 4, 0] = np.inf
        c[i, 4, m - 1] = -np.inf if m > 1 else np.inf
    return c


def row(frame, x, y, w, h, cls, k):
    return (frame, x, y, w, h, cls, 0x3F000000, k)


# every row is painted: an upsampled box, two overlapping masks (the order shows with alpha), odd coordinates, a box that
# hangs over every edge of its frame
PLACEMENTS = [
    row(0, 5, 7, 60, 50, 0, 3), row(0, 30, 20, 50, 45, 1, 7), row(0, 11, 13, 41, 37, 2, 0), row(0, -5, -4, 110, 90, 4, 11),
    row(1, 3, 5, 40, 30, 0, 5), row(1, 20, 10, 45, 35, 1, 2), row(1, 33, 11, 25, 29, 5, 9), row(1, -10, -10, 100, 80, -1, 1),
]
# rows 1 and 6 are painted; the others must be skipped: frame -1, the frame field of another slot, k = K, w = 0, a box that
# ends at -1 from x = -2^31, h = 0 ... and two with int32 extremes that do reach their frames
SKIPS = [
    row(-1, 5, 7, 60, 50, 0, 3), row(0, I32_MIN + 45, 3, I32_MAX, I32_MAX, 1, 4), row(1, 5, 7, 60, 50, 0, 3), row(0, 5, 7, 60, 50, 0, K),
    row(1, 3, 5, 0, 30, 0, 5), row(1, I32_MIN, 5, I32_MAX, 30, 1, 2), row(1, 8, I32_MIN + 40, I32_MAX, I32_MAX, 2, 6), row(1, 3, 5, 40, 30, 1, -1),
]
SKIPS_PAINTED = {1, 6}
# candidates 1 .. 4 (nonfinite_coeffs) and a finite one under and over them
NONFINITE = [
    row(0, 5, 7, 60, 50, 0, 0), row(0, 30, 20, 50, 45, 1, 1), row(0, 11, 13, 41, 37, 2, 2), row(0, 2, 30, 90, 45, 0, 3),
    row(1, 3, 5, 40, 30, 0, 4), row(1, 20, 10, 45, 35, 1, 1), row(1, 33, 11, 25, 29, 2, 3), row(1, 0, 0, 70, 50, 1, 5),
]


def noise_frames(fmt, seed=0):
    import annotate_model as am

    return [am.noise_frame(fmt, w, h, 7000 + 10 * seed + i) for i, (w, h) in enumerate(SIZES)]
