"""Frames that hold the WHOLE value domain of an 8-bit colour kernel, and the means to compare on them.

An 8-bit colour stage maps a triple of bytes to a triple of bytes (or floats): 2^24 inputs, which a 4096 x 4096 frame
holds exactly once each.  One launch on such a frame turns a sampled check of an instantiation into a proof.

    nv12_cube()    (6144, 4096) uint8: every (Y, U, V).  With c the row-major number of a chroma sample (2048 x 2048 of
                   them), (U, V) = ((c >> 6) & 255, c >> 14) and the four luma samples of c are 4 * (c & 63) + 2 * dy + dx
    rgb_cube()     (4096, 4096, 3) uint8: pixel k = (k >> 16, (k >> 8) & 255, k & 255); its three channels read as planes
                   are the YUV444 / RGB_PLANAR cube, the planes of nv12_cube() de-interleaved the YUV420 cube
    ragged twins   the same frames with two more columns (copies of columns 0 and 1): 4098 wide, so every row takes the
                   kernels' byte-granular instantiation, not only a tail
    p16_frame()    (384, 512) uint16, a 512 x 256 P10 / P12 frame: luma holds all 65,536 sample values twice, the
                   interleaved chroma plane each of them once -- low bits set too

Everything is built once per session (memo) and must be treated as read-only.  Comparisons are on raw bytes; a mismatch
is reported as a count and the first few (input triple -> got, want), never as the repr of a 48 MB array.
"""
from collections import OrderedDict

import numpy as np

SIDE = 4096            # a cube frame is SIDE x SIDE pixels: 2^24
RAGGED = SIDE + 2      # width of a ragged twin
P16_W, P16_H = 512, 256

# ---- memo -------------------------------------------------------------------------------------------------------------
# Cubes and reference results are large (a float32 reference of one frame is 192 MiB), so the memo is bounded: the least
# recently used entries leave once the total passes MEMO_BYTES.  The GPU tests order their cases so that cases which
# share a reference are neighbours.
MEMO_BYTES = 1 << 30
_memo = OrderedDict()


def _nbytes(v):
    if isinstance(v, (tuple, list)):
        return sum(_nbytes(x) for x in v)
    return int(getattr(v, "nbytes", 0))


def forget():
    """drop everything the memo holds (the GPU test module calls it when its last case has run)"""
    _memo.clear()


def memo(key, make):
    """make() once per key; the value is shared, so nobody writes to it"""
    if key in _memo:
        _memo.move_to_end(key)
        return _memo[key]
    v = make()
    for a in (v if isinstance(v, (tuple, list)) else (v,)):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _memo[key] = v
    total = sum(_nbytes(x) for x in _memo.values())
    while total > MEMO_BYTES and len(_memo) > 1:
        _, old = _memo.popitem(last=False)
        total -= _nbytes(old)
    return v


# ---- the cubes --------------------------------------------------------------------------------------------------------
def _widen(a):
    """the ragged twin: two more columns, copies of columns 0 and 1"""
    return np.ascontiguousarray(np.concatenate([a, a[:, :2]], axis=1))


def _nv12_cube():
    half = SIDE // 2
    c = np.arange(half * half, dtype=np.uint32).reshape(half, half)
    a = np.empty((SIDE * 3 // 2, SIDE), np.uint8)
    y0 = (4 * (c & 63)).astype(np.uint8)
    for dy in (0, 1):
        for dx in (0, 1):
            a[dy:SIDE:2, dx::2] = y0 + np.uint8(2 * dy + dx)
    a[SIDE:, 0::2] = ((c >> 6) & 255).astype(np.uint8)
    a[SIDE:, 1::2] = (c >> 14).astype(np.uint8)
    return a


def nv12_cube(ragged=False):
    """(6144, 4096) uint8, or (6144, 4098) for the ragged twin: luma rows, then interleaved chroma rows"""
    if ragged:
        return memo("nv12_cube_ragged", lambda: _widen(nv12_cube()))
    return memo("nv12_cube", _nv12_cube)


def _rgb_cube():
    k = np.arange(SIDE * SIDE, dtype=np.uint32).reshape(SIDE, SIDE)
    return np.stack([(k >> 16).astype(np.uint8), ((k >> 8) & 255).astype(np.uint8), (k & 255).astype(np.uint8)], -1)


def rgb_cube(ragged=False):
    """(4096, 4096, 3) uint8, or (4096, 4098, 3) for the ragged twin"""
    if ragged:
        return memo("rgb_cube_ragged", lambda: _widen(rgb_cube()))
    return memo("rgb_cube", _rgb_cube)


def cube_width(ragged):
    return RAGGED if ragged else SIDE


def yuv420_planes(nv12):
    """the planes (Y, U, V) of an NV12 frame given as (H * 3 / 2, W)"""
    h = nv12.shape[0] * 2 // 3
    return nv12[:h], nv12[h:, 0::2], nv12[h:, 1::2]


def host_image(fmt, ragged=False):
    """the cube as the flat, tightly packed host image of an 8-bit source format (Surface.HostSize layout).  BGR takes
    the bytes of rgb_cube() as they are: every (b, g, r) occurs once, as every (r, g, b) does"""
    def make():
        if fmt == "NV12":
            return nv12_cube(ragged).reshape(-1)
        if fmt == "YUV420":
            return np.concatenate([p.reshape(-1) for p in yuv420_planes(nv12_cube(ragged))])
        if fmt in ("RGB", "BGR"):
            return rgb_cube(ragged).reshape(-1)
        assert fmt in ("YUV444", "RGB_PLANAR"), fmt
        return np.ascontiguousarray(rgb_cube(ragged).transpose(2, 0, 1)).reshape(-1)
    if fmt in ("NV12", "RGB", "BGR"):
        return make()                    # views of the cubes themselves
    return memo(("host_image", fmt, ragged), make)


def _p16_frame():
    n = P16_W * P16_H
    a = np.empty((P16_H * 3 // 2, P16_W), np.uint16)
    k = np.arange(n, dtype=np.uint32)
    a[:P16_H] = (k & 0xffff).astype(np.uint16).reshape(P16_H, P16_W)
    # an odd multiplier is a bijection of the 16-bit values: neighbours in memory are unrelated samples
    a[P16_H:] = ((k[:n // 2] * 40503) & 0xffff).astype(np.uint16).reshape(P16_H // 2, P16_W)
    return a


def p16_frame():
    """(384, 512) uint16: a 512 x 256 P10 / P12 host frame (MSB-aligned samples are a subset of what it holds)"""
    return memo("p16_frame", _p16_frame)


# ---- properties (the host test asserts them) --------------------------------------------------------------------------
def triple_counts(a, b, c):
    """occurrences of each of the 2^24 triples (a, b, c) of three equally shaped uint8 arrays, by bincount"""
    key = (a.astype(np.uint32).reshape(-1) << 16) | (b.astype(np.uint32).reshape(-1) << 8) | c.reshape(-1)
    return np.bincount(key, minlength=1 << 24)


def nv12_triples(nv12):
    """(Y, U, V) per luma sample of an NV12 frame, chroma replicated over its 2 x 2 block"""
    y, u, v = yuv420_planes(nv12)
    return y, np.repeat(np.repeat(u, 2, 0), 2, 1), np.repeat(np.repeat(v, 2, 0), 2, 1)


# ---- where an element came from ---------------------------------------------------------------------------------------
def locate(fmt, w, h, i):
    """element i of a flat host image of `fmt` (bytes, or float32 elements) -> (x, y, channel name): the luma pixel it
    belongs to -- for a 4:2:0 chroma sample the top-left pixel of its 2 x 2 block"""
    i = int(i)
    if fmt in ("RGB", "BGR", "RGB_32F"):
        names = "BGR" if fmt == "BGR" else "RGB"
        return (i % (3 * w)) // 3, i // (3 * w), names[i % 3]
    if fmt in ("RGB_PLANAR", "RGB_32F_PLANAR", "YUV444", "Y"):
        names = "YUV" if fmt in ("YUV444", "Y") else "RGB"
        p, r = divmod(i, w * h)
        return r % w, r // w, names[p]
    if i < w * h:
        return i % w, i // w, "Y"
    r = i - w * h
    if fmt == "NV12":
        return (r % w) & ~1, 2 * (r // w), "UV"[r & 1]
    assert fmt == "YUV420", fmt
    cw, cn = w // 2, (w // 2) * (h // 2)
    p, r = divmod(r, cn)
    return 2 * (r % cw), 2 * (r // cw), "UV"[p]


def nv12_triple_at(nv12):
    h = nv12.shape[0] * 2 // 3
    return lambda x, y: (int(nv12[y, x]), int(nv12[h + y // 2, x & ~1]), int(nv12[h + y // 2, (x & ~1) + 1]))


def rgb_triple_at(px):
    return lambda x, y: tuple(int(v) for v in px[y, x])


def differences(got, want, describe, limit=6):
    """None when the two arrays hold the same bytes, else a short report: how many elements differ and the first few as
    `describe(i)` -> got, want.  Arrays are compared as flat arrays of their own element size"""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    if got.shape != want.shape or got.dtype.itemsize != want.dtype.itemsize:
        return f"shapes or element sizes differ: {got.shape} {got.dtype} and {want.shape} {want.dtype}"
    view = {1: np.uint8, 2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    gb, wb = got.view(view), want.view(view)
    if np.array_equal(gb, wb):
        return None
    bad = np.flatnonzero(gb != wb)
    def show(a, b, i):
        return f"{a[i].item()!r}" if a.dtype.kind in "ui" else f"{float(a[i])!r} (bits {int(b[i]):#x})"
    first = "; ".join(f"{describe(i)} -> got {show(got, gb, i)}, want {show(want, wb, i)}" for i in bad[:limit])
    return f"{bad.size} of {got.size} elements differ; first: {first}"


def assert_same(got, want, fmt, w, h, triple_at, what):
    """raw-byte equality of two flat host images of `fmt`; the message names input triples, not arrays"""
    def describe(i):
        x, y, ch = locate(fmt, w, h, i)
        return f"{triple_at(x, y)} at ({x}, {y}) {ch}"
    report = differences(got, want, describe)
    assert report is None, f"{what}: {report}"
