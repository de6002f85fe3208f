"""Host images, quantisation tables and restart intervals that drive the JPEG encoder (vali_jpeg_encode_batch) through
every Huffman symbol, through its colour conversion and onto the byte-level edges of its stuffing and assembly loops.
Everything is built from formulas and seeds; tests/test_jpeg_params_host.py proves on the CPU, with the model of
tests/jpeg_model.py, that each input has the property it is named for, and tests/test_gpu_jpeg_params.py encodes them.

`python tests/jpeg_encoder_inputs.py` repeats the seeded search behind BOUNDARY_SEEDS and prints the seeds it finds.
"""
from __future__ import annotations

import functools

import numpy as np

import jpeg_model as jm


# ---- tables ------------------------------------------------------------------------------------------------------------
def flat_table(v):
    return np.full(64, v, np.int64)


def random_table(seed):
    return np.random.default_rng(seed).integers(1, 256, 64).astype(np.int64)


def pass_table(k, q=1):
    """q at zigzag position k, 255 everywhere else: only the coefficient at k survives quantisation"""
    t = flat_table(255)
    t[jm.ZIGZAG[k]] = q
    return t


# (luma, chroma), natural order.  "pair" and "swapped" differ per component: reading the other component's table fails
TABLES = {
    "ones": (flat_table(1), flat_table(1)),
    "all255": (flat_table(255), flat_table(255)),
    "random": (random_table(11), random_table(12)),
    "pair": (random_table(21), np.clip(random_table(22) // 4, 1, 255)),
}
TABLES["swapped"] = TABLES["pair"][::-1]


# ---- planar YUV hosts -----------------------------------------------------------------------------------------------
def yuv_host(y, u, v):
    """the tightly packed host image of a planar YUV surface from its three planes"""
    return np.concatenate([np.asarray(p, np.uint8).reshape(-1) for p in (y, u, v)])


def blocks_to_plane(blocks):
    """(N, 8, 8) -> one row of blocks, (8, 8 N)"""
    return np.ascontiguousarray(np.asarray(blocks, np.uint8).transpose(1, 0, 2).reshape(8, -1))


# ---- symbol images ------------------------------------------------------------------------------------------------------
# the zigzag positions of the first (only) non-zero AC coefficient: k = run + 1 gives runs 0..15; 17, 33 and 49 put one,
# two and three ZRL in front; 63 has three ZRL, run 14 and no EOB
AC_POSITIONS = tuple(range(1, 17)) + (17, 33, 49, 63)
AMPLITUDES = tuple(np.round(np.geomspace(0.2, 2000.0, 400), 3))


def basis_block(k, amp):
    """clip(round(128 + amp cos cos)) of the DCT basis function at zigzag position k"""
    n = int(jm.ZIGZAG[k])
    v, u = divmod(n, 8)
    x = np.arange(8)
    cu, cv = np.cos((2 * x + 1) * u * np.pi / 16), np.cos((2 * x + 1) * v * np.pi / 16)
    return np.clip(np.rint(128 + amp * np.outer(cv, cu)), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def ac_blocks(k, q=1, sizes=tuple(range(1, 11))):
    """for zigzag position k: blocks whose only non-zero coefficient under pass_table(k, q) is the one at k, for each
    of `sizes` and each sign the first amplitude that gives it, then an empty block (EOB alone).  Rounding to 8-bit
    samples moves all samples of a basis function together, so with q = 1 the smallest values are skipped at some
    positions (3 follows 0 at k = 1); q = 8 brings them back.  A size no amplitude reaches is left out: that the
    cases together reach every size is what tests/test_jpeg_params_host.py asserts."""
    cand = np.stack([basis_block(k, s * a) for a in AMPLITUDES for s in (1, -1)])
    z = jm.quantize(jm.fdct_islow(cand.astype(np.int64) - 128).reshape(-1, 64), pass_table(k, q))
    alone = (np.count_nonzero(z, axis=1) == 1) & (z[:, k] != 0)
    blocks = []
    for size in sizes:
        for sign in (1, -1):
            hit = np.flatnonzero(alone & (z[:, k] * sign > 0) & (np.abs(z[:, k]) >> (size - 1) == 1))
            if hit.size:
                blocks.append(cand[hit[0]])
    blocks.append(np.full((8, 8), 128, np.uint8))
    return np.stack(blocks)


def dc_blocks():
    """flat blocks whose steps 0, 1, 2, 4, ..., 128, 255 go up from 0 and down from 255: with q[0] = 8 the DC
    differences are the steps (categories 0..8), with q[0] = 1 eight times the steps (categories 4..11)"""
    vals = []
    for d in (0, 1, 2, 3, 4, 7, 8, 16, 32, 64, 128, 255):
        vals += [0, d, 0, 255, 255 - d, 255]
    return np.broadcast_to(np.asarray(vals, np.uint8)[:, None, None], (len(vals), 8, 8))


def symbol_cases():
    """[(name, blocks (N, 8, 8), table)]: 20 AC positions at q = 1, and at q = 8 for sizes 1..3, and two DC steps"""
    out = [(f"ac{k}", ac_blocks(k), pass_table(k)) for k in AC_POSITIONS]
    out += [(f"ac{k}_q8", ac_blocks(k, 8, (1, 2, 3)), pass_table(k, 8)) for k in AC_POSITIONS]
    out += [(f"dc_q{q}", dc_blocks(), pass_table(0, q)) for q in (1, 8)]
    return out


def symbol_image(kind, blocks, table):
    """kind "luma": YUV444, the blocks in Y;  "chroma": YUV444, the blocks in U and V (V reversed, so its differences
    are others);  "chroma420": the same in YUV420 under a flat Y of twice the size.  The other planes are flat 128.
    Returns (format, host, width, height, (luma table, chroma table))"""
    plane = blocks_to_plane(blocks)
    w, h = plane.shape[1], 8
    grey = np.full((h, w), 128, np.uint8)
    if kind == "luma":
        return jm.YUV444, yuv_host(plane, grey, grey), w, h, (table, flat_table(255))
    rev = blocks_to_plane(blocks[::-1])
    if kind == "chroma":
        return jm.YUV444, yuv_host(grey, plane, rev), w, h, (flat_table(255), table)
    assert kind == "chroma420"
    return jm.YUV420, yuv_host(np.full((2 * h, 2 * w), 128, np.uint8), plane, rev), 2 * w, 2 * h, (flat_table(255), table)


SYMBOL_KINDS = ("luma", "chroma", "chroma420")


# ---- the symbol counter -------------------------------------------------------------------------------------------------
def symbols_of_scan(coefs, comp, blocks_per_mcu, R):
    """the set of (table, "DC" | "AC", symbol) a scan emits: table 0 = luma, 1 = chroma; the DC symbol is the category
    of the difference to the previous block of the component (0 at the start of every restart segment of R MCUs, R = 0:
    never), the AC symbol (run << 4) | size, 0xF0 for sixteen zeros and 0x00 for the zeros that end a block"""
    seen = set()
    last_dc = {}
    for i, (z, c) in enumerate(zip(np.asarray(coefs).tolist(), np.asarray(comp).tolist())):
        mcu, first = divmod(i, blocks_per_mcu)
        if first == 0 and (mcu == 0 or (R and mcu % R == 0)):
            last_dc = {}
        t = min(c, 1)
        d = z[0] - last_dc.get(c, 0)
        last_dc[c] = z[0]
        seen.add((t, "DC", len(bin(abs(d))) - 2 if d else 0))
        zeros = 0
        for v in z[1:]:
            if v == 0:
                zeros += 1
                continue
            seen.update([(t, "AC", 0xF0)] * (zeros // 16))
            seen.add((t, "AC", (zeros % 16) * 16 + (len(bin(abs(v))) - 2)))
            zeros = 0
        if zeros:
            seen.add((t, "AC", 0x00))
    return seen


def symbols_of_image(fmt, host, w, h, tables, R=None, quality=0):
    R = jm.restart_interval(fmt) if R is None else R
    coefs, comp, bpm = jm.scan_blocks(fmt, jm.planes_of(fmt, host, w, h), w, h, quality, tables=tables)
    return symbols_of_scan(coefs, comp, bpm, R)


def every_symbol():
    """all 12 DC categories and all 162 AC symbols of both tables: 348"""
    ac = {0x00, 0xF0} | {(r << 4) | s for r in range(16) for s in range(1, 11)}
    return {(t, "DC", s) for t in (0, 1) for s in range(12)} | {(t, "AC", s) for t in (0, 1) for s in ac}


# ---- colour lattice -----------------------------------------------------------------------------------------------------
def lattice_colours():
    """every R, G, B of 16 levels 0, 17, ..., 255, then the neighbours at +-1 of the eight cube corners: (4120, 3)"""
    lv = np.arange(16) * 17
    grid = np.stack(np.meshgrid(lv, lv, lv, indexing="ij"), -1).reshape(-1, 3)
    near = []
    for corner in np.stack(np.meshgrid(*[(0, 255)] * 3, indexing="ij"), -1).reshape(-1, 3):
        for ch in range(3):
            c = corner.copy()
            c[ch] += 1 if c[ch] == 0 else -1
            near.append(c)
    return np.concatenate([grid, np.asarray(near)]).astype(np.uint8)


LATTICE_SIZE = (512, 520)        # 64 x 65 blocks: 4096 lattice colours, 24 corner neighbours, mid grey to the end


def lattice_rgb():
    """(520, 512, 3): one flat 8 x 8 block per colour"""
    w, h = LATTICE_SIZE
    cols = np.full(((w // 8) * (h // 8), 3), 128, np.uint8)
    lc = lattice_colours()
    cols[:len(lc)] = lc
    return np.ascontiguousarray(np.repeat(np.repeat(cols.reshape(h // 8, w // 8, 3), 8, 0), 8, 1))


def rgb_host(fmt, rgb):
    """an (H, W, 3) RGB picture as the tightly packed host image of RGB, BGR or RGB_PLANAR"""
    if fmt == jm.RGB:
        return np.ascontiguousarray(rgb).reshape(-1)
    if fmt == jm.BGR:
        return np.ascontiguousarray(rgb[..., ::-1]).reshape(-1)
    assert fmt == jm.RGB_PLANAR
    return np.ascontiguousarray(rgb.transpose(2, 0, 1)).reshape(-1)


# ---- extreme content ----------------------------------------------------------------------------------------------------
CONTENTS = ("pixel_checker", "block_checker", "h_ramp", "v_ramp", "binary")


def extreme_rgb(content, w, h, seed=0):
    """(h, w, 3) u8: the patterns with the largest and the most regular coefficients"""
    y, x = np.mgrid[:h, :w]
    if content == "pixel_checker":
        g = ((x + y) & 1) * 255
    elif content == "block_checker":
        g = ((x // 8 + y // 8) & 1) * 255
    elif content == "h_ramp":
        g = (x * 255) // max(w - 1, 1)
    elif content == "v_ramp":
        g = (y * 255) // max(h - 1, 1)
    else:
        assert content == "binary"
        return (np.random.default_rng(seed).integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    # the three channels out of step, so chroma is not flat
    return np.stack([g, 255 - g, np.roll(g, 3, 1)], -1).astype(np.uint8)


def content_host(fmt, content, w, h, seed=0):
    """`content` as a host image of fmt: "noise" and "flat" as jm.make_host, else extreme_rgb (for a YUV format the
    picture's three channels are the three planes, subsampled by dropping samples)"""
    if content in ("noise", "flat"):
        return jm.make_host(fmt, w, h, content, seed=seed)
    if content == "grey":                                      # every DC difference is 0, also after a restart
        return np.full(jm.make_host(fmt, w, h, "flat").size, 128, np.uint8)
    pic = extreme_rgb(content, w, h, seed)
    if fmt in (jm.RGB, jm.BGR, jm.RGB_PLANAR):
        return rgb_host(fmt, pic)
    cw, ch = jm.chroma_size(fmt, w, h)
    sx, sy = w // cw, h // ch
    return yuv_host(pic[..., 0], pic[::sy, ::sx, 1][:ch, :cw], pic[::sy, ::sx, 2][:ch, :cw])


# ---- segments and boundary inputs -----------------------------------------------------------------------------------
def split_segments(body):
    """entropy data -> [(stuffed bytes of the segment, its RST marker byte or None for the last)].  In stuffed data
    FF Dn can only be a marker."""
    out, start, i = [], 0, 0
    while i + 1 < len(body):
        if body[i] == 0xFF:
            if 0xD0 <= body[i + 1] <= 0xD7:
                out.append((bytes(body[start:i]), body[i + 1]))
                start = i + 2
            i += 2
        else:
            i += 1
    out.append((bytes(body[start:]), None))
    return out


def unstuff(seg):
    assert seg.count(b"\xff") == seg.count(b"\xff\x00")
    return seg.replace(b"\xff\x00", b"\xff")


def _ff_at(pred):
    return lambda raw, last: any(b == 0xFF and pred(i) for i, b in enumerate(raw))


# property name -> predicate(unstuffed bytes of a segment, is the last segment)
PROPERTIES = {
    "ff_at_lane_word_end": _ff_at(lambda i: i % 4 == 3),
    "ff_at_255": _ff_at(lambda i: i == 255),
    "ff_at_256": _ff_at(lambda i: i == 256),
    "ff_before_rst": lambda raw, last: not last and raw[-1:] == b"\xff",
    "ff_ff": lambda raw, last: b"\xff\xff" in raw,
    "len_multiple_of_256": lambda raw, last: len(raw) > 0 and len(raw) % 256 == 0,
    "len_not_multiple_of_4": lambda raw, last: len(raw) % 4 != 0,
    "shorter_than_4": lambda raw, last: 0 < len(raw) < 4,
    "no_ff": lambda raw, last: len(raw) > 0 and b"\xff" not in raw,
}

# what the search looks in: (format, width, height, content, quality, R); the seed goes to content_host
SEARCH_SPACE = {
    "ff_at_lane_word_end": (jm.RGB, 48, 32, "noise", 100, 21),
    "ff_at_255": (jm.RGB, 48, 32, "noise", 100, 21),
    "ff_at_256": (jm.YUV420, 64, 32, "noise", 100, 10),
    "ff_before_rst": (jm.YUV422, 64, 24, "noise", 75, 3),
    "ff_ff": (jm.RGB, 48, 32, "binary", 100, 21),
    "len_multiple_of_256": (jm.RGB, 64, 40, "noise", 91, 4),
    "len_not_multiple_of_4": (jm.YUV444, 40, 24, "noise", 50, 2),
    "shorter_than_4": (jm.YUV444, 40, 24, "grey", 90, 1),
    "no_ff": (jm.YUV444, 40, 24, "flat", 90, 1),
}

# the first seed at which the search finds the property (python tests/jpeg_encoder_inputs.py)
BOUNDARY_SEEDS = {
    "ff_at_lane_word_end": 0,
    "ff_at_255": 171,
    "ff_at_256": 33,
    "ff_before_rst": 3,
    "ff_ff": 131,
    "len_multiple_of_256": 80,
    "len_not_multiple_of_4": 0,
    "shorter_than_4": 0,
    "no_ff": 0,
}


def boundary_case(name, seed=None):
    """(format, host, width, height, quality, R) of the boundary input `name`"""
    fmt, w, h, content, q, R = SEARCH_SPACE[name]
    seed = BOUNDARY_SEEDS[name] if seed is None else seed
    return fmt, content_host(fmt, content, w, h, seed), w, h, q, R


def has_property(name, body):
    segs = split_segments(body)
    return any(PROPERTIES[name](unstuff(s), m is None) for s, m in segs)


def search(limit=4000):
    found = {}
    for name in SEARCH_SPACE:
        for seed in range(limit):
            fmt, host, w, h, q, R = boundary_case(name, seed)
            if has_property(name, jm.entropy(fmt, host, w, h, q, R=R)):
                found[name] = seed
                break
    return found


if __name__ == "__main__":
    for name, seed in search().items():
        print(f'    "{name}": {seed},')
