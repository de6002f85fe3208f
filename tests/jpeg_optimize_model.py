"""numpy restatement of the encoder's per-image optimised Huffman tables (include/vali_hip.h, "JPEG", optimize = 1), for
the tests only.  Pixels, sampling, FDCT, quantisation and the scan order come from tests/jpeg_model.py and
tests/jpeg_subsample_model.py unchanged; this file adds the second pass of libjpeg's jchuff:

  - the symbol counts of the scan (DC size categories, AC run << 4 | size, ZRL, EOB; DC prediction restarts with every
    restart segment; dummy blocks count, because they are coded),
  - jpeg_gen_optimal_table of each of the four counts,
  - entropy coding with those tables, and the file layout of the GPU encoder: SOI, APP0, DQT, SOF0 from the host, then
    DHT (the image's own tables), DRI, SOS and the entropy data from the device.

tests/test_jpeg_optimize_host.py pins the tables and the entropy data to Pillow's save(optimize=True,
restart_marker_blocks=R).
"""
from __future__ import annotations

import numpy as np

import jpeg_model as jm
import jpeg_subsample_model as sm

# DHT order: table class << 4 | id
DHT_ORDER = (0x00, 0x10, 0x01, 0x11)        # DC luma, AC luma, DC chroma, AC chroma
# the worst case of what the device writes before the entropy data: DHT, DRI, SOS
PREFIX_MAX = (4 + 4 * 17 + 12 + 12 + 162 + 162) + 6 + 14


# ---- the scan, walked once for counting and once for coding ---------------------------------------------------------------
def walk(coefs, comp, blocks_per_mcu, R, dc, ac, restart):
    """jchuff encode_one_block over the scan: dc(table, size, diff) and ac(table, symbol, value) for every symbol in
    coding order (value is None for ZRL and EOB), restart(index) before MCU m = k R"""
    pred = [0, 0, 0]
    for m in range(len(coefs) // blocks_per_mcu):
        if R and m and m % R == 0:
            restart(m // R - 1)
            pred = [0, 0, 0]
        for b in range(m * blocks_per_mcu, (m + 1) * blocks_per_mcu):
            c, z = int(comp[b]), coefs[b]
            t = 0 if c == 0 else 1
            diff = int(z[0]) - pred[c]
            pred[c] = int(z[0])
            dc(t, jm._size(diff), diff)
            last = 0
            for k in np.flatnonzero(z[1:]) + 1:
                run = int(k) - last - 1
                while run > 15:
                    ac(t, 0xF0, None)
                    run -= 16
                v = int(z[k])
                ac(t, (run << 4) | jm._size(v), v)
                last = int(k)
            if last < 63:
                ac(t, 0x00, None)


def symbol_counts(coefs, comp, blocks_per_mcu, R):
    """(4, 256) counts in DHT order: DC luma, AC luma, DC chroma, AC chroma"""
    counts = np.zeros((4, 256), np.int64)

    def dc(t, s, diff):
        counts[2 * t, s] += 1

    def ac(t, sym, v):
        counts[2 * t + 1, sym] += 1

    walk(coefs, comp, blocks_per_mcu, R, dc, ac, lambda i: None)
    return counts


# ---- jpeg_gen_optimal_table --------------------------------------------------------------------------------------------
def code_sizes(counts):
    """the unlimited code length of each of the 257 symbols (256 is the pseudo-symbol that keeps the all-ones code
    free): the depth in the merge tree.  c1 is the largest index among the minima, c2 the largest among the minima of
    the rest, and the sum stays at c1."""
    freq = [int(v) for v in counts] + [1]
    size = [0] * 257
    others = [-1] * 257
    while True:
        c1, v = -1, None
        for i in range(257):
            if freq[i] and (v is None or freq[i] <= v):
                v, c1 = freq[i], i
        c2, v = -1, None
        for i in range(257):
            if freq[i] and i != c1 and (v is None or freq[i] <= v):
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        size[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            size[c1] += 1
        others[c1] = c2
        size[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            size[c2] += 1
    return size


def optimal_table(counts):
    """(BITS[1..16], HUFFVAL) of 256 symbol counts, as libjpeg's jpeg_gen_optimal_table"""
    size = code_sizes(counts)
    assert max(size) <= 32
    bits = [0] * 33
    for s in size:
        if s:
            bits[s] += 1
    for i in range(32, 16, -1):                 # Annex K.2, figure K.3
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                # the pseudo-symbol's code
    vals = [j for length in range(1, 33) for j in range(256) if size[j] == length]
    return bits[1:17], vals


def tables_of(counts):
    """the four (BITS, HUFFVAL) tables in DHT order"""
    return [optimal_table(c) for c in counts]


# ---- coding ------------------------------------------------------------------------------------------------------------------
def huffman(coefs, comp, blocks_per_mcu, R, tables):
    """jm.huffman with the four tables of `tables` (DHT order) instead of Annex K's"""
    codes = [jm.huff_codes(t) for t in tables]
    bits = jm._Bits()

    def dc(t, s, diff):
        bits.put(*codes[2 * t][s])
        if s:
            bits.put(diff if diff >= 0 else diff - 1, s)

    def ac(t, sym, v):
        bits.put(*codes[2 * t + 1][sym])
        if v is not None:
            bits.put(v if v >= 0 else v - 1, sym & 15)

    def restart(i):
        bits.flush()
        bits.out += bytes([0xFF, 0xD0 + i % 8])

    walk(coefs, comp, blocks_per_mcu, R, dc, ac, restart)
    bits.flush()
    return bytes(bits.out)


def samp_of(fmt, samp=None):
    return samp or {jm.YUV422: "422", jm.YUV420: "420"}.get(fmt, "444")


def scan_blocks(fmt, host, w, h, quality, samp=None):
    """the scan of a host image of any of the six formats; samp: the sampling of an RGB source (None: 4:4:4)"""
    if fmt in (jm.RGB, jm.BGR, jm.RGB_PLANAR):
        return sm.scan_blocks(fmt, host, w, h, quality, samp_of(fmt, samp))
    return jm.scan_blocks(fmt, jm.planes_of(fmt, host, w, h), w, h, quality)


def analyse(fmt, host, w, h, quality, samp=None, R=None):
    """(tables in DHT order, entropy data, counts) of one image"""
    R = sm.restart_interval(samp_of(fmt, samp)) if R is None else R
    coefs, comp, bpm = scan_blocks(fmt, host, w, h, quality, samp)
    counts = symbol_counts(coefs, comp, bpm, R)
    tables = tables_of(counts)
    return tables, huffman(coefs, comp, bpm, R, tables), counts


# ---- file -------------------------------------------------------------------------------------------------------------------
def fixed_header(w, h, fmt, quality, samp=None):
    """what vali_jpeg_header writes with optimize = 1: the plain header up to and including SOF0"""
    plain = sm.header(w, h, quality, samp_of(fmt, samp))
    return plain[:plain.index(b"\xff\xc4")]


def prefix(tables, R):
    """what the device writes before the entropy data: DHT (the four tables in one segment), DRI, SOS"""
    dht = b"".join(bytes([cls_id]) + bytes(bits) + bytes(vals) for cls_id, (bits, vals) in zip(DHT_ORDER, tables))
    return jm._seg(0xC4, dht) + jm._seg(0xDD, R.to_bytes(2, "big")) + jm._seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11,
                                                                                            0, 63, 0]))


def encode(fmt, host, w, h, quality, samp=None, R=None):
    """the whole file PyNvJpegEncoder(backend="hip") writes with Context(quality, fmt, samp, optimize=True)"""
    R = sm.restart_interval(samp_of(fmt, samp)) if R is None else R
    tables, data, _ = analyse(fmt, host, w, h, quality, samp, R)
    return fixed_header(w, h, fmt, quality, samp) + prefix(tables, R) + data + b"\xff\xd9"


def tables_of_file(data):
    """the Huffman tables of a JPEG file: {class << 4 | id: (BITS, HUFFVAL)}, from all of its DHT segments"""
    out, i = {}, 2
    while True:
        assert data[i] == 0xFF, i
        marker, length = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        if marker == 0xC4:
            k, end = i + 4, i + 2 + length
            while k < end:
                bits = list(data[k + 1:k + 17])
                out[data[k]] = (bits, list(data[k + 17:k + 17 + sum(bits)]))
                k += 17 + sum(bits)
            assert k == end
        i += 2 + length
        if marker == 0xDA:
            return out


# ---- inputs and Pillow ----------------------------------------------------------------------------------------------------
def smooth_host(fmt, w, h, seed=0):
    """a smooth picture: a colour gradient with a little noise, so that few symbols carry most of the counts"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    rgb = np.stack([40 + 150 * xx / max(w - 1, 1), 200 - 120 * yy / max(h - 1, 1), 90 + 60 * (xx + yy) / max(w + h - 2, 1)],
                   -1) + rng.normal(0, 1.5, (h, w, 3))
    return jm.make_host(fmt, w, h, "frame", frame=np.clip(np.rint(rgb), 0, 255).astype(np.uint8))


def long_code_host(w=512, h=512):
    """a grey RGB picture whose AC luma code lengths reach 17 before limiting at quality 100: vertical bands, each half
    the width of the last, of Gaussian noise on level 128 whose sigma grows 2.2x per band from 0.6"""
    rng = np.random.default_rng(3)
    grey = np.full((h, w), 128.0)
    x0, bw, sigma = 0, w // 2, 0.6
    while bw >= 1 and x0 < w:
        grey[:, x0:x0 + bw] += rng.normal(0, sigma, (h, bw))
        x0, bw, sigma = x0 + bw, bw // 2, sigma * 2.2
    g = np.clip(np.rint(grey), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(g[..., None], 3, -1)).reshape(-1)


def make_host(fmt, w, h, content, seed=0, frame=None):
    if content == "smooth":
        return smooth_host(fmt, w, h, seed)
    return jm.make_host(fmt, w, h, content, seed, frame)


def pillow_encode(fmt, host, w, h, quality, samp=None, R=0, optimize=True):
    """Pillow's (libjpeg-turbo's) file for the same pixels: optimize=True builds the tables from the image's own symbol
    statistics; R MCUs per restart interval (0: none)"""
    import io

    from PIL import Image

    host = np.asarray(host, np.uint8).reshape(-1)
    if fmt in (jm.RGB, jm.BGR, jm.RGB_PLANAR):
        img = Image.fromarray(np.ascontiguousarray(sm.rgb_of(fmt, host, w, h)), "RGB")
    else:
        y, u, v = jm.planes_of(fmt, host, w, h)
        u = np.repeat(np.repeat(u, h // u.shape[0], 0), w // u.shape[1], 1)
        v = np.repeat(np.repeat(v, h // v.shape[0], 0), w // v.shape[1], 1)
        img = Image.fromarray(np.ascontiguousarray(np.stack([y, u, v], -1)), "YCbCr")
    out = io.BytesIO()
    img.save(out, format="JPEG", quality=max(1, min(100, int(quality))),
             subsampling=sm.PILLOW_SUBSAMPLING[samp_of(fmt, samp)], optimize=optimize, restart_marker_blocks=R)
    return out.getvalue()
