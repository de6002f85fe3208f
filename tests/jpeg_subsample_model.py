"""numpy restatement of the encoder's chroma downsampling for RGB, BGR and RGB_PLANAR sources coded 4:2:2 or 4:2:0
(include/vali_hip.h, "JPEG"), for the tests only.  Everything else comes from tests/jpeg_model.py.

The definition is libjpeg-turbo's default pipeline (jccolor, jcprepct, jcsample; no smoothing, no fancy downsampling):
every full-resolution pixel goes through rgb_ycc and is truncated to 8 bits, then chroma is averaged with an
alternating bias,
    4:2:0   c[y][x] = (p[2y][2x] + p[2y][2x+1] + p[2y+1][2x] + p[2y+1][2x+1] + (1, 2, 1, 2, ...)[x]) >> 2
    4:2:2   c[y][x] = (p[y][2x] + p[y][2x+1] + (0, 1, 0, 1, ...)[x]) >> 1
and the edges are not symmetric: horizontally the FULL-RESOLUTION row is replicated out to the edge of the chroma
component's last real block (a chroma sample past the component's width is an average of replicated pixels, with its
own bias, not a copy of its neighbour); vertically the full-resolution image is replicated to a multiple of V rows only,
and the downsampled rows are replicated below that.
"""
from __future__ import annotations

import numpy as np

import jpeg_model as jm

SAMPLINGS = {"444": (1, 1), "422": (2, 1), "420": (2, 2)}
PILLOW_SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def restart_interval(samp):
    """R: MCUs per restart segment, at most 64 blocks each: 21 / 16 / 10"""
    H, V = SAMPLINGS[samp]
    return 64 // (H * V + 2)


def rgb_of(fmt, host, w, h):
    """(h, w, 3) RGB pixels of a tightly packed host image of one of the three RGB layouts"""
    host = np.asarray(host, np.uint8).reshape(-1)[:w * h * 3]
    if fmt == jm.RGB:
        return host.reshape(h, w, 3)
    if fmt == jm.BGR:
        return host.reshape(h, w, 3)[..., ::-1]
    assert fmt == jm.RGB_PLANAR, fmt
    return host.reshape(3, h, w).transpose(1, 2, 0)


def downsample(plane, H, V):
    """jcsample h2v1_downsample / h2v2_downsample of one full-resolution chroma plane, out to the last real block:
    (bh * 8, bw * 8) samples, bw = ceil(ceil(w / H) / 8), bh = ceil(ceil(h / V) / 8)"""
    h, w = plane.shape
    cw, ch = -(-w // H), -(-h // V)
    bw, bh = -(-cw // 8), -(-ch // 8)
    # index form: chroma (x, y) reads columns min(2x, w-1), min(2x+1, w-1) and, with y' = min(y, ch-1), rows
    # min(2y', h-1), min(2y'+1, h-1) at 4:2:0, row y' at 4:2:2
    x = np.arange(bw * 8)
    y = np.minimum(np.arange(bh * 8), ch - 1)
    x0, x1 = np.minimum(2 * x, w - 1), np.minimum(2 * x + 1, w - 1)
    p = plane.astype(np.int64)
    if V == 2:
        y0, y1 = np.minimum(2 * y, h - 1), np.minimum(2 * y + 1, h - 1)
        s = p[y0][:, x0] + p[y0][:, x1] + p[y1][:, x0] + p[y1][:, x1]
        return ((s + 1 + (x & 1)[None, :]) >> 2).astype(np.uint8)
    s = p[y][:, x0] + p[y][:, x1]
    return ((s + (x & 1)[None, :]) >> 1).astype(np.uint8)


def planes_of(fmt, host, w, h, samp):
    """the three component planes the scan codes: luma at full size, chroma downsampled out to its last real block (the
    part past ceil(w / H) x ceil(h / V) is what jm.component_blocks must see instead of its own edge replication)"""
    H, V = SAMPLINGS[samp]
    y, cb, cr = jm.rgb_to_ycc(rgb_of(fmt, host, w, h))
    if (H, V) == (1, 1):
        return [y, cb, cr]
    return [y, downsample(cb, H, V), downsample(cr, H, V)]


def scan_blocks(fmt, host, w, h, quality, samp, tables=None):
    """every block in MCU-interleaved scan order, dummy blocks included (jm.scan_blocks with the chroma planes above)"""
    H, V = SAMPLINGS[samp]
    planes = planes_of(fmt, host, w, h, samp)
    if (H, V) == (1, 1):
        return jm.scan_blocks(fmt, planes, w, h, quality, tables=tables)
    mx, my = -(-w // (8 * H)), -(-h // (8 * V))
    lq, cq = tables if tables is not None else jm.quant_tables(quality)
    comps = []
    for c, (pl, hs, vs) in enumerate(zip(planes, (H, 1, 1), (V, 1, 1))):
        cw, ch = -(-w * hs // H), -(-h * vs // V)
        bw, bh = -(-cw // 8), -(-ch // 8)
        # luma: replicate the last column and row; chroma: already (bh * 8, bw * 8), nothing left to replicate
        real = jm.component_blocks(np.asarray(pl) if c else np.asarray(pl)[:ch, :cw], lq if c == 0 else cq, bw, bh)
        full = np.zeros((my * vs, mx * hs, 64), np.int32)
        full[:bh, :bw] = real
        for x in range(bw, mx * hs):
            full[:bh, x, 0] = full[:bh, x - 1, 0]
        for y in range(bh, my * vs):
            for m in range(mx):
                full[y, m * hs:(m + 1) * hs, 0] = full[y - 1, m * hs + hs - 1, 0]
        comps.append((full, hs, vs))
    coefs, comp = [], []
    for m_y in range(my):
        rows = []
        for full, hs, vs in comps:
            rows.append(full[m_y * vs:(m_y + 1) * vs].reshape(vs, mx, hs, 64).transpose(1, 0, 2, 3).reshape(mx, vs * hs, 64))
        coefs.append(np.concatenate(rows, 1).reshape(-1, 64))
        comp.append(np.tile(np.repeat(np.arange(3), [H * V, 1, 1]), mx))
    return np.concatenate(coefs), np.concatenate(comp), H * V + 2


def header(w, h, quality, samp, R=None, tables=None):
    """jm.header with the luma sampling of `samp` in SOF0 and its restart interval in DRI (R = 0: no DRI)"""
    H, V = SAMPLINGS[samp]
    R = restart_interval(samp) if R is None else R
    base = jm.header(w, h, jm.RGB, quality, R, tables)      # 4:4:4: the SOF0 sampling byte is 0x11
    sof = base.index(b"\xff\xc0")
    at = sof + 4 + 1 + 2 + 2 + 1 + 1                        # marker, length, precision, height, width, count, id
    assert base[at] == 0x11
    return base[:at] + bytes([(H << 4) | V]) + base[at + 1:]


def entropy(fmt, host, w, h, quality, samp, R=None, tables=None):
    R = restart_interval(samp) if R is None else R
    if tables is not None:
        tables = tuple(np.asarray(t) for t in tables)
    coefs, comp, bpm = scan_blocks(fmt, host, w, h, quality, samp, tables)
    return jm.huffman(coefs, comp, bpm, R)


def encode(fmt, host, w, h, quality, samp, R=None, tables=None):
    """the whole file PyNvJpegEncoder(backend="hip") writes with Context(quality, fmt, subsampling=samp)"""
    return header(w, h, quality, samp, R, tables) + entropy(fmt, host, w, h, quality, samp, R, tables) + b"\xff\xd9"


def pillow_encode(fmt, host, w, h, quality, samp):
    """Pillow's (libjpeg-turbo's) file for the same pixels and sampling: no restart markers"""
    import io

    from PIL import Image

    out = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb_of(fmt, host, w, h)), "RGB").save(
        out, format="JPEG", quality=max(1, min(100, int(quality))), subsampling=PILLOW_SUBSAMPLING[samp])
    return out.getvalue()


def make_host(fmt, w, h, content, seed=0, frame=None):
    """jm.make_host plus "checker": a one-pixel checkerboard of two colours whose chroma differ by an odd amount, so
    every 2x1 and 2x2 sum is odd / leaves a remainder and the alternating bias decides each chroma sample;
    "binary": every channel 0 or 255"""
    if content in ("noise", "flat", "frame"):
        return jm.make_host(fmt, w, h, content, seed, frame)
    rng = np.random.default_rng(seed)
    if content == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        a, b = np.array([200, 30, 61], np.uint8), np.array([17, 180, 244], np.uint8)
        rgb = np.where(((xx + yy) & 1)[..., None] == 0, a, b).astype(np.uint8)
    else:
        assert content == "binary", content
        rgb = (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    if fmt == jm.RGB:
        return np.ascontiguousarray(rgb).reshape(-1)
    if fmt == jm.BGR:
        return np.ascontiguousarray(rgb[..., ::-1]).reshape(-1)
    return np.ascontiguousarray(rgb.transpose(2, 0, 1)).reshape(-1)
