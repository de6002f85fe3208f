"""numpy restatement of the baseline JPEG encoder of include/vali_hip.h (vali_jpeg_encode_batch), for the tests only.

Every stage follows libjpeg (the 6b / libjpeg-turbo C code Pillow bundles): rgb_ycc (jccolor), edge replication and the
dummy blocks of a partial MCU (jcprepct / jccoefct), the accurate integer FDCT "islow" (jfdctint), quantisation
(jcdctmgr) and Huffman coding with the standard tables of ITU T.81 Annex K (jchuff).  With R = 0 (no restart markers)
the entropy data equals what Pillow writes for the same pixels (tests/test_jpeg_host.py pins it); with R > 0 it is what
vali_jpeg_encode_batch writes.
"""
from __future__ import annotations

import numpy as np

# formats (enum vali_pixel_format)
RGB, YUV420, RGB_PLANAR, BGR, YUV444, YUV422 = 2, 4, 5, 6, 7, 10
FORMATS = (RGB, BGR, RGB_PLANAR, YUV444, YUV422, YUV420)

# natural index of zigzag position k
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                   7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                   39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# Annex K.1, natural order
LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                   14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                     47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)

# Annex K.3: (BITS[1..16], HUFFVAL)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14,
    0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09,
    0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a,
    0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65,
    0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88,
    0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9,
    0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
    0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea,
    0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32,
    0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16,
    0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39,
    0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64,
    0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86,
    0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8,
    0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9,
    0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])


def huff_codes(table):
    """Annex C: symbol -> (code, length) for a (BITS, HUFFVAL) table"""
    bits, vals = table
    code, k, out = 0, 0, {}
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def sampling(fmt):
    """luma (H, V) sampling factors; chroma is 1 x 1"""
    return {YUV422: (2, 1), YUV420: (2, 2)}.get(fmt, (1, 1))


def restart_interval(fmt):
    """R: MCUs per restart segment, at most 64 blocks each"""
    h, v = sampling(fmt)
    return 64 // (h * v + 2)


def quant_tables(quality):
    """jpeg_set_quality(quality, force_baseline=TRUE): (luma, chroma) in natural order"""
    q = max(1, min(100, int(quality)))
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((t * scale + 50) // 100, 1, 255) for t in (LUMA_Q, CHROMA_Q))


def quant_recip(q8):
    """jcdctmgr compute_reciprocal for the divisor 8q: (reciprocal, correction, shift) with
    (|x| + correction) * reciprocal >> shift == round_half_away(|x| / 8q) for every |x| < 2^15 (test_jpeg_host)"""
    b = int(q8).bit_length() - 1
    r = 16 + b
    fq, fr, c = (1 << r) // q8, (1 << r) % q8, q8 // 2
    if fr == 0:
        fq, r = fq >> 1, r - 1
    elif fr <= q8 // 2:
        c += 1
    else:
        fq += 1
    return fq, c, r


# ---- colour ----------------------------------------------------------------------------------------------------------
def _fix(x):
    return int(x * 65536 + 0.5)


def rgb_to_ycc(rgb):
    """jccolor rgb_ycc_convert: (H, W, 3) u8 -> three u8 planes"""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    half = 1 << 15
    y = (_fix(0.299) * r + _fix(0.587) * g + _fix(0.114) * b + half) >> 16
    cb = (-_fix(0.16874) * r - _fix(0.33126) * g + _fix(0.5) * b + (128 << 16) + half - 1) >> 16
    cr = (_fix(0.5) * r - _fix(0.41869) * g - _fix(0.08131) * b + (128 << 16) + half - 1) >> 16
    return [p.astype(np.uint8) for p in (y, cb, cr)]


def planes_of(fmt, host, w, h):
    """the three component planes the encoder reads from a tightly packed host image (Surface.HostSize layout)"""
    host = np.asarray(host, np.uint8).reshape(-1)
    if fmt == RGB:
        return rgb_to_ycc(host[:w * h * 3].reshape(h, w, 3))
    if fmt == BGR:
        return rgb_to_ycc(host[:w * h * 3].reshape(h, w, 3)[..., ::-1])
    if fmt == RGB_PLANAR:
        return rgb_to_ycc(host[:w * h * 3].reshape(3, h, w).transpose(1, 2, 0))
    cw, ch = (w, h) if fmt == YUV444 else (w // 2, h) if fmt == YUV422 else (w // 2, h // 2)
    y = host[:w * h].reshape(h, w)
    u = host[w * h: w * h + cw * ch].reshape(ch, cw)
    v = host[w * h + cw * ch: w * h + 2 * cw * ch].reshape(ch, cw)
    return [y, u, v]


# ---- transform + quantisation ------------------------------------------------------------------------------------------
C = dict(c0298=2446, c0390=3196, c0541=4433, c0765=6270, c0899=7373, c1175=9633, c1501=12299, c1847=15137,
         c1961=16069, c2053=16819, c2562=20995, c3072=25172)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """one pass of jfdctint over the last axis (8 values); pass 1 (rows) keeps PASS1_BITS = 2 extra bits"""
    s = [d[..., i] for i in range(8)]
    tmp0, tmp7 = s[0] + s[7], s[0] - s[7]
    tmp1, tmp6 = s[1] + s[6], s[1] - s[6]
    tmp2, tmp5 = s[2] + s[5], s[2] - s[5]
    tmp3, tmp4 = s[3] + s[4], s[3] - s[4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    out = [None] * 8
    sh = 13 - 2 if first else 13 + 2
    if first:
        out[0], out[4] = (tmp10 + tmp11) << 2, (tmp10 - tmp11) << 2
    else:
        out[0], out[4] = _descale(tmp10 + tmp11, 2), _descale(tmp10 - tmp11, 2)
    z1 = (tmp12 + tmp13) * C["c0541"]
    out[2] = _descale(z1 + tmp13 * C["c0765"], sh)
    out[6] = _descale(z1 - tmp12 * C["c1847"], sh)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * C["c1175"]
    tmp4, tmp5, tmp6, tmp7 = tmp4 * C["c0298"], tmp5 * C["c2053"], tmp6 * C["c3072"], tmp7 * C["c1501"]
    z1, z2, z3, z4 = -z1 * C["c0899"], -z2 * C["c2562"], -z3 * C["c1961"] + z5, -z4 * C["c0390"] + z5
    out[7] = _descale(tmp4 + z1 + z3, sh)
    out[5] = _descale(tmp5 + z2 + z4, sh)
    out[3] = _descale(tmp6 + z2 + z3, sh)
    out[1] = _descale(tmp7 + z1 + z4, sh)
    return np.stack(out, -1)


def fdct_islow(blocks):
    """(N, 8, 8) level-shifted samples -> (N, 8, 8) coefficients scaled by 8 (jfdctint)"""
    d = blocks.astype(np.int64)
    d = _fdct_1d(d, True)                                   # rows
    d = _fdct_1d(d.transpose(0, 2, 1), False)               # columns
    return d.transpose(0, 2, 1)


def quantize(coef, qtab):
    """(N, 64) natural-order coefficients / (8 q), rounded half away from zero -> zigzag order"""
    q8 = (8 * qtab.astype(np.int64))[None, :]
    a = np.abs(coef)
    v = (a + q8 // 2) // q8
    return np.where(coef < 0, -v, v)[:, ZIGZAG].astype(np.int32)


def component_blocks(plane, qtab, bw, bh):
    """plane replicated at its last column / row out to (bw, bh) blocks -> (bh, bw, 64) zigzag coefficients"""
    ph, pw = plane.shape
    p = np.pad(plane, ((0, bh * 8 - ph), (0, bw * 8 - pw)), mode="edge").astype(np.int64) - 128
    blk = p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
    return quantize(fdct_islow(blk).reshape(-1, 64), qtab).reshape(bh, bw, 64)


def scan_blocks(fmt, planes, w, h, quality, tables=None, samp=None):
    """every block in MCU-interleaved scan order, dummy blocks included: (coefficients (N, 64), component (N,)).
    tables: (luma, chroma) quantisation tables instead of those of `quality`; samp: (H, V) instead of fmt's"""
    H, V = samp or sampling(fmt)
    mx, my = -(-w // (8 * H)), -(-h // (8 * V))
    lq, cq = tables if tables is not None else quant_tables(quality)
    comps = []
    for c, (pl, hs, vs) in enumerate(zip(planes, (H, 1, 1), (V, 1, 1))):
        cw, ch = -(-w * hs // H), -(-h * vs // V)           # component size (jdiv_round_up)
        bw, bh = -(-cw // 8), -(-ch // 8)
        real = component_blocks(np.asarray(pl)[:ch, :cw], lq if c == 0 else cq, bw, bh)
        full = np.zeros((my * vs, mx * hs, 64), np.int32)
        full[:bh, :bw] = real
        for x in range(bw, mx * hs):                        # dummy column of the last MCU: DC from the block to the left
            full[:bh, x, 0] = full[:bh, x - 1, 0]
        for y in range(bh, my * vs):                        # dummy row: DC from the previous block of this MCU
            for m in range(mx):
                full[y, m * hs:(m + 1) * hs, 0] = full[y - 1, m * hs + hs - 1, 0]
        comps.append((full, hs, vs))
    coefs, comp = [], []
    for m_y in range(my):
        rows = []
        for c, (full, hs, vs) in enumerate(comps):
            # (mx, vs*hs, 64): blocks of component c in each MCU of this MCU row
            part = full[m_y * vs:(m_y + 1) * vs].reshape(vs, mx, hs, 64).transpose(1, 0, 2, 3).reshape(mx, vs * hs, 64)
            rows.append(part)
        per_mcu = np.concatenate(rows, 1)                   # (mx, blocks per MCU, 64)
        coefs.append(per_mcu.reshape(-1, 64))
        comp.append(np.tile(np.repeat(np.arange(3), [H * V, 1, 1]), mx))
    return np.concatenate(coefs), np.concatenate(comp), H * V + 2


# ---- entropy coding ----------------------------------------------------------------------------------------------------
_DC = [huff_codes(DC_LUMA), huff_codes(DC_CHROMA)]
_AC = [huff_codes(AC_LUMA), huff_codes(AC_CHROMA)]


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)   # pad with 1-bits


def _size(v):
    return int(abs(int(v))).bit_length()


def huffman(coefs, comp, blocks_per_mcu, R):
    """jchuff encode_one_block over the scan; R MCUs per restart segment (R = 0: no restart markers)"""
    bits = _Bits()
    pred = [0, 0, 0]
    n_mcu = len(coefs) // blocks_per_mcu
    for m in range(n_mcu):
        if R and m and m % R == 0:
            bits.flush()
            bits.out += bytes([0xFF, 0xD0 + (m // R - 1) % 8])
            pred = [0, 0, 0]
        for b in range(m * blocks_per_mcu, (m + 1) * blocks_per_mcu):
            c, z = int(comp[b]), coefs[b]
            t = 0 if c == 0 else 1
            diff = int(z[0]) - pred[c]
            pred[c] = int(z[0])
            s = _size(diff)
            bits.put(*_DC[t][s])
            if s:
                bits.put(diff if diff >= 0 else diff - 1, s)
            run = 0
            nz = np.flatnonzero(z[1:]) + 1
            last = 0
            for k in nz:
                run = int(k) - last - 1
                while run > 15:
                    bits.put(*_AC[t][0xF0])
                    run -= 16
                v = int(z[k])
                s = _size(v)
                bits.put(*_AC[t][(run << 4) | s])
                bits.put(v if v >= 0 else v - 1, s)
                last = int(k)
            if last < 63:
                bits.put(*_AC[t][0x00])
    bits.flush()
    return bytes(bits.out)


# ---- file ----------------------------------------------------------------------------------------------------------------
def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def header(w, h, fmt, quality, R=None, tables=None):
    """SOI, APP0 (JFIF 1.1, aspect 1:1), DQT (both tables), SOF0, DHT (four tables), DRI, SOS.
    tables: (luma, chroma) quantisation tables in natural order instead of those of `quality`"""
    R = restart_interval(fmt) if R is None else R
    H, V = sampling(fmt)
    lq, cq = (np.asarray(t) for t in tables) if tables is not None else quant_tables(quality)
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += _seg(0xDB, bytes([0]) + bytes(lq[ZIGZAG].tolist()) + bytes([1]) + bytes(cq[ZIGZAG].tolist()))
    out += _seg(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([3, 1, (H << 4) | V, 0,
                                                                                       2, 0x11, 1, 3, 0x11, 1]))
    dht = b""
    for cls_id, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        dht += bytes([cls_id]) + bytes(bits) + bytes(vals)
    out += _seg(0xC4, dht)
    if R:
        out += _seg(0xDD, R.to_bytes(2, "big"))
    out += _seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def entropy(fmt, host, w, h, quality, R=None, tables=None):
    """the entropy-coded data (restart markers included) of one image"""
    R = restart_interval(fmt) if R is None else R
    if tables is not None:
        tables = tuple(np.asarray(t) for t in tables)
    coefs, comp, bpm = scan_blocks(fmt, planes_of(fmt, host, w, h), w, h, quality, tables=tables)
    return huffman(coefs, comp, bpm, R)


def encode(fmt, host, w, h, quality, R=None, tables=None):
    """the whole file vali_jpeg_header + vali_jpeg_encode_batch + EOI produce"""
    return header(w, h, fmt, quality, R, tables) + entropy(fmt, host, w, h, quality, R, tables) + b"\xff\xd9"


def entropy_of_file(data):
    """the entropy-coded data of a baseline JPEG file: from after the SOS segment up to EOI"""
    i = 2
    while True:
        assert data[i] == 0xFF, i
        marker, length = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        i += 2 + length
        if marker == 0xDA:
            break
    assert data[-2:] == b"\xff\xd9"
    return bytes(data[i:-2])


# ---- test inputs and the Pillow encoder of the CPU backend --------------------------------------------------------------
def chroma_size(fmt, w, h):
    return (w, h) if fmt == YUV444 else (w // 2, h) if fmt == YUV422 else (w // 2, h // 2)


def make_host(fmt, w, h, content="noise", seed=0, frame=None):
    """a tightly packed host image of `fmt` (Surface.HostSize layout): "noise", "flat" or "frame" (an (H, W, 3) u8
    RGB picture tiled to w x h)"""
    rng = np.random.default_rng(seed)
    if content == "noise":
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif content == "flat":
        rgb = np.broadcast_to(rng.integers(0, 256, 3, dtype=np.uint8), (h, w, 3))
    else:
        fh, fw = frame.shape[:2]
        rgb = np.tile(frame, (-(-h // fh), -(-w // fw), 1))[:h, :w]
    if fmt == RGB:
        return np.ascontiguousarray(rgb).reshape(-1)
    if fmt == BGR:
        return np.ascontiguousarray(rgb[..., ::-1]).reshape(-1)
    if fmt == RGB_PLANAR:
        return np.ascontiguousarray(rgb.transpose(2, 0, 1)).reshape(-1)
    y, u, v = rgb_to_ycc(np.asarray(rgb))
    sx, sy = {YUV444: (1, 1), YUV422: (2, 1), YUV420: (2, 2)}[fmt]
    cw, ch = chroma_size(fmt, w, h)
    return np.concatenate([y.reshape(-1), u[::sy, ::sx][:ch, :cw].reshape(-1), v[::sy, ::sx][:ch, :cw].reshape(-1)])


def pillow_encode(fmt, host, w, h, quality, tables=None):
    """what the CPU backend of PyNvJpegEncoder writes for this host image (vali_amd/codecs.py: Pillow, libjpeg).
    tables: (luma, chroma) in natural order, unscaled, instead of those of `quality`; the order and the scale Pillow
    applies are checked by reading the file's tables back"""
    import io

    from PIL import Image

    host = np.asarray(host, np.uint8).reshape(-1)
    if fmt in (RGB, BGR, RGB_PLANAR):
        rgb = {RGB: lambda a: a.reshape(h, w, 3), BGR: lambda a: a.reshape(h, w, 3)[..., ::-1],
               RGB_PLANAR: lambda a: a.reshape(3, h, w).transpose(1, 2, 0)}[fmt](host[:w * h * 3])
        img, sub = Image.fromarray(np.ascontiguousarray(rgb), "RGB"), 0
    else:
        y, u, v = planes_of(fmt, host, w, h)
        u = np.repeat(np.repeat(u, h // u.shape[0], 0), w // u.shape[1], 1)
        v = np.repeat(np.repeat(v, h // v.shape[0], 0), w // v.shape[1], 1)
        img = Image.fromarray(np.ascontiguousarray(np.stack([y, u, v], -1)), "YCbCr")
        sub = {YUV444: 0, YUV422: 1, YUV420: 2}[fmt]
    out = io.BytesIO()
    if tables is None:
        img.save(out, format="JPEG", quality=max(1, min(100, int(quality))), subsampling=sub)
        return out.getvalue()
    want = [[int(v) for v in t] for t in tables]
    img.save(out, format="JPEG", qtables=want, subsampling=sub)    # no quality: Pillow would scale the tables by it
    back = Image.open(io.BytesIO(out.getvalue())).quantization
    assert [list(back[0]), list(back[1])] == want, "Pillow did not write the tables as given"
    return out.getvalue()
