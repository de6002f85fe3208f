"""numpy restatement of the baseline JPEG decoder of include/vali_hip.h (vali_jpeg_decode_batch), for the tests only.

Every stage follows libjpeg-turbo's default decompression (what Pillow's Image.open(...).convert(...) gives): Huffman
decoding (jdhuff), DC prediction restarting at every restart marker, dequantisation and the accurate integer IDCT
"islow" (jidctint) with jdmaster's post-IDCT range-limit table, fancy upsampling (jdsample: h2v1 / h2v2 triangle
filters when the chroma width exceeds 2, replication otherwise, h1v2 triangle filter; rows replicated at the top and
bottom) and the fixed-point ycc_rgb_convert of jdcolor.  tests/test_jpeg_decode_host.py pins it to Pillow.

Corrupt entropy data (the decoder's definition, stricter than libjpeg's recovery): an invalid Huffman code, a run
past coefficient 63, a code word running past the end of its restart segment, a segment that ends before its last
MCU, an FF followed by anything but 00 or the expected RSTn, a wrong number of RSTn markers.  decode() returns None.
"""
from __future__ import annotations

import functools

import numpy as np

from jpeg_model import ZIGZAG

NATURAL = ZIGZAG                       # natural index of zigzag position k


class Unsupported(ValueError):
    pass


def parse(data: bytes) -> dict:
    """the header fields the decoder uses (supported files only; Unsupported otherwise)"""
    d = bytes(data)
    assert d[:2] == b"\xff\xd8"
    qt, ht, ri, i = {}, {}, 0, 2
    frame = None
    while True:
        assert d[i] == 0xFF, i
        while d[i] == 0xFF:
            i += 1
        mk = d[i]
        ln = (d[i + 1] << 8) | d[i + 2]
        p = d[i + 3:i + 1 + ln]
        i += 1 + ln
        if mk in (0xC0, 0xC1):
            if p[0] != 8:
                raise Unsupported("precision")
            h, w, nc = (p[1] << 8) | p[2], (p[3] << 8) | p[4], p[5]
            frame = dict(w=w, h=h, comps=[(p[6 + 3 * c], p[7 + 3 * c] >> 4, p[7 + 3 * c] & 15, p[8 + 3 * c])
                                          for c in range(nc)])
        elif mk in (0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCC, 0xCD, 0xCE, 0xCF, 0xDC):
            raise Unsupported(hex(mk))
        elif mk == 0xC4:
            o = 0
            while o < len(p):
                bits = list(p[o + 1:o + 17])
                n = sum(bits)
                ht[(p[o] >> 4, p[o] & 15)] = (bits, list(p[o + 17:o + 17 + n]))
                o += 17 + n
        elif mk == 0xDB:
            o = 0
            while o < len(p):
                pq, tq = p[o] >> 4, p[o] & 15
                if pq:
                    v = [(p[o + 1 + 2 * k] << 8) | p[o + 2 + 2 * k] for k in range(64)]
                else:
                    v = list(p[o + 1:o + 65])
                t = np.zeros(64, np.int64)
                t[NATURAL] = v
                qt[tq] = t
                o += 1 + 64 * (pq + 1)
        elif mk == 0xDD:
            ri = (p[0] << 8) | p[1]
        elif mk == 0xDA:
            ns = p[0]
            tabs = [(p[2 + 2 * c] >> 4, p[2 + 2 * c] & 15) for c in range(ns)]
            break
    comps = frame["comps"]
    nc = len(comps)
    if nc == 1:
        H = V = 1
    else:
        H, V = comps[0][1], comps[0][2]
    start = i
    end = len(d)
    for x in range(start, len(d) - 1):
        if d[x] == 0xFF and d[x + 1] != 0 and not 0xD0 <= d[x + 1] <= 0xD7:
            end = x
            break
    return dict(w=frame["w"], h=frame["h"], nc=nc, H=H, V=V, ri=ri,
                q=[qt[c[3]] for c in comps],
                dc=[_huff_table(*ht[(0, t[0])]) for t in tabs], ac=[_huff_table(*ht[(1, t[1])]) for t in tabs],
                data=d[start:end])


def _huff_table(bits, vals):
    """Annex C: {bit string: symbol}"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[format(code, f"0{length}b")] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return out


def geometry(info):
    H, V, nc = info["H"], info["V"], info["nc"]
    if nc == 1:
        mcux, mcuy, bpm = -(-info["w"] // 8), -(-info["h"] // 8), 1
    else:
        mcux, mcuy, bpm = -(-info["w"] // (8 * H)), -(-info["h"] // (8 * V)), H * V + 2
    return mcux, mcuy, bpm


def segments(data: bytes, nseg: int):
    """unstuffed bytes of every restart segment, or None when the markers are corrupt"""
    segs, cur, m, x, n = [], bytearray(), 0, 0, len(data)
    while x < n:
        b = data[x]
        if b != 0xFF:
            cur.append(b)
            x += 1
            continue
        if x + 1 >= n:
            return None
        nx = data[x + 1]
        if nx == 0:
            cur.append(0xFF)
        elif 0xD0 <= nx <= 0xD7:
            if (nx & 7) != (m & 7):
                return None
            m += 1
            segs.append(bytes(cur))
            cur = bytearray()
        else:
            return None
        x += 2
    segs.append(bytes(cur))
    return segs if len(segs) == nseg else None


def entropy_decode(info):
    """(list of (bh, bw, 64) natural-order coefficient arrays per component, MCU-padded), or None when corrupt"""
    mcux, mcuy, bpm = geometry(info)
    H, V, nc = info["H"], info["V"], info["nc"]
    nmcu = mcux * mcuy
    R = info["ri"] or nmcu
    nseg = -(-nmcu // R)
    segs = segments(info["data"], nseg)
    if segs is None:
        return None
    comp_of = [0] * (H * V) + [1, 2] if nc == 3 else [0]
    blocks = np.zeros((nmcu * bpm, 64), np.int64)
    b = 0
    for s, seg in enumerate(segs):
        bits = "".join(format(x, "08b") for x in seg)
        nb, p = len(bits), 0
        pred = [0, 0, 0]
        for _ in range(min(R, nmcu - s * R)):
            for pos in range(bpm):
                c = comp_of[pos]
                blk = blocks[b]
                k = 0
                while k < 64:
                    tab = info["dc"][c] if k == 0 else info["ac"][c]
                    sym = None
                    for ln in range(1, 17):
                        if p + ln > nb:
                            return None              # runs past the segment's end
                        sym = tab.get(bits[p:p + ln])
                        if sym is not None:
                            break
                    if sym is None:
                        return None                  # invalid code
                    p += ln
                    r, sz = (0, sym) if k == 0 else (sym >> 4, sym & 15)
                    v = 0
                    if sz:
                        if p + sz > nb:
                            return None
                        e = int(bits[p:p + sz], 2)
                        p += sz
                        v = e - (1 << sz) + 1 if e < (1 << (sz - 1)) else e
                    if k == 0:
                        pred[c] += v
                        blk[0] = ((pred[c] + 32768) & 0xFFFF) - 32768      # JCOEF cast of the int predictor
                        k = 1
                    elif sz:
                        if k + r > 63:
                            return None              # run past 63
                        blk[NATURAL[k + r]] = v
                        k += r + 1
                    elif r == 15:
                        if k + 16 > 64:
                            return None
                        k += 16
                    else:
                        k = 64                        # EOB
                b += 1
    # scatter the MCU-ordered blocks into per-component block grids
    out = []
    for c in range(nc):
        hs, vs = (H, V) if c == 0 else (1, 1)
        out.append(np.zeros((mcuy * vs, mcux * hs, 64), np.int64))
    for m in range(nmcu):
        mx, my = m % mcux, m // mcux
        for pos in range(bpm):
            c = comp_of[pos]
            if c == 0 and nc == 3:
                out[0][my * V + pos // H, mx * H + pos % H] = blocks[m * bpm + pos]
            elif c == 0:
                out[0][my, mx] = blocks[m]
            else:
                out[c][my, mx] = blocks[m * bpm + pos]
    return out


# ---- IDCT -----------------------------------------------------------------------------------------------------------------
F = dict(c0298=2446, c0390=3196, c0541=4433, c0765=6270, c0899=7373, c1175=9633, c1501=12299, c1847=15137,
         c1961=16069, c2053=16819, c2562=20995, c3072=25172)


def _idct_1d(x, sh):
    """one jidctint pass over the last axis (JLONG arithmetic), DESCALE by sh"""
    s = [x[..., i] for i in range(8)]
    z2, z3 = s[2], s[6]
    z1 = (z2 + z3) * F["c0541"]
    tmp2, tmp3 = z1 - z3 * F["c1847"], z1 + z2 * F["c0765"]
    tmp0, tmp1 = (s[0] + s[4]) << 13, (s[0] - s[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = s[7], s[5], s[3], s[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F["c1175"]
    t0, t1, t2, t3 = t0 * F["c0298"], t1 * F["c2053"], t2 * F["c3072"], t3 * F["c1501"]
    z1, z2 = -z1 * F["c0899"], -z2 * F["c2562"]
    z3, z4 = -z3 * F["c1961"] + z5, -z4 * F["c0390"] + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    half = 1 << (sh - 1)
    o = [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]
    return np.stack([(v + half) >> sh for v in o], -1)


def range_limit(x):
    """jdmaster's post-IDCT table indexed by x & RANGE_MASK (1023)"""
    u = np.asarray(x, np.int64) & 1023
    return np.where(u < 128, u + 128, np.where(u < 512, 255, np.where(u < 896, 0, u - 896))).astype(np.uint8)


def idct_plane(blocks, q):
    """(bh, bw, 64) coefficients -> (bh * 8, bw * 8) u8 samples"""
    bh, bw = blocks.shape[:2]
    qs = np.asarray(q, np.int64)
    qs = ((qs + 32768) & 0xFFFF) - 32768                      # ISLOW_MULT_TYPE is a short
    d = (blocks.reshape(-1, 8, 8) * qs.reshape(8, 8)).astype(np.int64)
    d = _idct_1d(d.transpose(0, 2, 1), 11).transpose(0, 2, 1)             # columns
    d = ((d + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)                         # int workspace
    d = _idct_1d(d, 18)                                                     # rows
    s = range_limit(d)
    return s.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def component_planes(info):
    """MCU-padded u8 planes of every component, or None when the entropy data is corrupt"""
    coefs = entropy_decode(info)
    if coefs is None:
        return None
    return [idct_plane(c, info["q"][i]) for i, c in enumerate(coefs)]


def component_sizes(info):
    H, V, w, h = info["H"], info["V"], info["w"], info["h"]
    if info["nc"] == 1:
        return [(w, h)]
    return [(w, h)] + [(-(-w // H), -(-h // V))] * 2


# ---- upsampling + colour -----------------------------------------------------------------------------------------------------
def upsample(plane, cw, ch, H, V, w, h):
    """jdsample for one chroma plane (cw x ch real samples) -> h x w"""
    p = plane.astype(np.int64)
    xs, ys = np.arange(w), np.arange(h)
    if (H, V) == (1, 1):
        return p[:h, :w]
    if (H, V) == (2, 1):
        i = xs >> 1
        if cw <= 2:
            return p[:h, i]
        nb = np.where(xs & 1, np.minimum(i + 1, cw - 1), np.maximum(i - 1, 0))
        return np.where(xs & 1, (3 * p[:h, i] + p[:h, nb] + 2) >> 2, (3 * p[:h, i] + p[:h, nb] + 1) >> 2)
    if (H, V) == (1, 2):
        r = ys >> 1
        nr = np.where(ys & 1, np.minimum(r + 1, ch - 1), np.maximum(r - 1, 0))
        return (3 * p[r][:, :w] + p[nr][:, :w] + np.where(ys & 1, 2, 1)[:, None]) >> 2
    r, i = ys >> 1, xs >> 1
    if cw <= 2:
        return p[r][:, i]
    nr = np.where(ys & 1, np.minimum(r + 1, ch - 1), np.maximum(r - 1, 0))
    cs = 3 * p[r] + p[nr]                                  # (h, padded width) column sums
    ni = np.where(xs & 1, np.minimum(i + 1, cw - 1), np.maximum(i - 1, 0))
    return np.where(xs & 1, (3 * cs[:, i] + cs[:, ni] + 7) >> 4, (3 * cs[:, i] + cs[:, ni] + 8) >> 4)


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = (np.asarray(a, np.int64) for a in (y, cb, cr))
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=4)
def _parsed_planes(data: bytes):
    """(info, component planes) of a file; kept for the next outputs asked of the same file (nothing writes to them)"""
    info = parse(data)
    return info, component_planes(info)


def decode(data, out="RGB"):
    """out: "RGB" -> (h, w, 3); "Y" -> (h, w); "planes" -> the component planes cropped to the image.
    None when the entropy data is corrupt."""
    info, planes = _parsed_planes(bytes(data))
    if planes is None:
        return None
    w, h = info["w"], info["h"]
    sizes = component_sizes(info)
    if out == "planes":
        return [pl[:ch, :cw] for pl, (cw, ch) in zip(planes, sizes)]
    y = planes[0][:h, :w]
    if out == "Y":
        return y
    if info["nc"] == 1:
        return np.repeat(y[..., None], 3, -1)
    cw, ch = sizes[1]
    cb = upsample(planes[1], cw, ch, info["H"], info["V"], w, h)
    cr = upsample(planes[2], cw, ch, info["H"], info["V"], w, h)
    return ycc_to_rgb(y, cb, cr)


def surface_bytes(data, fmt_name):
    """the tightly packed host image (Surface.HostSize layout) vali_jpeg_decode_batch writes for `fmt_name`"""
    if fmt_name in ("RGB", "BGR", "RGB_PLANAR"):
        rgb = decode(data, "RGB")
        if rgb is None:
            return None
        if fmt_name == "BGR":
            rgb = rgb[..., ::-1]
        if fmt_name == "RGB_PLANAR":
            rgb = rgb.transpose(2, 0, 1)
        return np.ascontiguousarray(rgb).reshape(-1)
    if fmt_name == "Y":
        y = decode(data, "Y")
        return None if y is None else y.reshape(-1)
    pl = decode(data, "planes")
    if pl is None:
        return None
    if fmt_name == "NV12":
        uv = np.empty((pl[1].shape[0], 2 * pl[1].shape[1]), np.uint8)
        uv[:, 0::2], uv[:, 1::2] = pl[1], pl[2]
        return np.concatenate([pl[0].reshape(-1), uv.reshape(-1)])
    return np.concatenate([p.reshape(-1) for p in pl])
