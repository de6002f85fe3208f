"""A baseline JPEG stream writer for the decoder tests only: quantised coefficient blocks in, a complete file out, with
every choice an encoder has left to the caller -- Huffman tables of any legal shape per component, quantisation tables
of 8 or 16 bits, SOF0 / SOF1, component ids, Tq / Td / Ta, how the tables are split over DQT / DHT segments (decoy
definitions that a later segment overrides included), DRI (a later DRI overriding an earlier one included), extra
APPn / COM segments, FF fill bytes before header markers and bytes after EOI.  Its files do not depend on Pillow.

Blocks are what jpeg_model.scan_blocks gives: (N, 64) coefficients in zigzag order, MCU-interleaved, and the
component (0, 1, 2) of every block.  A table spec is (BITS[1..16], HUFFVAL) as in a DHT segment."""
from __future__ import annotations

import heapq
from collections import Counter

import numpy as np

import jpeg_model as jm

ANNEX_K_DC = {0: jm.DC_LUMA, 1: jm.DC_CHROMA}
ANNEX_K_AC = {0: jm.AC_LUMA, 1: jm.AC_CHROMA}
DEFAULT_COMPS = ((1, 0, 0, 0), (2, 1, 1, 1), (3, 1, 1, 1))          # (component id, Tq, Td, Ta)


# ---- table specs ----------------------------------------------------------------------------------------------------------
def check_spec(spec):
    """a spec a baseline decoder must accept: canonical codes of 1..16 bits that are prefix-free (Kraft sum below 1:
    the all-ones code of the longest length stays free), every symbol once"""
    bits, vals = spec
    assert len(bits) == 16 and sum(bits) == len(vals) and 1 <= len(vals) <= 256
    assert len(set(vals)) == len(vals) and all(0 <= v <= 255 for v in vals)
    code = 0
    for length in range(1, 17):
        code += bits[length - 1]
        assert code < (1 << length), "oversubscribed, or the all-ones code is in use"
        code <<= 1
    return list(bits), list(vals)


def spec_from_lengths(symbols, lengths):
    """symbols[i] gets a code of lengths[i] bits"""
    order = sorted(range(len(symbols)), key=lambda i: (lengths[i], i))
    bits = [0] * 16
    for i in order:
        bits[lengths[i] - 1] += 1
    return check_spec((bits, [symbols[i] for i in order]))


def table_spec(symbols, shape):
    """a valid spec for `symbols` (most frequent first):
    "short"    every code at most 9 bits: lengths 2, 3, ..., 8, then 9 for the rest;
    "deep_ac"  one code at each length 2...15, the rest at 16 (at least 15 symbols);
    "deep_dc"  five short codes (2, 2, 3, 3, 3), one at each of 10...16, the rest at 16 (at least 12 symbols)"""
    n = len(symbols)
    if shape == "short":
        lengths = [min(i + 2, 9) for i in range(n)]
    elif shape == "deep_ac":
        assert n >= 15
        lengths = [min(i + 2, 16) for i in range(n)]
    elif shape == "deep_dc":
        assert n >= 12
        lengths = ([2, 2, 3, 3, 3] + list(range(10, 17)) + [16] * (n - 12))
    else:
        raise ValueError(shape)
    return spec_from_lengths(list(symbols), lengths)


def sparse_spec(counts):
    """only the symbols that occur (counts: symbol -> occurrences), with the code lengths of ITU T.81 K.2: Huffman's
    algorithm with one reserved code point, so that no code is all ones, then limited to 16 bits"""
    freq = {int(s): int(c) for s, c in counts.items() if c > 0}
    assert freq
    heap = [(c, s, (s,)) for s, c in freq.items()] + [(0, 256, (256,))]      # 256: the reserved point, rarest
    heapq.heapify(heap)
    size = Counter()
    while len(heap) > 1:
        c1, s1, m1 = heapq.heappop(heap)
        c2, s2, m2 = heapq.heappop(heap)
        for s in m1 + m2:
            size[s] += 1
        heapq.heappush(heap, (c1 + c2, max(s1, s2), m1 + m2))
    bits = [0] * (max(size.values()) + 2)
    for s in size:
        bits[size[s]] += 1
    for i in range(len(bits) - 1, 16, -1):                                     # K.3: no code longer than 16 bits
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = max(k for k in range(len(bits)) if bits[k])
    bits[i] -= 1                                                               # the reserved point leaves
    vals = sorted((s for s in size if s != 256), key=lambda s: (size[s], s))
    b16 = bits[1:17]
    return check_spec((b16 + [0] * (16 - len(b16)), vals))


# ---- entropy coding -------------------------------------------------------------------------------------------------------
def _events(coefs, comp, bpm, R):
    """the scan as ("rst", n) and (component, "dc" | "ac", symbol, value, size) events (jchuff encode_one_block)"""
    pred = [0, 0, 0]
    for m in range(len(coefs) // bpm):
        if R and m and m % R == 0:
            yield ("rst", (m // R - 1) % 8)
            pred = [0, 0, 0]
        for b in range(m * bpm, (m + 1) * bpm):
            c, z = int(comp[b]), coefs[b]
            diff = int(z[0]) - pred[c]
            pred[c] = int(z[0])
            s = abs(diff).bit_length()
            yield (c, "dc", s, diff, s)
            last = 0
            for k in np.flatnonzero(z[1:]) + 1:
                run = int(k) - last - 1
                while run > 15:
                    yield (c, "ac", 0xF0, 0, 0)
                    run -= 16
                v = int(z[k])
                s = abs(v).bit_length()
                yield (c, "ac", (run << 4) | s, v, s)
                last = int(k)
            if last < 63:
                yield (c, "ac", 0x00, 0, 0)


def symbol_counts(coefs, comp, bpm, R=0):
    """({component: Counter of DC symbols}, {component: Counter of AC symbols}) of the scan"""
    dc, ac = {}, {}
    for ev in _events(coefs, comp, bpm, R):
        if ev[0] != "rst":
            (dc if ev[1] == "dc" else ac).setdefault(ev[0], Counter())[ev[2]] += 1
    return dc, ac


def by_frequency(counter, universe=()):
    """the symbols that occur, most frequent first, then the rest of `universe` in order"""
    seen = [s for s, _ in sorted(counter.items(), key=lambda kv: (-kv[1], kv[0]))]
    return seen + [s for s in universe if s not in counter]


def entropy(coefs, comp, bpm, R, dc_specs, ac_specs, used=None):
    """the entropy-coded data; dc_specs / ac_specs: one spec per component.  used (a dict) receives, per
    ("dc" | "ac", component), the Counter of the code lengths written"""
    dc = [jm.huff_codes(s) for s in dc_specs]
    ac = [jm.huff_codes(s) for s in ac_specs]
    bits = jm._Bits()
    for ev in _events(coefs, comp, bpm, R):
        if ev[0] == "rst":
            bits.flush()
            bits.out += bytes([0xFF, 0xD0 + ev[1]])
            continue
        c, kind, sym, v, s = ev
        code, length = (dc if kind == "dc" else ac)[c][sym]
        bits.put(code, length)
        if s:
            bits.put(v if v >= 0 else v - 1, s)
        if used is not None:
            used.setdefault((kind, c), Counter())[length] += 1
    bits.flush()
    return bytes(bits.out)


# ---- file ---------------------------------------------------------------------------------------------------------------
def _qt_entry(tq, table):
    precision, values = table
    v = [int(x) for x in np.asarray(values).reshape(64)[jm.ZIGZAG]]
    if precision:
        return bytes([0x10 | tq]) + b"".join(x.to_bytes(2, "big") for x in v)
    return bytes([tq]) + bytes(v)


def _ht_entry(cls, th, spec):
    bits, vals = check_spec(spec)
    return bytes([(cls << 4) | th]) + bytes(bits) + bytes(vals)


def jpeg_file(w, h, coefs, comp, bpm, *, H=1, V=1, qtabs, dc=None, ac=None, comps=None, sof=0xC0, R=0, dri=None,
              split_dqt=False, split_dht=False, decoy_dqt=None, decoy_dht=None, extra=(), fill=0, trailer=b"",
              used=None):
    """A complete file.
    coefs, comp, bpm  the blocks (see the module docstring); one component (gray) when bpm == 1 and H == V == 1
    H, V              luma sampling factors
    qtabs             {Tq: (precision 0 | 1, 64 values in natural order)}
    dc, ac            {table id: spec}; Annex K tables on ids 0 and 1 by default
    comps             (component id, Tq, Td, Ta) per component
    sof               0xC0 or 0xC1
    R, dri            restart interval of the entropy data; dri: the DRI segments written, in order (the last one must
                      give R; default: one DRI when R > 0)
    split_dqt / dht   one segment per table instead of one segment for all of them
    decoy_dqt / dht   {Tq: table} / {(class, id): spec} written in a segment of their own BEFORE the real definitions
    extra             (marker, payload) segments between APP0 and the tables
    fill              FF fill bytes in front of every header marker after SOI
    trailer           bytes after EOI"""
    gray = bpm == 1
    dc = dict(ANNEX_K_DC) if dc is None else dc
    ac = dict(ANNEX_K_AC) if ac is None else ac
    comps = list(DEFAULT_COMPS[:1] if gray else DEFAULT_COMPS) if comps is None else list(comps)
    assert len(comps) == (1 if gray else 3)
    dri = ([R] if R else []) if dri is None else list(dri)
    assert (dri[-1] if dri else 0) == R

    def seg(marker, payload):
        assert len(payload) + 2 <= 65535
        return b"\xff" * fill + bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)

    def grouped(entries, split):
        return [e for e in entries] if split else [b"".join(entries)]

    out = b"\xff\xd8" + seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for marker, payload in extra:
        out += seg(marker, payload)
    if decoy_dqt:
        out += seg(0xDB, b"".join(_qt_entry(tq, t) for tq, t in sorted(decoy_dqt.items())))
    for part in grouped([_qt_entry(tq, t) for tq, t in sorted(qtabs.items())], split_dqt):
        out += seg(0xDB, part)
    frame = bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([len(comps)])
    for i, (cid, tq, _, _) in enumerate(comps):
        frame += bytes([cid, ((H << 4) | V) if i == 0 and not gray else 0x11, tq])
    out += seg(sof, frame)
    if decoy_dht:
        out += seg(0xC4, b"".join(_ht_entry(cls, th, s) for (cls, th), s in sorted(decoy_dht.items())))
    tables = [_ht_entry(0, th, s) for th, s in sorted(dc.items())] + [_ht_entry(1, th, s) for th, s in sorted(ac.items())]
    for part in grouped(tables, split_dht):
        out += seg(0xC4, part)
    for r in dri:
        out += seg(0xDD, int(r).to_bytes(2, "big"))
    scan = bytes([len(comps)])
    for cid, _, td, ta in comps:
        scan += bytes([cid, (td << 4) | ta])
    out += seg(0xDA, scan + bytes([0, 63, 0]))
    body = entropy(coefs, comp, bpm, R, [dc[c[2]] for c in comps], [ac[c[3]] for c in comps], used)
    return out + body + b"\xff\xd9" + bytes(trailer)


# ---- blocks from pictures -----------------------------------------------------------------------------------------------
def picture_blocks(rgb, H, V, tables, gray=False):
    """(coefs, comp, bpm) of an (h, w, 3) u8 picture: jpeg_model's colour conversion, FDCT and quantisation by
    `tables` = (luma, chroma) in natural order; chroma subsampled by taking every H-th / V-th sample"""
    h, w = rgb.shape[:2]
    y, u, v = jm.rgb_to_ycc(rgb)
    if gray:
        H = V = 1
    cw, ch = -(-w // H), -(-h // V)
    planes = [y, u[::V, ::H][:ch, :cw], v[::V, ::H][:ch, :cw]]
    coefs, comp, bpm = jm.scan_blocks(jm.YUV444, planes, w, h, None, tables=tables, samp=(H, V))
    if gray:
        keep = comp == 0
        return coefs[keep], comp[keep], 1
    return coefs, comp, bpm


def entropy_bounds(data):
    """(start, end) of the entropy-coded data of a file with one scan: after the SOS segment, up to the EOI marker"""
    i = 2
    while True:
        while data[i] == 0xFF:
            i += 1
        marker, length = data[i], int.from_bytes(data[i + 1:i + 3], "big")
        i += 1 + length
        if marker == 0xDA:
            break
    x = i
    while not (data[x] == 0xFF and data[x + 1] == 0xD9):
        x += 2 if data[x] == 0xFF else 1
    return i, x
