"""The files of the decoder's variant tests (tests/test_jpeg_decode_variants_host.py on the CPU,
tests/test_gpu_jpeg_decode_variants.py on the GPU): JPEGs as other encoders write them -- optimised, sparse and
hand-built Huffman tables, table ids and component ids of every kind, marker layouts with payloads that look like
markers, stuffed bytes and restart markers pinned to the unstuffer's chunk boundaries, restart-interval edges, a batch
of 300 and the ends of the dynamic range.  Every group is a list of Case(name, data, raw, pillow):
raw     the raw surface format the file decodes to besides RGB and Y (None: none)
pillow  True where libjpeg-turbo (Pillow) is the definition; False where only the numpy model is (the file is
        beyond the range in which libjpeg-turbo's C and SIMD paths agree)"""
from __future__ import annotations

import functools
import io
from collections import Counter, namedtuple
from pathlib import Path

import numpy as np

import jpeg_decode_files as jf
import jpeg_model as jm
import jpeg_stream_writer as sw

Case = namedtuple("Case", "name data raw pillow")
GOLDEN = Path(__file__).resolve().parent / "golden"
HV = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "440": (1, 2), "gray": (1, 1)}
RAW = {"444": "YUV444", "422": "YUV422", "420": "NV12"}
ONES = np.ones(64, np.int64)
DC_SYMBOLS = list(range(12))
AC_SYMBOLS = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]      # the 162 of baseline


def raw_of(sampling, w, h):
    """the raw format a w x h file of `sampling` decodes to (4:2:x surfaces have even sizes)"""
    if sampling == "422" and w % 2 == 0 or sampling == "420" and w % 2 == 0 and h % 2 == 0 or sampling == "444":
        return RAW[sampling]
    return None


@functools.lru_cache(maxsize=None)
def frame():
    from PIL import Image

    return np.asarray(Image.open(GOLDEN / "frame_0.jpg").convert("RGB"))


def q8(*tables):
    return {i: (0, t) for i, t in enumerate(tables)}


@functools.lru_cache(maxsize=None)
def noise_blocks(w, h, sampling, seed, quality=100):
    H, V = HV[sampling]
    tables = jm.quant_tables(quality)
    return sw.picture_blocks(jf.picture(w, h, "noise", seed), H, V, tables, sampling == "gray") + (H, V, tables)


def writer_file(w, h, sampling, seed, quality=100, **kw):
    coefs, comp, bpm, H, V, tables = noise_blocks(w, h, sampling, seed, quality)
    kw.setdefault("qtabs", q8(*tables))
    return sw.jpeg_file(w, h, coefs, comp, bpm, H=H, V=V, **kw)


# ---- a. optimised tables from Pillow ------------------------------------------------------------------------------------
def pillow_optimised(rgb, sampling, quality, restart_blocks=0, **kw):
    from PIL import Image

    out = io.BytesIO()
    if restart_blocks:
        kw["restart_marker_blocks"] = restart_blocks
    if sampling == "gray":
        Image.fromarray(rgb).convert("L").save(out, "JPEG", quality=quality, optimize=True, **kw)
    else:
        Image.fromarray(rgb).save(out, "JPEG", quality=quality, optimize=True, subsampling=jf._PIL_SUB[sampling], **kw)
    return out.getvalue()


A_SAMPLINGS = ("444", "422", "420", "gray")
A_SIZES = [(1, 1), (7, 9), (17, 33), (96, 64)]


@functools.lru_cache(maxsize=None)
def group_a(sampling):
    cases = []
    for w, h in A_SIZES:
        for q in (1, 50, 100):
            for restart in (False, True):
                rgb = jf.picture(w, h, "noise" if q == 100 else "frame", q + w, frame())
                data = pillow_optimised(rgb, sampling, q, 7 if restart else 0)
                cases.append(Case(f"opt {sampling} {w}x{h} q{q} rst{int(restart)}", data, raw_of(sampling, w, h), True))
    if sampling in ("422", "420"):                 # the odd sizes again as the even sizes their raw surfaces need
        for w, h in ((2, 2), (8, 10), (18, 34)):
            data = pillow_optimised(jf.picture(w, h, "frame", w, frame()), sampling, 50)
            cases.append(Case(f"opt {sampling} {w}x{h} q50 even", data, raw_of(sampling, w, h), True))
    flat = np.broadcast_to(np.array([200, 90, 30], np.uint8), (24, 40, 3)).copy()
    cases.append(Case(f"opt {sampling} flat 40x24", pillow_optimised(flat, sampling, 75), raw_of(sampling, 40, 24), True))
    return cases


# ---- b. hand-built tables -------------------------------------------------------------------------------------------------
B_VARIANTS = ("short", "deep", "sparse", "sof1 three pairs", "luma id 1 chroma id 0", "tq 3 0 2", "ids 0 1 2",
              "ids 10 20 30", "decoys", "one segment", "segment per table")
B_SAMPLINGS = ("420", "444")
B_SIZES = [(17, 33), (96, 64)]


def _merged(counts, comps):
    total = Counter()
    for c in comps:
        total.update(counts.get(c, {}))
    return total


def shaped_tables(coefs, comp, bpm, shape, groups=((0,), (1, 2))):
    """(dc, ac): {table id: spec} of one shape, table i for the components of groups[i]"""
    dcc, acc = sw.symbol_counts(coefs, comp, bpm)
    dc, ac = {}, {}
    for i, g in enumerate(groups):
        d, a = _merged(dcc, g), _merged(acc, g)
        if not d:
            continue                                   # gray: no chroma tables
        if shape == "sparse":
            dc[i], ac[i] = sw.sparse_spec(d), sw.sparse_spec(a)
        elif shape == "short":
            dc[i] = sw.table_spec(sw.by_frequency(d, DC_SYMBOLS), "short")
            ac[i] = sw.table_spec(sw.by_frequency(a, AC_SYMBOLS), "short")
        else:
            # the frequent symbols on the long codes, so that the lengths 10...16 carry most of the stream: DC in
            # reverse order, AC with the seven most frequent symbols on the lengths 9...15
            dc[i] = sw.table_spec(sw.by_frequency(d, DC_SYMBOLS)[::-1], "deep_dc")
            f = sw.by_frequency(a, AC_SYMBOLS)
            ac[i] = sw.table_spec(f[7:14] + f[:7] + f[14:], "deep_ac")
    return dc, ac


def variant_file(variant, w, h, sampling, seed, used=None):
    coefs, comp, bpm, H, V, tables = noise_blocks(w, h, sampling, seed)
    kw = dict(H=H, V=V, qtabs=q8(*tables), used=used)
    if variant in ("short", "deep", "sparse"):
        kw["dc"], kw["ac"] = shaped_tables(coefs, comp, bpm, variant)
    elif variant == "sof1 three pairs":
        per = [shaped_tables(coefs, comp, bpm, s, groups=((c,),)) for c, s in enumerate(("sparse", "short", "deep"))]
        kw.update(sof=0xC1, comps=[(1, 0, 2, 3), (2, 1, 0, 1), (3, 1, 3, 0)],
                  dc={2: per[0][0][0], 0: per[1][0][0], 3: per[2][0][0]},
                  ac={3: per[0][1][0], 1: per[1][1][0], 0: per[2][1][0]})
    elif variant == "luma id 1 chroma id 0":
        kw.update(comps=[(1, 0, 1, 1), (2, 1, 0, 0), (3, 1, 0, 0)], dc={1: jm.DC_LUMA, 0: jm.DC_CHROMA},
                  ac={1: jm.AC_LUMA, 0: jm.AC_CHROMA})
    elif variant == "tq 3 0 2":
        k = np.arange(64)
        kw.update(comps=[(1, 3, 0, 0), (2, 0, 1, 1), (3, 2, 1, 1)], qtabs={3: (0, ONES), 0: (0, 1 + k % 2), 2: (0, 1 + k % 3)})
    elif variant == "ids 0 1 2":
        kw["comps"] = [(0, 0, 0, 0), (1, 1, 1, 1), (2, 1, 1, 1)]
    elif variant == "ids 10 20 30":
        kw["comps"] = [(10, 0, 0, 0), (20, 1, 1, 1), (30, 1, 1, 1)]
    elif variant == "decoys":
        dc, ac = shaped_tables(coefs, comp, bpm, "sparse")
        kw.update(dc=dc, ac=ac, decoy_dqt={0: (1, 7 * ONES), 1: (0, 9 * ONES)},
                  decoy_dht={(0, 0): jm.DC_CHROMA, (1, 0): jm.AC_CHROMA, (0, 1): dc[0], (1, 1): ac[0]})
    elif variant == "segment per table":
        kw.update(split_dqt=True, split_dht=True)
    else:
        assert variant == "one segment"                    # the Annex K tables, as jpeg_model writes them
    return sw.jpeg_file(w, h, coefs, comp, bpm, **kw)


@functools.lru_cache(maxsize=None)
def group_b(variant, sampling):
    return [Case(f"{variant} {sampling} {w}x{h}", variant_file(variant, w, h, sampling, 3 + w), raw_of(sampling, w, h),
                 True) for w, h in B_SIZES]


# ---- c. marker layout -------------------------------------------------------------------------------------------------------
MARKER_BYTES = b"\xff\xd8\xff\xc4\x00\x05\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00\x12\xff\x00\x34\xff\xd0\xff\xd9"


def _pillow_c(seed, **kw):
    from PIL import Image

    out = io.BytesIO()
    Image.fromarray(jf.picture(40, 24, "frame", seed, frame())).save(out, "JPEG", quality=85, subsampling=2, **kw)
    return out.getvalue()


@functools.lru_cache(maxsize=None)
def group_c():
    thumb = jf.pillow_file(jf.picture(16, 8, "frame", 1, frame()), "420", 60)       # a whole JPEG inside the EXIF
    exif = b"Exif\x00\x00MM\x00\x2a\x00\x00\x00\x08\x00\x00" + thumb + MARKER_BYTES
    rng = np.random.default_rng(5)
    icc = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()
    icc = icc[:1000] + MARKER_BYTES + icc[1000:65500] + MARKER_BYTES + icc[65500:]
    com = b"comment " + MARKER_BYTES
    cases = [Case("pillow exif thumbnail", _pillow_c(1, exif=exif), "NV12", True),
             Case("pillow comment", _pillow_c(2, comment=com), "NV12", True),
             Case("pillow icc 70 KB", _pillow_c(3, icc_profile=icc), "NV12", True),
             Case("pillow exif comment icc", _pillow_c(4, exif=exif, comment=com, icc_profile=icc), "NV12", True)]
    extra = [(0xFE, MARKER_BYTES), (0xE1, exif), (0xEC, b"\xff" * 40 + MARKER_BYTES), (0xFE, b"")]
    cases += [Case("writer com holds a file", writer_file(40, 24, "420", 1, extra=extra), "NV12", True),
              Case("writer fill bytes", writer_file(40, 24, "420", 2, fill=3, extra=extra[:1], R=2), "NV12", True),
              Case("writer bytes after eoi", writer_file(40, 24, "444", 3, trailer=b"\x00\xff\xd8tail\xff\xda\xff"),
                   "YUV444", True),
              Case("writer fill and trailer gray", writer_file(40, 24, "gray", 4, fill=1, trailer=MARKER_BYTES), None, True)]
    return cases


@functools.lru_cache(maxsize=None)
def equal_header_pair():
    """two files with one header (EXIF with a thumbnail, a comment) and different entropy data"""
    exif_com = dict(exif=b"Exif\x00\x00" + MARKER_BYTES, comment=MARKER_BYTES)
    a, b = _pillow_c(7, **exif_com), _pillow_c(8, **exif_com)
    return a, b


# ---- d. unstuffer boundaries ------------------------------------------------------------------------------------------------
# (sampling, R, seed) found by search_unstuff_seeds(): between them the files have every property of unstuff_props()
UNSTUFF_FILES = (("444", 0, 0), ("444", 1, 1), ("gray", 1, 12), ("gray", 0, 14), ("gray", 1, 58), ("gray", 0, 131),
                 ("444", 1, 137))
UNSTUFF_PROPS = ("stuffed FF at 4095", "stuffed FF at 0", "stuffed FF at 0 mod 4", "stuffed FF at 1 mod 4",
                 "stuffed FF at 2 mod 4", "stuffed FF at 3 mod 4", "RST FF at 4095", "RST FF at 4094", "RST FF at 0",
                 "FF 00 FF 00")


def unstuff_file(sampling, R, seed):
    return writer_file(64, 64, sampling, seed, R=R)


def unstuff_props(data):
    """which unstuffer boundaries the entropy data of a file touches (offsets from its first byte; the decoder
    works in chunks of 4096 bytes, 4 bytes per lane)"""
    a, b = sw.entropy_bounds(data)
    e = data[a:b]
    got = set()
    x = 0
    while x < len(e):
        if e[x] != 0xFF:
            x += 1
            continue
        if e[x + 1] == 0:
            got.add(f"stuffed FF at {x % 4} mod 4")
            if x % 4096 in (0, 4095) and x > 0:
                got.add(f"stuffed FF at {x % 4096}")
            if e[x + 2:x + 4] == b"\xff\x00":
                got.add("FF 00 FF 00")
        elif x % 4096 in (0, 4094, 4095) and x > 0:
            got.add(f"RST FF at {x % 4096}")
        x += 2
    return got


def search_unstuff_seeds(limit=4000):
    """the search that gave UNSTUFF_FILES: the first seeds, per kind of file, that add a property not yet covered"""
    found, missing = [], set(UNSTUFF_PROPS)
    for seed in range(limit):
        for sampling, R in (("444", 0), ("444", 1), ("gray", 1), ("gray", 0)):
            new = unstuff_props(unstuff_file(sampling, R, seed)) & missing
            if new:
                found.append((sampling, R, seed))
                missing -= new
        noise_blocks.cache_clear()
        if not missing:
            break
    return found, missing


@functools.lru_cache(maxsize=None)
def group_d():
    return [Case(f"unstuff {s} R{R} seed {seed}", unstuff_file(s, R, seed), RAW.get(s), True) for s, R, seed in UNSTUFF_FILES]


# ---- e. restart-interval edges ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def group_e():
    cases = [Case(f"420 48x32 R{R}", writer_file(48, 32, "420", R, quality=90, R=R), "NV12", True) for R in (7, 3, 4, 65535)]
    cases.append(Case("420 48x32 DRI 5 then DRI 0", writer_file(48, 32, "420", 9, quality=90, R=0, dri=[5, 0]), "NV12", True))
    cases.append(Case("gray 80x8 R1", writer_file(80, 8, "gray", 10, quality=90, R=1), None, True))
    return cases


# ---- f. batch scale -----------------------------------------------------------------------------------------------------
BATCH = 300
BATCH_BAD = 271


@functools.lru_cache(maxsize=None)
def group_f():
    cases = []
    for i in range(BATCH):
        sampling = jf.SAMPLINGS[i % 5]
        w, h = 1 + (i * 7) % 24, 1 + (i * 5) % 16
        q = (30, 75, 95)[i % 3]
        if i % 2 == 0 and sampling != "440":
            data = jf.pillow_file(jf.picture(w, h, "noise", i), sampling, q, restart_blocks=(0, 3)[i // 2 % 2])
        else:
            coefs, comp, bpm, H, V, tables = noise_blocks(w, h, sampling, i, q)
            kw = {}
            if i % 3 == 0:
                kw["dc"], kw["ac"] = shaped_tables(coefs, comp, bpm, "sparse")
            data = sw.jpeg_file(w, h, coefs, comp, bpm, H=H, V=V, qtabs=q8(*tables), R=(0, 1, 2)[i % 3], **kw)
        cases.append(Case(f"batch {i} {sampling} {w}x{h}", data, None, True))
    return cases


def truncated_in_scan(data):
    a, b = sw.entropy_bounds(data)
    return data[:a + (b - a) // 2]


# ---- g. dynamic range -------------------------------------------------------------------------------------------------------
def rewrite_dqt16(data, mult=None, value=None):
    """the file with every quantisation table written with 16-bit values: multiplied by mult, or all = value"""
    out, i = bytearray(data[:2]), 2
    while True:
        marker, length = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        if marker == 0xDA:
            return bytes(out) + data[i:]
        body, new, o = data[i + 4:i + 2 + length], b"", 0
        if marker == 0xDB:
            while o < len(body):
                pq, tq = body[o] >> 4, body[o] & 15
                n = 64 * (pq + 1)
                vals = [int.from_bytes(body[o + 1 + (pq + 1) * k:o + 1 + (pq + 1) * (k + 1)], "big") for k in range(64)]
                vals = [value if value is not None else v * mult for v in vals]
                assert max(vals) <= 65535
                new += bytes([0x10 | tq]) + b"".join(v.to_bytes(2, "big") for v in vals)
                o += 1 + n
            out += b"\xff\xdb" + (len(new) + 2).to_bytes(2, "big") + new
        else:
            out += data[i:i + 2 + length]
        i += 2 + length


@functools.lru_cache(maxsize=None)
def range_fixture():
    """the 40 x 24 4:2:0 q50 file the boundary between libjpeg-turbo's C and SIMD paths is measured on"""
    return jf.pillow_file(jf.picture(40, 24, "frame", 6, frame()), "420", 50)


def saturated_pictures():
    yy, xx = np.mgrid[0:24, 0:40]
    rng = np.random.default_rng(17)
    return {"checkerboard 1": np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[..., None], 3, -1),
            "checkerboard 8": np.repeat(((((xx >> 3) + (yy >> 3)) & 1) * 255).astype(np.uint8)[..., None], 3, -1),
            "noise 0 255": (rng.integers(0, 2, (24, 40, 3)) * 255).astype(np.uint8)}


def saturated_file(name, sampling):
    """all-ones quantisation tables; coefficients above 1023 need AC sizes of 11, so the tables are the file's own"""
    H, V = HV[sampling]
    coefs, comp, bpm = sw.picture_blocks(saturated_pictures()[name], H, V, (ONES, ONES))
    dc, ac = shaped_tables(coefs, comp, bpm, "sparse")
    return sw.jpeg_file(40, 24, coefs, comp, bpm, H=H, V=V, qtabs=q8(ONES, ONES), dc=dc, ac=ac), int(np.abs(coefs).max())


def extreme_stream():
    """gray 16 x 8, two blocks: DC differences of size 11 (+2047, then -2047) and AC values of sizes 10 to 15, the
    int16 extremes among them"""
    coefs = np.zeros((2, 64), np.int64)
    coefs[0, 0], coefs[1, 0] = 2047, 0                                  # differences +2047 and -2047: size 11
    coefs[0, 1:7] = [1023, -2047, 4095, -8191, 16383, -32767]            # sizes 10 ... 15, largest of each
    coefs[1, 1:7] = [-512, 1024, -2048, 4096, -8192, 16384]              # sizes 10 ... 15, smallest of each
    coefs[0, 63], coefs[1, 40] = 32767, -16384
    comp = np.zeros(2, np.int64)
    dcc, acc = sw.symbol_counts(coefs, comp, 1)
    return sw.jpeg_file(16, 8, coefs, comp, 1, qtabs={0: (0, ONES)}, dc={0: sw.sparse_spec(dcc[0])},
                        ac={0: sw.sparse_spec(acc[0])})


@functools.lru_cache(maxsize=None)
def group_g():
    cases = []
    for name in saturated_pictures():
        for sampling in ("444", "420"):
            cases.append(Case(f"{name} {sampling} all-ones tables", saturated_file(name, sampling)[0], RAW[sampling], True))
    fx = range_fixture()
    cases += [Case("16-bit tables x3", rewrite_dqt16(fx, mult=3), "NV12", True),
              Case("16-bit tables x40", rewrite_dqt16(fx, mult=40), "NV12", False),
              Case("16-bit tables all 65535", rewrite_dqt16(fx, value=65535), "NV12", False),
              Case("extreme gray 16x8", extreme_stream(), None, False)]
    return cases
