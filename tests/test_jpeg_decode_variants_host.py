"""CPU side of the decoder's variant tests (the files of tests/jpeg_variant_files.py): the numpy model against Pillow's
libjpeg-turbo byte for byte on every kind of file, so that the GPU tests compare with a trusted reference;
vali_jpeg_parse against the model's reading of the header, down to every Huffman code through the tables the kernels
walk; PyNvJpegDecoder's header cache against the parser; and the range of quantisation values in which libjpeg-turbo's
C path (the decoder's definition) and its SIMD path (what Pillow runs) agree."""
import io

import numpy as np
import pytest

import jpeg_decode_model as dm
import jpeg_stream_writer as sw
import jpeg_variant_files as vf

GROUPS = {f"a {s}": (lambda s=s: vf.group_a(s)) for s in vf.A_SAMPLINGS}
GROUPS.update({f"b {v} {s}": (lambda v=v, s=s: vf.group_b(v, s)) for v in vf.B_VARIANTS for s in vf.B_SAMPLINGS})
GROUPS.update({"c": vf.group_c, "d": vf.group_d, "e": vf.group_e, "f": vf.group_f, "g": vf.group_g})
PILLOW_GROUPS = [g for g in GROUPS if g[0] in "acfg"]            # groups with files that Pillow wrote


def cases_of(group):
    if group in PILLOW_GROUPS:
        pytest.importorskip("PIL.Image")
    return GROUPS[group]()


def pillow_rgb(data):
    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def pillow_y(data):
    from PIL import Image

    im = Image.open(io.BytesIO(data))
    im.draft("L", im.size)
    return np.asarray(im.convert("L"))


def shim():
    from vali_amd._native import shim as s

    return s


# ---- the writer itself ----------------------------------------------------------------------------------------------------
def test_table_specs_have_the_shapes_they_are_named_for():
    ac = sw.table_spec(vf.AC_SYMBOLS, "short")
    assert sum(ac[0][9:]) == 0 and sum(ac[0]) == 162
    ac = sw.table_spec(vf.AC_SYMBOLS, "deep_ac")
    assert ac[0][1:15] == [1] * 14 and ac[0][15] == 162 - 14 and ac[0][0] == 0
    dc = sw.table_spec(vf.DC_SYMBOLS, "deep_dc")
    assert dc[0] == [0, 2, 3, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1]
    dc = sw.table_spec(vf.DC_SYMBOLS, "short")
    assert sum(dc[0][9:]) == 0 and sum(dc[0]) == 12
    assert sw.sparse_spec({5: 10}) == ([1] + [0] * 15, [5])
    assert sw.sparse_spec({5: 10, 0: 3}) == ([1, 1] + [0] * 14, [5, 0])
    # 200 symbols with Fibonacci-like counts: Huffman's lengths pass 16 bits and are limited
    counts = {s: int(1.5 ** min(s, 60)) + 1 for s in range(200)}
    bits, vals = sw.sparse_spec(counts)
    assert sum(bits) == 200 and sorted(vals) == list(range(200)) and bits[15] > 0
    for bad in (([2] + [0] * 15, [0, 1]), ([0, 4] + [0] * 14, [0, 1, 2, 3]), ([1, 1, 2] + [0] * 13, [0, 1, 2, 3])):
        with pytest.raises(AssertionError):
            sw.check_spec(bad)


def test_hand_built_files_read_codes_of_every_length():
    """the deep files of case b really use codes of each length 10...16, the short ones none above 9, and the
    sparse ones define nothing but what occurs"""
    used = {}
    vf.variant_file("deep", 96, 64, "444", 99, used)
    for comps in ((0,), (1, 2)):                                   # the components that share a table pair
        ac = sum((used[("ac", c)] for c in comps), vf.Counter())
        dc = sum((used[("dc", c)] for c in comps), vf.Counter())
        assert set(range(10, 17)) <= set(ac) and sum(ac[n] for n in range(10, 17)) > sum(ac.values()) // 2, ac
        assert max(dc) == 16 and len([n for n in dc if n >= 10]) >= 4, dc
    used = {}
    vf.variant_file("short", 96, 64, "444", 99, used)
    assert max(max(u) for u in used.values()) <= 9
    coefs, comp, bpm = vf.noise_blocks(96, 64, "444", 99)[:3]
    dcc, acc = sw.symbol_counts(coefs, comp, bpm)
    dc, ac = vf.shaped_tables(coefs, comp, bpm, "sparse")
    assert sorted(dc[0][1]) == sorted(dcc[0]) and sorted(ac[1][1]) == sorted(set(acc[1]) | set(acc[2]))


def test_flat_pictures_give_tables_of_one_or_two_symbols():
    pytest.importorskip("PIL.Image")
    for sampling in vf.A_SAMPLINGS:
        info = dm.parse(vf.group_a(sampling)[-1].data)
        sizes = sorted(len(t) for t in info["dc"] + info["ac"])
        assert sizes[0] == 1 and sizes[-1] <= 2, (sampling, sizes)


def test_unstuffer_files_touch_every_boundary():
    got = set()
    for case in vf.group_d():
        got |= vf.unstuff_props(case.data)
    assert got >= set(vf.UNSTUFF_PROPS), set(vf.UNSTUFF_PROPS) - got
    kinds = {(s, R) for s, R, _ in vf.UNSTUFF_FILES}
    assert kinds == {("444", 0), ("444", 1), ("gray", 0), ("gray", 1)}


def test_dynamic_range_files_reach_the_values_they_are_named_for():
    for sampling in ("444", "420"):
        assert vf.saturated_file("checkerboard 8", sampling)[1] == 1024          # the DC of a black block: -1024
        assert vf.saturated_file("checkerboard 1", sampling)[1] > 800            # the AC coefficient (7, 7)
    info = dm.parse(vf.extreme_stream())
    coefs = dm.entropy_decode(info)[0].reshape(-1, 64)
    assert coefs.max() == 32767 and coefs.min() == -32767 and coefs[0, 0] == 2047 and coefs[1, 0] == 0
    sizes = {s & 15 for s in info["ac"][0].values()}
    assert sizes >= set(range(10, 16)) and 11 in info["dc"][0].values()


# ---- the model against Pillow -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(GROUPS))
def test_model_equals_pillow(group):
    pytest.importorskip("PIL.Image")
    for case in cases_of(group):
        if case.pillow:
            assert np.array_equal(dm.decode(case.data, "RGB"), pillow_rgb(case.data)), case.name
            assert np.array_equal(dm.decode(case.data, "Y"), pillow_y(case.data)), case.name
        else:
            assert dm.decode(case.data, "RGB") is not None, case.name


def test_model_says_the_truncated_batch_file_is_corrupt():
    pytest.importorskip("PIL.Image")
    assert dm.decode(vf.truncated_in_scan(vf.group_f()[vf.BATCH_BAD].data)) is None


# ---- the parser against the model ---------------------------------------------------------------------------------------------
HUFF = np.dtype([("look", "<u2", 512), ("maxcode", "<i4", 18), ("valoff", "<i4", 18), ("vals", "u1", 256)])
INFO = np.dtype([("head", "<i4", 10), ("data_offset", "<u8"), ("data_len", "<u8"), ("qtable", "<u2", (3, 64)),
                 ("dc", HUFF, 3), ("ac", HUFF, 3)])


def huff_sym(t, w):
    """huff_sym of vali_amd/csrc/jpeg_decode.hip: (length, symbol) of the code at the top of the 32-bit word w"""
    e = int(t["look"][w >> 23])
    if e:
        return e >> 8, e & 255
    for length in range(10, 17):
        code = w >> (32 - length)
        if code <= int(t["maxcode"][length]):
            return length, int(t["vals"][(code + int(t["valoff"][length])) & 255])
    return 0, 0


def check_tables(parsed, model_table, name):
    for code, sym in model_table.items():
        n = len(code)
        top = int(code, 2) << (32 - n)
        for w in (top, top | ((1 << (32 - n)) - 1), top | (0x55555555 >> n)):
            assert huff_sym(parsed, w) == (n, sym), (name, code)
    if not any(set(c) == {"1"} and len(c) == 16 for c in model_table):
        assert huff_sym(parsed, 0xFFFFFFFF)[0] == 0, name           # the all-ones code is never a code


@pytest.mark.parametrize("group", list(GROUPS))
def test_parser_gives_the_models_geometry_and_tables(group):
    s = shim()
    assert INFO.itemsize == s.JPEG_INFO_SIZE
    for case in cases_of(group):
        want = dm.parse(case.data)
        got = s.jpeg_parse(case.data)
        mcux, mcuy, bpm = dm.geometry(want)
        assert (got.width, got.height, got.components, got.mcux, got.mcuy) == (want["w"], want["h"], want["nc"], mcux,
                                                                             mcuy), case.name
        assert (got.h_samp, got.v_samp, got.restart_interval) == (want["H"], want["V"], want["ri"]), case.name
        assert got.segments == (-(-(mcux * mcuy) // want["ri"]) if want["ri"] else 1), case.name
        assert case.data[got.data_offset:got.data_offset + got.data_len] == want["data"], case.name
        raw = np.frombuffer(got.tobytes(), INFO)[0]
        assert int(raw["head"][8]) == bpm
        for c in range(want["nc"]):
            assert np.array_equal(raw["qtable"][c], want["q"][c]), (case.name, c)
            check_tables(raw["dc"][c], want["dc"][c], (case.name, "dc", c))
            check_tables(raw["ac"][c], want["ac"][c], (case.name, "ac", c))


# ---- the header cache against the parser ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(GROUPS))
def test_header_cache_gives_what_the_parser_gives(vali, group):
    from vali_amd import codecs

    s = shim()
    dec = vali.PyNvJpegDecoder.__new__(vali.PyNvJpegDecoder)
    dec._headers = {}
    files = [c.data for c in cases_of(group)]
    if group == "c":
        files += list(vf.equal_header_pair())
    if group == "f":
        files.append(vf.truncated_in_scan(files[vf.BATCH_BAD]))
    for turn in range(2):                                   # the second turn finds every header in the cache
        for k, f in enumerate(files):
            a = np.frombuffer(f, np.uint8)
            want = s.jpeg_parse(f)
            assert dec._parse(a).tobytes() == want.tobytes(), (group, k, turn)
            assert codecs._sos_end(a) == want.data_offset, (group, k)
            assert codecs._entropy_len(a, int(want.data_offset)) == want.data_len, (group, k)
    assert 1 <= len(dec._headers) <= len(files)
    if group == "c":
        a, b = vf.equal_header_pair()
        ia, ib = s.jpeg_parse(a), s.jpeg_parse(b)
        assert a[:ia.data_offset] == b[:ib.data_offset] and a[ia.data_offset:] != b[ib.data_offset:]
        assert len(dec._headers) == len(files) - 1           # the pair shares one entry


# ---- where libjpeg-turbo's two paths part ---------------------------------------------------------------------------------------
def test_model_equals_pillow_up_to_three_times_the_q50_tables():
    """The decoder's definition is libjpeg-turbo's C path (jidctint.c: the dequantised coefficient is an int); Pillow
    runs the SIMD path, which keeps dequantised coefficients and their first sums in 16-bit lanes.  The two agree while
    those stay within 16 bits.  On the 40 x 24 4:2:0 q50 fixture with its tables rewritten as 16-bit values and
    multiplied, this sweep prints the largest multiplier up to which they agree (measured: x3, largest table value
    363; x4 and everything above differs) and asserts exactly that part, x1 ... x3, never the inequality, which depends
    on the CPU's SIMD path."""
    pytest.importorskip("PIL.Image")
    fx = vf.range_fixture()
    assert max(int(t.max()) for t in dm.parse(fx)["q"]) == 121
    equal = []
    for mult in range(1, 41):
        f = vf.rewrite_dqt16(fx, mult=mult)
        equal.append(np.array_equal(dm.decode(f), pillow_rgb(f)) and np.array_equal(dm.decode(f, "Y"), pillow_y(f)))
    agree = equal.index(False) if False in equal else len(equal)
    print(f"model == Pillow for every multiplier up to x{agree}; equal at {[m + 1 for m, e in enumerate(equal) if e]}")
    assert all(equal[:3]), equal[:3]
