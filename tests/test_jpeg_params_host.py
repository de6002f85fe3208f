"""The inputs of tests/jpeg_encoder_inputs.py do what they are named for, on the CPU: the model stays pinned to Pillow's
libjpeg under custom quantisation tables, the symbol images emit every Huffman symbol of all four tables, every boundary
seed puts its 0xFF or its segment length where the name says, and the host-only C entry points take custom tables and
restart intervals through the shim's setters."""
import io

import numpy as np
import pytest

import jpeg_encoder_inputs as ji
import jpeg_model as jm

PIL = pytest.importorskip("PIL.Image")


@pytest.fixture(scope="module")
def shim():
    from vali_amd._native import shim

    return shim


def as_lists(tables):
    return [[int(v) for v in t] for t in tables]


# ---- the model against Pillow, custom tables -----------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [jm.RGB, jm.YUV420], ids=["RGB", "YUV420"])
@pytest.mark.parametrize("name", list(ji.TABLES))
def test_model_equals_pillow_with_custom_tables(name, fmt):
    w, h = 46, 26
    for content in ("noise", "binary"):
        host = ji.content_host(fmt, content, w, h, seed=3)
        want = jm.entropy_of_file(jm.pillow_encode(fmt, host, w, h, 0, tables=ji.TABLES[name]))
        assert jm.entropy(fmt, host, w, h, 0, R=0, tables=ji.TABLES[name]) == want, content


@pytest.mark.parametrize("kind", ji.SYMBOL_KINDS)
def test_model_equals_pillow_on_the_symbol_images(kind):
    for name, blocks, table in ji.symbol_cases():
        fmt, host, w, h, tables = ji.symbol_image(kind, blocks, table)
        want = jm.entropy_of_file(jm.pillow_encode(fmt, host, w, h, 0, tables=tables))
        assert jm.entropy(fmt, host, w, h, 0, R=0, tables=tables) == want, name


@pytest.mark.parametrize("content", ji.CONTENTS)
def test_model_equals_pillow_on_extreme_content(content):
    for fmt, (w, h) in ((jm.RGB, (23, 17)), (jm.YUV444, (40, 24))):
        host = ji.content_host(fmt, content, w, h, seed=5)
        for q in (1, 100):
            want = jm.entropy_of_file(jm.pillow_encode(fmt, host, w, h, q))
            assert jm.entropy(fmt, host, w, h, q, R=0) == want, (fmt, q)


def test_model_equals_pillow_on_the_colour_lattice():
    """and with all-ones tables the DC coefficient of a flat block is 8 (Y - 128): rgb_ycc read off bit for bit"""
    w, h = ji.LATTICE_SIZE
    rgb = ji.lattice_rgb()
    host = ji.rgb_host(jm.RGB, rgb)
    want = jm.entropy_of_file(jm.pillow_encode(jm.RGB, host, w, h, 0, tables=ji.TABLES["ones"]))
    assert jm.entropy(jm.RGB, host, w, h, 0, R=0, tables=ji.TABLES["ones"]) == want
    cols = ji.lattice_colours()
    assert len(cols) == 4096 + 24 and len(np.unique(cols, axis=0)) == len(cols)
    assert {0, 255} <= set(cols[:, 0].tolist()) and np.array_equal(rgb[::8, ::8].reshape(-1, 3)[:len(cols)], cols)
    coefs, comp, _ = jm.scan_blocks(jm.RGB, jm.planes_of(jm.RGB, host, w, h), w, h, 0, tables=ji.TABLES["ones"])
    assert not coefs[:, 1:].any()
    ycc = np.stack(jm.rgb_to_ycc(cols[None]), -1)[0].astype(np.int64)          # (4120, 3)
    dc = coefs[:, 0].reshape(-1, 3)[:len(cols)]                                # one MCU of Y, Cb, Cr per colour
    assert np.array_equal(dc, 8 * (ycc - 128))
    for fmt in (jm.BGR, jm.RGB_PLANAR):
        assert all(np.array_equal(a, b) for a, b in zip(jm.planes_of(fmt, ji.rgb_host(fmt, rgb), w, h),
                                                        jm.planes_of(jm.RGB, host, w, h)))


# ---- coverage ----------------------------------------------------------------------------------------------------------
def test_symbol_images_emit_every_symbol_of_every_table():
    """a condition on the construction of the symbol images: 348 of 348, through luma alone and chroma alone"""
    seen = {kind: set() for kind in ji.SYMBOL_KINDS}
    for kind in ji.SYMBOL_KINDS:
        for _, blocks, table in ji.symbol_cases():
            fmt, host, w, h, tables = ji.symbol_image(kind, blocks, table)
            seen[kind] |= ji.symbols_of_image(fmt, host, w, h, tables)
    want = ji.every_symbol()
    assert len(want) == 348
    luma = {s for s in want if s[0] == 0}
    chroma = want - luma
    assert len(luma) == len(chroma) == 174
    assert luma <= seen["luma"], sorted(luma - seen["luma"])
    assert chroma <= seen["chroma"], sorted(chroma - seen["chroma"])
    assert chroma <= seen["chroma420"], sorted(chroma - seen["chroma420"])
    assert (seen["luma"] | seen["chroma"]) == want


def test_symbol_counter_counts_what_the_coder_codes():
    """the counter and jm.huffman are written apart: a scan whose symbols are known by construction"""
    z = np.zeros((4, 64), np.int32)
    z[0, 0], z[0, 1], z[0, 63] = 5, -1, 1023         # DC 3; (0, 1); three ZRL then (13, 10); no EOB
    z[1, 0] = 5                                      # DC difference 0; EOB
    z[2, 0], z[2, 17] = -2040 + 5, 2                 # chroma-free scan: comp 0 only; DC 11; ZRL, (0, 2), EOB
    z[3, 0] = z[2, 0]                                # after a restart (R = 3): the difference is the value itself
    got = ji.symbols_of_scan(z, np.zeros(4, np.int64), 1, 3)
    assert got == {(0, "DC", 3), (0, "AC", 0x01), (0, "AC", 0xF0), (0, "AC", 0xDA), (0, "DC", 0), (0, "AC", 0x00),
                   (0, "DC", 11), (0, "AC", 0x02)}
    assert (0, "DC", 0) not in ji.symbols_of_scan(z[2:], np.zeros(2, np.int64), 1, 1)
    assert ji.symbols_of_scan(z[2:], np.ones(2, np.int64), 1, 0) == {(1, "DC", 11), (1, "DC", 0), (1, "AC", 0xF0),
                                                                      (1, "AC", 0x02), (1, "AC", 0x00)}


# ---- boundary seeds ------------------------------------------------------------------------------------------------------
def test_segment_splitter():
    body = bytes([1, 0xFF, 0x00, 2, 0xFF, 0xD0, 0xFF, 0x00, 0xFF, 0xD1, 7])
    assert ji.split_segments(body) == [(bytes([1, 0xFF, 0, 2]), 0xD0), (bytes([0xFF, 0]), 0xD1), (bytes([7]), None)]
    assert ji.unstuff(bytes([1, 0xFF, 0, 2])) == bytes([1, 0xFF, 2])


@pytest.mark.parametrize("name", list(ji.SEARCH_SPACE))
def test_boundary_seed_has_its_property(name):
    assert set(ji.BOUNDARY_SEEDS) == set(ji.SEARCH_SPACE) == set(ji.PROPERTIES)
    fmt, host, w, h, q, R = ji.boundary_case(name)
    body = jm.entropy(fmt, host, w, h, q, R=R)
    segs = [(ji.unstuff(s), s, m) for s, m in ji.split_segments(body)]
    assert len(segs) == -(-(-(-w // (8 * jm.sampling(fmt)[0])) * -(-h // (8 * jm.sampling(fmt)[1]))) // R)
    hits = [(raw, s, m) for raw, s, m in segs if ji.PROPERTIES[name](raw, m is None)]
    assert hits, name
    raw, stuffed, marker = hits[0]
    ff = [i for i, b in enumerate(raw) if b == 0xFF]
    if name == "ff_at_lane_word_end":
        assert any(i % 4 == 3 for i in ff)
    elif name == "ff_at_255":
        assert 255 in ff and len(raw) > 256                  # the last byte of the first 256-byte step, not of the segment
    elif name == "ff_at_256":
        assert 256 in ff
    elif name == "ff_before_rst":
        assert marker is not None and stuffed[-2:] == b"\xff\x00"
        assert stuffed + bytes([0xFF, marker]) in body       # FF 00 FF Dn
    elif name == "ff_ff":
        assert any(b - a == 1 for a, b in zip(ff, ff[1:])) and b"\xff\x00\xff\x00" in stuffed
    elif name == "len_multiple_of_256":
        assert len(raw) in (256, 512, 768, 1024)
    elif name == "len_not_multiple_of_4":
        assert len(raw) % 4 in (1, 2, 3)
    elif name == "shorter_than_4":
        assert len(raw) in (1, 2, 3) and fmt == jm.YUV444 and R == 1
    else:
        assert name == "no_ff" and not ff and stuffed == raw


# ---- the C ABI, host-only entry points, through the shim's setters -------------------------------------------------------
def test_setters_change_only_their_field(shim):
    p = shim.jpeg_params_init(75, jm.YUV420)
    before = p.qtable
    p.restart_interval = 3
    assert p.restart_interval == 3 and p.qtable == before and (p.h_samp, p.v_samp, p.format) == (2, 2, jm.YUV420)
    p.qtable = as_lists(ji.TABLES["pair"])
    assert p.qtable == as_lists(ji.TABLES["pair"]) and p.restart_interval == 3 and p.quality == 75
    with pytest.raises(TypeError):
        p.qtable = [[1] * 64]
    with pytest.raises(TypeError):
        p.qtable = [[1] * 64, [256] * 64]


@pytest.mark.parametrize("fmt", jm.FORMATS)
@pytest.mark.parametrize("name", list(ji.TABLES) + ["ac63"])
def test_header_with_custom_tables_and_interval(shim, fmt, name):
    tables = ji.TABLES[name] if name in ji.TABLES else (ji.pass_table(63), ji.pass_table(63, 8))
    w, h = 40, 24
    host = ji.content_host(fmt, "noise", w, h, seed=2)
    for R in (1, 2, jm.restart_interval(fmt) - 1, jm.restart_interval(fmt)):
        p = shim.jpeg_params_init(50, fmt)
        p.restart_interval = R
        p.qtable = as_lists(tables)
        hdr = shim.jpeg_header(w, h, p)
        assert hdr == jm.header(w, h, fmt, 50, R=R, tables=tables), R
        img = PIL.open(io.BytesIO(hdr + jm.entropy(fmt, host, w, h, 50, R=R, tables=tables) + b"\xff\xd9"))
        img.load()
        assert img.size == (w, h) and [list(img.quantization[0]), list(img.quantization[1])] == as_lists(tables)


@pytest.mark.parametrize("fmt", jm.FORMATS)
def test_bad_tables_and_intervals_are_refused(shim, fmt):
    w, h = 32, 16
    rmax = 64 // (jm.sampling(fmt)[0] * jm.sampling(fmt)[1] + 2)
    good = shim.jpeg_params_init(90, fmt)
    good.restart_interval = rmax
    good.qtable = as_lists(ji.TABLES["all255"])
    assert shim.jpeg_stream_capacity(w, h, good) > 0
    for t in (0, 1):
        for k in (0, 5, 63):
            p = shim.jpeg_params_init(90, fmt)
            tables = as_lists(ji.TABLES["random"])
            tables[t][k] = 0
            p.qtable = tables                                  # the setter validates nothing
            assert p.qtable[t][k] == 0
            for call in (lambda: shim.jpeg_stream_capacity(w, h, p), lambda: shim.jpeg_header(w, h, p),
                         lambda: shim.jpeg_workspace_size(1, w, h, p)):
                with pytest.raises(ValueError, match="holds 0"):
                    call()
    for R in (0, -1, rmax + 1, 65):
        p = shim.jpeg_params_init(90, fmt)
        p.restart_interval = R
        with pytest.raises(ValueError, match="restart interval"):
            shim.jpeg_stream_capacity(w, h, p)
        with pytest.raises(ValueError, match="restart interval"):
            shim.jpeg_workspace_size(1, w, h, p)


def test_capacity_follows_the_interval(shim):
    """nseg x (2 x 208 bytes per block of a segment + the RST marker)"""
    for fmt, bpm in ((jm.YUV444, 3), (jm.YUV422, 4), (jm.YUV420, 6)):
        w, h = 128, 64
        H, V = jm.sampling(fmt)
        nmcu = (w // (8 * H)) * (h // (8 * V))
        for R in (1, 2, 64 // bpm):
            p = shim.jpeg_params_init(90, fmt)
            p.restart_interval = R
            assert shim.jpeg_stream_capacity(w, h, p) == -(-nmcu // R) * (2 * R * bpm * 208 + 2)
