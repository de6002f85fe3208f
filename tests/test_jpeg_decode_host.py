"""CPU side of the JPEG decoder: the numpy model (tests/jpeg_decode_model.py) against Pillow's libjpeg-turbo byte for
byte, and vali_jpeg_parse / vali_jpeg_decode_workspace_size through the C ABI (no GPU needed)."""
import io
from pathlib import Path

import numpy as np
import pytest

import jpeg_decode_files as jf
import jpeg_decode_model as dm
import jpeg_model as jm

PIL = pytest.importorskip("PIL.Image")
GOLDEN = Path(__file__).resolve().parent / "golden"
SIZES = [(1, 1), (7, 9), (17, 33), (62, 30)]


@pytest.fixture(scope="module")
def frame():
    return np.asarray(PIL.open(GOLDEN / "frame_0.jpg").convert("RGB"))


def pillow_rgb(data):
    return np.asarray(PIL.open(io.BytesIO(data)).convert("RGB"))


def pillow_y(data):
    im = PIL.open(io.BytesIO(data))
    im.draft("L", im.size)
    return np.asarray(im.convert("L"))


@pytest.mark.parametrize("sampling", jf.SAMPLINGS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_model_equals_pillow(frame, sampling, size):
    w, h = size
    for q in (1, 50, 75, 90, 100):
        for restart in (False, True):
            data = jf.make_file(sampling, w, h, q, "noise" if q == 100 else "frame", seed=q, frame=frame,
                                restart=restart)
            assert (dm.parse(data)["ri"] > 0) == restart
            assert np.array_equal(dm.decode(data, "RGB"), pillow_rgb(data)), (sampling, w, h, q, restart)
            assert np.array_equal(dm.decode(data, "Y"), pillow_y(data)), (sampling, w, h, q, restart)


def test_model_equals_pillow_with_restarts_from_jpeg_model(frame):
    """jpeg_model.encode with R writes restart markers of its own (the GPU encoder's files)"""
    for fmt in (jm.RGB, jm.YUV422, jm.YUV420):
        host = jm.make_host(fmt, 64, 48, "frame", frame=frame)
        for R in (1, 3, jm.restart_interval(fmt)):
            data = jm.encode(fmt, host, 64, 48, 90, R)
            assert np.array_equal(dm.decode(data), pillow_rgb(data)), (fmt, R)


def test_model_equals_pillow_at_1080p(frame):
    rgb = jf.picture(1920, 1080, "frame", 2, frame)
    data = jf.pillow_file(rgb, "420", 90)
    assert np.array_equal(dm.decode(data), pillow_rgb(data))


def test_model_equals_pillow_on_frame0():
    data = (GOLDEN / "frame_0.jpg").read_bytes()
    assert np.array_equal(dm.decode(data), pillow_rgb(data))
    assert np.array_equal(dm.decode(data, "Y"), pillow_y(data))


def test_model_planes_are_the_idct_of_the_components(frame):
    """raw outputs: the component planes cropped to the image, chroma at its own resolution"""
    data = jf.make_file("420", 34, 18, 90, frame=frame)
    y, cb, cr = dm.decode(data, "planes")
    assert y.shape == (18, 34) and cb.shape == (9, 17) and cr.shape == (9, 17)
    assert np.array_equal(y, dm.decode(data, "Y"))
    nv12 = dm.surface_bytes(data, "NV12")
    assert nv12.size == 34 * 18 * 3 // 2 and np.array_equal(nv12[34 * 18::2], cb.reshape(-1))


# ---- C ABI --------------------------------------------------------------------------------------------------------------
def shim():
    from vali_amd._native import shim as s

    return s


def test_parse_frame0():
    info = shim().jpeg_parse((GOLDEN / "frame_0.jpg").read_bytes())
    assert (info.width, info.height, info.components, info.h_samp, info.v_samp) == (848, 464, 3, 1, 1)
    assert info.restart_interval == 0 and info.segments == 1
    assert (info.mcux, info.mcuy) == (106, 58)
    data = (GOLDEN / "frame_0.jpg").read_bytes()
    assert data[info.data_offset - 14:info.data_offset - 12] == b"\xff\xda"
    assert data[info.data_offset + info.data_len:] == b"\xff\xd9"
    assert shim().JPEG_INFO_SIZE == 8984


@pytest.mark.parametrize("name", ["frame_0_90_deg.jpg", "frame_0_180_deg.jpg", "frame_0_270_deg.jpg"])
def test_parse_refuses_progressive(name):
    s = shim()
    rc, _ = s.jpeg_parse_rc((GOLDEN / name).read_bytes())
    assert rc == s.ERR_UNSUPPORTED and "progressive" in s.last_error()


def test_parse_fields_and_16_bit_tables(frame):
    s = shim()
    data = jf.make_file("420", 100, 60, 90, frame=frame, restart=True)
    info = s.jpeg_parse(data)
    assert (info.h_samp, info.v_samp, info.restart_interval) == (2, 2, dm.parse(data)["ri"])
    assert info.segments == -(-(info.mcux * info.mcuy) // info.restart_interval)
    assert info.qtable[0] == dm.parse(data)["q"][0].tolist()
    # the same file with its luma DQT rewritten as a 16-bit table
    i = data.index(b"\xff\xdb")
    ln = int.from_bytes(data[i + 2:i + 4], "big")
    body = data[i + 4:i + 2 + ln]
    assert body[0] == 0 and len(body) >= 65
    t16 = bytes([0x10]) + b"".join(int(v).to_bytes(2, "big") for v in body[1:65]) + body[65:]
    d16 = data[:i] + b"\xff\xdb" + (len(t16) + 2).to_bytes(2, "big") + t16 + data[i + 2 + ln:]
    assert s.jpeg_parse(d16).qtable == info.qtable
    assert np.array_equal(dm.decode(d16), dm.decode(data))


def test_parse_refuses_unsupported_headers(frame):
    s = shim()
    data = jf.make_file("444", 32, 16, 90, frame=frame)
    sof = data.index(b"\xff\xc0")

    def rc(d):
        return s.jpeg_parse_rc(d)[0]

    assert rc(data[:sof] + b"\xff\xc1" + data[sof + 2:]) == 0                          # SOF1, 8-bit: fine
    assert rc(data[:sof] + b"\xff\xc9" + data[sof + 2:]) == s.ERR_UNSUPPORTED          # arithmetic
    assert rc(data[:sof] + b"\xff\xc3" + data[sof + 2:]) == s.ERR_UNSUPPORTED          # lossless
    assert rc(data[:sof + 4] + b"\x0c" + data[sof + 5:]) == s.ERR_UNSUPPORTED          # 12-bit
    assert rc(data[:sof + 5] + b"\x00\x00" + data[sof + 7:]) == s.ERR_UNSUPPORTED      # height 0: DNL
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"
    assert rc(data[:2] + adobe + data[2:]) == s.ERR_UNSUPPORTED                         # transform 0
    assert rc(data[:2] + adobe[:-1] + b"\x01" + data[2:]) == 0                          # transform 1: YCbCr
    rgbids = data[:sof + 10] + b"R" + data[sof + 11:sof + 13] + b"G" + data[sof + 14:sof + 16] + b"B" + data[sof + 17:]
    assert rc(rgbids) != 0
    assert rc(data[:-2] + b"\xff\xda" + data[-2:]) == s.ERR_UNSUPPORTED                 # a second scan


def test_parse_refuses_truncated_headers_and_bad_tables(frame):
    s = shim()
    data = jf.make_file("420", 32, 16, 90, frame=frame)
    sos = data.index(b"\xff\xda")
    for cut in (0, 1, 3, 10, 100, sos, sos + 5):
        assert s.jpeg_parse_rc(data[:cut])[0] == s.ERR_INVALID_ARG, cut
    dht = data.index(b"\xff\xc4")
    # oversubscribed: three codes of length 1
    bad = bytearray(data)
    bad[dht + 5] = 3
    assert s.jpeg_parse_rc(bytes(bad))[0] != 0
    # the all-ones code: the DC luma table of Annex K with one more code of length 9 (BITS[9] = 2)
    bad = bytearray(data)
    assert list(bad[dht + 5:dht + 21]) == jm.DC_LUMA[0]
    bad[dht + 5 + 8] += 1
    bad[dht + 21 + 12:dht + 21 + 12] = b"\x0b"
    ln = int.from_bytes(bad[dht + 2:dht + 4], "big") + 1
    bad[dht + 2:dht + 4] = ln.to_bytes(2, "big")
    rc, _ = s.jpeg_parse_rc(bytes(bad))
    assert rc == s.ERR_INVALID_ARG and "all-ones" in s.last_error()


def test_parse_survives_seeded_header_mutations(frame):
    """mutated headers give an error or an info that passes the decoder's own consistency rules, never a crash"""
    s = shim()
    base = jf.make_file("420", 40, 24, 90, frame=frame, restart=True)
    hdr_end = base.index(b"\xff\xda") + 14
    rng = np.random.default_rng(11)
    ok = 0
    for _ in range(3000):
        b = bytearray(base)
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(2, hdr_end))] = int(rng.integers(0, 256))
        if rng.random() < 0.2:
            b = b[:int(rng.integers(2, len(b)))]
        rc, info = s.jpeg_parse_rc(bytes(b))
        assert rc in (0, s.ERR_INVALID_ARG, s.ERR_UNSUPPORTED)
        if rc == 0:
            ok += 1
            assert 1 <= info.width <= 65535 and 1 <= info.height <= 65535 and info.components in (1, 3)
            assert info.data_offset + info.data_len <= len(b)
            assert s.jpeg_decode_workspace_size([info]) > 0
    assert ok > 0


def test_workspace_size_covers_worst_cases(frame):
    s = shim()
    small = s.jpeg_parse(jf.make_file("420", 64, 48, 90, frame=frame))
    noise = s.jpeg_parse(jf.pillow_file(jf.picture(640, 480, "noise", 1), "444", 100))
    tiny_rst = s.jpeg_parse(jf.model_file(jf.picture(64, 48, "noise", 1), 1, 1, 100, R=1))
    one = s.jpeg_decode_workspace_size([small])
    assert s.jpeg_decode_workspace_size([small, small]) > one
    ws = s.jpeg_decode_workspace_size([noise])
    blocks = noise.mcux * noise.mcuy * 3
    # the coefficient blocks, the planes, the unstuffed data and one subsequence record per 1024 bits
    assert ws >= blocks * 192 + noise.data_len + 20 * (noise.data_len * 8 // 1024)
    assert s.jpeg_decode_workspace_size([tiny_rst]) >= 20 * tiny_rst.segments
    assert s.jpeg_decode_workspace_size([]) > 0
    with pytest.raises(ValueError):
        bad = small.copy()
        bad.data_len = 1 << 30
        s.jpeg_decode_workspace_size([bad])


def test_header_cache_gives_what_the_parser_gives(vali, frame):
    """PyNvJpegDecoder caches infos by header bytes: MJPEG-style frames with one header, entropy lengths that differ"""
    dec = vali.PyNvJpegDecoder.__new__(vali.PyNvJpegDecoder)
    dec._headers = {}
    files = [jm.encode(jm.YUV420, jm.make_host(jm.YUV420, 64, 48, "frame", seed=i, frame=np.roll(frame, 9 * i, 0)),
                       64, 48, 75) for i in range(4)]
    s = shim()
    for f in files:
        got = dec._parse(np.frombuffer(f, np.uint8))
        want = s.jpeg_parse(f)
        assert got.tobytes() == want.tobytes()
    assert len(dec._headers) == 1
    info = dec.Info(files[0])
    assert (info.width, info.height, info.components, info.sampling, info.restart_interval) == (64, 48, 3, "420", 10)
