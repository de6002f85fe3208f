"""vali_jpeg_encode_batch away from its defaults: every Huffman symbol of all four tables, restart intervals from 1 to
the largest, custom quantisation tables, the largest coefficients, the colour conversion on a lattice of colours, and
0xFF bytes and segment lengths on the edges of the stuffing and assembly loops.  Every result is compared byte for byte
with the numpy model of tests/jpeg_model.py, which tests/test_jpeg_params_host.py pins to Pillow's libjpeg on the same
inputs (tests/jpeg_encoder_inputs.py builds them).  Every call runs between 0xA5 sentinels that must survive."""
import functools
import io

import numpy as np
import pytest

import jpeg_encoder_inputs as ji
import jpeg_model as jm

PIL = pytest.importorskip("PIL.Image")

pytestmark = pytest.mark.gpu

NAMES = {jm.RGB: "RGB", jm.BGR: "BGR", jm.RGB_PLANAR: "RGB_PLANAR", jm.YUV444: "YUV444", jm.YUV422: "YUV422",
         jm.YUV420: "YUV420"}
TAIL = 4096


def upload(vali, gpu, fmt, host, w, h):
    s = vali.Surface.Make(vali.PixelFormat(fmt), w, h, gpu)
    assert s.HostSize == host.size
    ok, info = vali.PyFrameUploader(gpu).Run(np.ascontiguousarray(host), s)
    assert ok, info
    return s


def params(fmt, quality=75, R=None, tables=None):
    from vali_amd._native import shim

    p = shim.jpeg_params_init(quality, fmt)
    if R is not None:
        p.restart_interval = R
    if tables is not None:
        p.qtable = [[int(v) for v in t] for t in tables]
    return p


def encode_descs(vali, gpu, fmt, descs, w, h, p, n=None):
    """vali_jpeg_encode_batch through the shim's C-ABI wrappers: the entropy data of every image.  The output buffer and
    the size array are filled with 0xA5 first; everything past an image's bytes must still hold it afterwards."""
    from vali_amd._native import shim

    n = len(descs) if n is None else n
    cap = shim.jpeg_stream_capacity(w, h, p)
    wsb = shim.jpeg_workspace_size(n, w, h, p)
    stream = vali.HipResMgr.Instance().GetStream(gpu)
    total = max(n, 1) * cap + TAIL
    nsz = 4 * (n + 4)
    ws, out, sizes = shim.mem_alloc(gpu, wsb), shim.mem_alloc(gpu, total), shim.mem_alloc(gpu, nsz)
    d_src = shim.descs_upload(gpu, descs, stream)
    got, lens = np.zeros(total, np.uint8), np.zeros(n + 4, np.uint32)
    try:
        shim.memset2d_async(gpu, out, total, 0xA5, total, 1, stream)
        shim.memset2d_async(gpu, sizes, nsz, 0xA5, nsz, 1, stream)
        assert shim.jpeg_encode_batch(d_src, n, w, h, fmt, p, ws, wsb, out, cap, sizes, stream) == 0
        shim.memcpy2d_async(gpu, got.ctypes.data, total, out, total, total, 1, 1, stream)
        shim.memcpy2d_async(gpu, lens.ctypes.data, nsz, sizes, nsz, nsz, 1, 1, stream)
        shim.stream_sync(gpu, stream)
    finally:
        for ptr in (d_src, ws, out, sizes):
            shim.mem_free(gpu, ptr)
    assert np.all(lens[n:] == 0xA5A5A5A5)
    bodies = []
    for i in range(n):
        size = int(lens[i])
        assert size <= cap, (i, size, cap)
        bodies.append(bytes(got[i * cap: i * cap + size]))
        assert np.all(got[i * cap + size: (i + 1) * cap] == 0xA5), i      # nothing past the image's bytes
    assert np.all(got[n * cap:] == 0xA5)
    return bodies


def gpu_file(vali, gpu, fmt, host, w, h, p):
    from vali_amd._native import shim

    s = upload(vali, gpu, fmt, host, w, h)
    body = encode_descs(vali, gpu, fmt, [s.desc()], w, h, p)[0]
    return shim.jpeg_header(w, h, p) + body + b"\xff\xd9"


def where(a, b):
    """the first differing byte, for the assertion message"""
    n = min(len(a), len(b))
    d = np.flatnonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))
    return (len(a), len(b), int(d[0]) if d.size else n)


def check(vali, gpu, fmt, host, w, h, quality=75, R=None, tables=None):
    got = gpu_file(vali, gpu, fmt, host, w, h, params(fmt, quality, R, tables))
    want = jm.encode(fmt, host, w, h, quality, R=R, tables=tables)
    assert got == want, (NAMES[fmt], w, h, quality, R) + where(got, want)
    return got


# ---- every symbol --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ji.SYMBOL_KINDS)
def test_every_symbol(vali, gpu, kind):
    """luma: the blocks in Y; chroma: in U and V; chroma420: the same with six blocks per MCU, where the blocks of
    index >= 4 read the chroma tables.  test_jpeg_params_host: the three runs emit 174 of 174 symbols each."""
    for name, blocks, table in ji.symbol_cases():
        fmt, host, w, h, tables = ji.symbol_image(kind, blocks, table)
        check(vali, gpu, fmt, host, w, h, tables=tables)


# ---- restart intervals -----------------------------------------------------------------------------------------------------
def mcu_grid(n):
    """n MCUs as the squarest mcux x mcuy"""
    my = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
    return n // my, my


def image_of_mcus(fmt, n):
    """a size of exactly n MCUs whose last column and row of MCUs are partial"""
    H, V = jm.sampling(fmt)
    mx, my = mcu_grid(n)
    return mx * 8 * H - 2 * H - (fmt == jm.YUV444), my * 8 * V - 2 * V - (fmt == jm.YUV444)


def interval_cases():
    out = []
    for fmt in (jm.YUV444, jm.YUV422, jm.YUV420):
        rmax = jm.restart_interval(fmt)
        for R in (1, 2, rmax - 1, rmax):
            # one segment; a short last segment; a last segment of exactly R MCUs; 8 and 9 segments (RST7 -> RST0)
            mcus = sorted({R, R + 1, 2 * R, 8 * R, 8 * R + 1, 9 * R})
            out.append(pytest.param(fmt, R, mcus, id=f"{NAMES[fmt]}-R{R}"))
    return out


@pytest.mark.parametrize("fmt, R, mcus", interval_cases())
def test_restart_intervals(vali, gpu, fmt, R, mcus):
    for n in mcus:
        w, h = image_of_mcus(fmt, n)
        host = ji.content_host(fmt, "noise", w, h, seed=n)
        got = check(vali, gpu, fmt, host, w, h, quality=60, R=R)
        assert len(ji.split_segments(jm.entropy_of_file(got))) == -(-n // R)


@pytest.mark.parametrize("nseg", [256, 257, 272])
@pytest.mark.parametrize("fmt", [jm.YUV444, jm.YUV422, jm.YUV420], ids=NAMES.get)
def test_segment_counts_around_the_offsets_chunk(vali, gpu, fmt, nseg):
    """k_jpeg_offsets scans 256 segments at a time: exactly one chunk, one more segment, and a second partial chunk"""
    w, h = image_of_mcus(fmt, nseg)
    host = ji.content_host(fmt, "noise", w, h, seed=nseg)
    got = check(vali, gpu, fmt, host, w, h, quality=40, R=1)
    assert len(ji.split_segments(jm.entropy_of_file(got))) == nseg


# ---- tables ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [jm.RGB, jm.YUV420], ids=NAMES.get)
@pytest.mark.parametrize("name", list(ji.TABLES))
def test_custom_tables(vali, gpu, name, fmt):
    w, h = 46, 26
    for content in ("noise", "binary"):
        check(vali, gpu, fmt, ji.content_host(fmt, content, w, h, seed=3), w, h, tables=ji.TABLES[name])


# ---- extreme content ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [jm.RGB, jm.YUV444], ids=NAMES.get)
@pytest.mark.parametrize("content", ji.CONTENTS)
def test_extreme_content(vali, gpu, content, fmt):
    for w, h in ((23, 17), (40, 24), (65, 9)):
        host = ji.content_host(fmt, content, w, h, seed=5)
        for q in (100, 1):
            check(vali, gpu, fmt, host, w, h, quality=q)


# ---- colour lattice ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice_file():
    w, h = ji.LATTICE_SIZE
    return jm.encode(jm.RGB, ji.rgb_host(jm.RGB, ji.lattice_rgb()), w, h, 0, tables=ji.TABLES["ones"])


@pytest.mark.parametrize("fmt", [jm.RGB, jm.BGR, jm.RGB_PLANAR], ids=NAMES.get)
def test_colour_lattice(vali, gpu, fmt):
    """4120 flat blocks under all-ones tables: the DC of each is 8 (Y - 128), so every colour's rgb_ycc result is in
    the bytes.  The three layouts hold the same picture, and the header does not name the layout: one file for all."""
    w, h = ji.LATTICE_SIZE
    got = gpu_file(vali, gpu, fmt, ji.rgb_host(fmt, ji.lattice_rgb()), w, h, params(fmt, tables=ji.TABLES["ones"]))
    want = lattice_file()
    assert got == want, where(got, want)


# ---- boundary seeds ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ji.SEARCH_SPACE))
def test_boundary_seed(vali, gpu, name):
    fmt, host, w, h, q, R = ji.boundary_case(name)
    check(vali, gpu, fmt, host, w, h, quality=q, R=R)


# ---- batch and slots -------------------------------------------------------------------------------------------------------
def test_batch_with_custom_interval_and_tables(vali, gpu):
    fmt, w, h, R, tables = jm.YUV420, 48, 32, 2, ji.TABLES["pair"]
    hosts = [ji.content_host(fmt, c, w, h, seed=i) for i, c in enumerate(("noise", "binary", "block_checker"))]
    surfs = [upload(vali, gpu, fmt, hst, w, h) for hst in hosts]
    p = params(fmt, R=R, tables=tables)
    batch = encode_descs(vali, gpu, fmt, [s.desc() for s in surfs], w, h, p)
    for i, s in enumerate(surfs):
        assert batch[i] == jm.entropy(fmt, hosts[i], w, h, 0, R=R, tables=tables), i
        assert batch[i] == encode_descs(vali, gpu, fmt, [s.desc()], w, h, p)[0], i


def test_empty_batch_writes_nothing(vali, gpu):
    s = vali.Surface.Make(vali.RGB, 32, 16, gpu)
    assert encode_descs(vali, gpu, jm.RGB, [s.desc()], 32, 16, params(jm.RGB, R=2), n=0) == []


# ---- geometry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w, h", [(8191, 1), (1, 8191)])
def test_one_pixel_wide_or_high(vali, gpu, w, h):
    check(vali, gpu, jm.RGB, ji.content_host(jm.RGB, "noise", w, h, seed=9), w, h, quality=90)


def test_widest_subsampled_row(vali, gpu):
    """65534 x 2, 4:2:0: 4096 MCUs in one row, the second block row of every MCU a dummy row"""
    w, h = 65534, 2
    check(vali, gpu, jm.YUV420, ji.content_host(jm.YUV420, "flat", w, h, seed=4), w, h, quality=90)


def test_planes_at_odd_addresses_with_odd_pitch(vali, gpu):
    """three DLPack views as the planes of a YUV444 surface: no row of any plane but by chance starts on a multiple
    of 4, so load_row_u8 reads them byte by byte"""
    import torch

    from vali_amd._native import shim

    fmt, w, h, pitch = jm.YUV444, 50, 21, 61
    host = ji.content_host(fmt, "noise", w, h, seed=6)
    big = torch.zeros(3 * (h * pitch + 2) + 8, dtype=torch.uint8, device=f"cuda:{gpu}")
    planes, views = [], []
    for c in range(3):
        start = 1 + c * (h * pitch + 2)                              # 1, 1284, 2567 -> made odd below
        start += 1 - (start & 1)
        view = big[start:start + h * pitch].view(h, pitch)[:, :w]
        view.copy_(torch.from_numpy(host[c * w * h:(c + 1) * w * h].reshape(h, w)).to(big.device))
        views.append(view)
        planes.append(vali.Surface.from_dlpack(torch.utils.dlpack.to_dlpack(view), vali.Y))
    torch.cuda.synchronize()
    for pl in planes:
        assert pl.PixelPtr(0) & 1 and pl.Pitch == pitch and (pl.Width, pl.Height) == (w, h)
    desc = shim.SurfaceDesc([pl.PixelPtr(0) for pl in planes], [pitch] * 3, w, h, fmt)
    p = params(fmt, 85)
    got = encode_descs(vali, gpu, fmt, [desc], w, h, p)[0]
    want = jm.entropy(fmt, host, w, h, 85)
    assert got == want, where(got, want)


# ---- independent of the model ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [jm.RGB, jm.YUV420], ids=NAMES.get)
@pytest.mark.parametrize("name", ["random", "pair", "swapped"])
def test_decoders_read_the_same_picture(vali, gpu, name, fmt):
    """Pillow decodes the GPU's file to the pixels it decodes from its own file written with the same tables, and so
    does PyNvJpegDecoder (libjpeg-turbo's default decompression bit for bit)"""
    w, h = 46, 26
    tables = ji.TABLES[name]
    host = ji.content_host(fmt, "noise", w, h, seed=8)
    theirs = np.asarray(PIL.open(io.BytesIO(jm.pillow_encode(fmt, host, w, h, 0, tables=tables))).convert("RGB"))
    dec = vali.PyNvJpegDecoder(gpu)
    for R in (1, jm.restart_interval(fmt)):
        ours = gpu_file(vali, gpu, fmt, host, w, h, params(fmt, R=R, tables=tables))
        assert np.array_equal(np.asarray(PIL.open(io.BytesIO(ours)).convert("RGB")), theirs), R
        surfs, info = dec.Run([ours], vali.RGB)
        assert info == vali.TaskExecInfo.SUCCESS, R
        back = np.zeros(surfs[0].HostSize, np.uint8)
        assert vali.PySurfaceDownloader(gpu).Run(surfs[0], back)[0]
        assert np.array_equal(back.reshape(h, w, 3), theirs), R
