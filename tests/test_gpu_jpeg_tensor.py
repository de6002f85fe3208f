"""PyNvJpegEncoder.RunTensor on the GPU: float32 / float16 / bfloat16 / uint8 tensors of shape (N, 3, H, W) straight to JPEG.

1. every file equals, byte for byte, the file `Run` writes for an 8-bit surface of the model's pixels
   (tests/jpeg_tensor_model.py, pinned to the torch chain by tests/test_jpeg_tensor_host.py);
2. the quantiser alone, made observable: YUV444 at quality 100 with tensors constant over each 8x8 block -- the block's
   quantised DC is then 8 (p - 128) (the DCT's DC term of a constant block, all quantisers 1), so a file is right only
   if every block's pixel value is;
3. the hip backend's files decode (Pillow) to the pixels the cpu backend's files decode to;
4. the contract around it."""
import io
import types

import numpy as np
import pytest

import jpeg_decode_model as dm
import jpeg_model as jm
import jpeg_tensor_model as tm

PIL = pytest.importorskip("PIL.Image")
torch = pytest.importorskip("torch")

gpu_test = pytest.mark.gpu

LAYOUTS = ("contiguous", "channels_last", "slice", "step")
# (format, subsampling): the channels' names come from the format
CODINGS = (("RGB", "444"), ("RGB", "422"), ("RGB", "420"), ("BGR", "444"), ("BGR", "422"), ("BGR", "420"),
           ("YUV444", "444"))
# 1x1, 7x5, 8x8, 16x16: edge replication and partial MCUs at every sampling; 17x9: dummy blocks; 250x3: wide and flat;
# 120x104: 585 blocks / 104 MCUs / 56 MCUs at 4:4:4 / 4:2:2 / 4:2:0 -- more than one workgroup (256 blocks, 64 and 42 MCUs)
# and more than one restart segment at every sampling
SIZES = ((1, 1), (7, 5), (8, 8), (16, 16), (17, 9), (33, 31), (250, 3), (120, 104))
BIG = (120, 104)


def _sampling(coding):
    """which form of the kernel a coding takes: "444", "422", "420" or "yuv" """
    return "yuv" if coding[0] == "YUV444" else coding[1]


def _wants(case):
    """what a case covers: every pair of values of two axes (dtype, layout, coding, N, size), and the kernel
    instantiation with the path it takes, dtype x layout x sampling"""
    axes = case[:5]
    pairs = {(a, axes[a], b, axes[b]) for a in range(5) for b in range(a + 1, 5)}
    return pairs | {("kernel", case[0], case[1], _sampling(case[2]))}


def _cases():
    """A pairwise-covering subset of dtype x layout x coding x N x size: greedily, the case that covers most of what is
    still uncovered, until every pair of values of any two axes and every dtype x layout x sampling has a case; the
    (scale, offset) pairs are dealt round afterwards (uint8 mostly with its default)."""
    import itertools

    space = list(itertools.product(tm.DTYPES, LAYOUTS, CODINGS, (1, 3), SIZES))
    todo = set().union(*(_wants(c) for c in space))
    # the issue's own: every dtype with both layouts at 120x104 "420"
    cases = [(d, lay, ("RGB", "420"), 1 + 2 * li, BIG) for d in tm.DTYPES
             for li, lay in enumerate(("contiguous", "channels_last"))]
    for c in cases:
        todo -= _wants(c)
    while todo:
        best = max(space, key=lambda c: len(_wants(c) & todo))       # the first of equals: deterministic
        cases.append(best)
        todo -= _wants(best)
    out = []
    for k, c in enumerate(cases):
        pair = k % 4
        if c[0] == "uint8" and k % 3:
            pair = None
        out.append(c + (pair,))
    return out


CASES = _cases()


def _case_id(case):
    dtype, layout, (fmt, samp), n, (w, h), pair = case
    return f"{dtype}-{layout}-{fmt}{samp}-n{n}-{w}x{h}-s{pair}"


def test_cases_cover_every_pair_of_axis_values():
    import itertools

    axes = (tm.DTYPES, LAYOUTS, CODINGS, (1, 3), SIZES)
    for a, b in itertools.combinations(range(5), 2):
        have = {(c[a], c[b]) for c in CASES}
        missing = set(itertools.product(axes[a], axes[b])) - have
        assert not missing, (a, b, sorted(missing, key=str)[:5])
    # every instantiation of the tensor kernel, on the vector path and on the per-element path
    have = {(c[0], c[1], _sampling(c[2])) for c in CASES}
    assert have == set(itertools.product(tm.DTYPES, LAYOUTS, ("444", "422", "420", "yuv")))
    # sizes against samplings: edge replication, partial MCUs and dummy blocks at every sampling, whatever the order
    assert {(c[4], _sampling(c[2])) for c in CASES} == set(itertools.product(SIZES, ("444", "422", "420", "yuv")))
    for dtype in tm.DTYPES:
        for layout in ("contiguous", "channels_last"):
            assert any(c[:3] == (dtype, layout, ("RGB", "420")) and c[4] == BIG for c in CASES), (dtype, layout)
    assert {c[5] for c in CASES} == {None, 0, 1, 2, 3}
    for dtype in tm.DTYPES[:3]:
        assert {c[5] for c in CASES if c[0] == dtype} == {0, 1, 2, 3}, dtype
    assert len(CASES) <= 110


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def device_tensor(bits, dtype, layout, gpu):
    """a GPU tensor of logical shape (N, 3, H, W) holding `bits` ((N, H, W, 3) bit patterns) in the given layout"""
    dev = f"cuda:{gpu}"
    x = tm.torch_tensor(bits, dtype).permute(0, 3, 1, 2).contiguous().to(dev)           # (N, 3, H, W) contiguous
    n, _, h, w = x.shape
    if layout == "contiguous":
        t = x
    elif layout == "channels_last":
        t = x.contiguous(memory_format=torch.channels_last)
    elif layout == "slice":
        # an odd element offset: rows start off every vector boundary, so the per-element path is taken everywhere
        big = torch.full((n, 3, h + 2, w + 5), 77, dtype=x.dtype, device=dev)
        t = big[:, :, 1:1 + h, 3:3 + w]
        t.copy_(x)
    else:
        big = torch.full((2 * n, 3, h, w), 77, dtype=x.dtype, device=dev)
        t = big[::2]
        t.copy_(x)
    torch.cuda.synchronize()
    assert t.shape == x.shape
    return t


def host_of(fmt, p):
    """the host image (Surface.HostSize layout) of format `fmt` whose channels, in the format's own order, are p[..., c]"""
    if fmt in ("RGB", "BGR"):
        return np.ascontiguousarray(p).reshape(-1)
    return np.ascontiguousarray(p.transpose(2, 0, 1)).reshape(-1)


def upload(vali, gpu, fmt, host, w, h):
    s = vali.Surface.Make(getattr(vali, fmt), w, h, gpu)
    assert s.HostSize == host.size
    ok, info = vali.PyFrameUploader(gpu).Run(host, s)
    assert ok, info
    return s


@pytest.fixture(scope="module")
def enc(vali, gpu):
    return vali.PyNvJpegEncoder(gpu, backend="hip")


@pytest.fixture(scope="module")
def cpu_enc(vali, gpu):
    return vali.PyNvJpegEncoder(gpu, backend="cpu")


def run_tensor(vali, enc, ctx, t, scale=None, offset=0.0):
    out, info = enc.RunTensor(ctx, t, scale, offset)
    assert info == vali.TaskExecInfo.SUCCESS
    return [bytes(b.tobytes()) for b in out]


def run_surfaces(vali, enc, ctx, surfaces):
    out, info = enc.Run(ctx, surfaces)
    assert info == vali.TaskExecInfo.SUCCESS
    return [bytes(b.tobytes()) for b in out]


def pair_of(pair, dtype):
    """(scale, offset) as RunTensor takes them, and as the model does"""
    if pair is None:
        d = 1.0 if dtype == "uint8" else 255.0
        return (None, 0.0), ((d,) * 3, (0.0,) * 3)
    scale, offset = tm.SCALE_OFFSETS[pair]
    if pair < 3:                                # one number for all channels
        return (scale[0], offset[0]), (scale, offset)
    return (scale, offset), (scale, offset)


# ---- 1. byte identity with the surface path ---------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_file_equals_the_surface_path(vali, gpu, enc, case):
    dtype, layout, (fmt, samp), n, (w, h), pair = case
    given, (scale, offset) = pair_of(pair, dtype)
    bits = tm.noise_bits(dtype, (n, h, w, 3), scale, offset, seed=w * 1000 + h)
    p = tm.quantise(tm.as_float32(bits, dtype), scale, offset)                    # (N, H, W, 3)
    if dtype != "uint8" and p.size >= 300:
        outside = np.mean((p == 0) | (p == 255))
        assert 0.03 < outside < 0.25, outside                                     # about a tenth is clamped
    ctx = enc.Context(90, getattr(vali, fmt), subsampling=samp)
    got = run_tensor(vali, enc, ctx, device_tensor(bits, dtype, layout, gpu), *given)
    surfs = [upload(vali, gpu, fmt, host_of(fmt, p[i]), w, h) for i in range(n)]
    want = run_surfaces(vali, enc, ctx, surfs)
    assert len(got) == n
    for i in range(n):
        assert got[i] == want[i], (case, i, len(got[i]), len(want[i]))
    if n == 3:                                                                     # the items differ: none was read twice
        assert len(set(got)) == 3 or w * h < 4


@gpu_test
def test_rgb_planar_names_the_channels_as_rgb_does(vali, gpu, enc):
    w, h = 33, 31
    bits = tm.noise_bits("float16", (2, h, w, 3), (255.0,) * 3, (0.0,) * 3, seed=5)
    t = device_tensor(bits, "float16", "contiguous", gpu)
    for samp in ("444", "420"):
        a = run_tensor(vali, enc, enc.Context(90, vali.RGB, subsampling=samp), t)
        b = run_tensor(vali, enc, enc.Context(90, vali.RGB_PLANAR, subsampling=samp), t)
        assert a == b


# ---- 2. the quantiser, made observable ----------------------------------------------------------------------------------------
# a different (scale, offset) in every channel; the second channel of both and the third of the first hold inputs that a
# fused multiply-add would quantise differently (tests/test_jpeg_tensor_host.py)
TRIPLES = (((255.0, tm.SCALE_OFFSETS[3][0][1], 127.5), (0.0, tm.SCALE_OFFSETS[3][1][1], 127.5)), tm.SCALE_OFFSETS[3])
BLOCKS_WIDE = 32


def block_image(dtype):
    """(bit patterns (1, H, W, 3) constant over each 8x8 block, the blocks' patterns (bh, bw)): block k carries the k-th
    value of the dtype's edge set, the same in every channel (the channels differ in scale and offset)"""
    vals = tm.edge_bits(dtype)
    bh = -(-vals.size // BLOCKS_WIDE)
    grid = np.zeros(bh * BLOCKS_WIDE, vals.dtype)
    grid[:vals.size] = vals
    grid = grid.reshape(bh, BLOCKS_WIDE)
    img = np.repeat(np.repeat(grid, 8, 0), 8, 1)
    return np.repeat(img[None, :, :, None], 3, 3), grid


_trusted = {}


def expected_block_file(dtype, ti):
    """the model's file for block_image(dtype) under TRIPLES[ti] -- after making sure, on the host, that the file shows
    every block's pixel value: the DC terms decoded back from it are 8 (p - 128) in every block of every component, so
    no two images that differ in any block's p share a file; and, literally, a single block's p moved by +-1 gives
    another file"""
    if (dtype, ti) in _trusted:
        return _trusted[dtype, ti]
    scale, offset = TRIPLES[ti]
    bits, grid = block_image(dtype)
    h, w = bits.shape[1:3]
    pb = tm.quantise(tm.as_float32(np.repeat(grid[:, :, None], 3, 2), dtype), scale, offset)      # (bh, bw, 3)
    planes = [np.repeat(np.repeat(pb[..., c], 8, 0), 8, 1) for c in range(3)]
    coefs, comp, bpm = jm.scan_blocks(jm.YUV444, planes, w, h, 100)
    assert bpm == 3 and (coefs[:, 1:] == 0).all()
    assert np.array_equal(coefs[:, 0].reshape(-1, 3), 8 * (pb.reshape(-1, 3).astype(np.int64) - 128))
    R = jm.restart_interval(jm.YUV444)
    body = jm.huffman(coefs, comp, bpm, R)
    want = jm.header(w, h, jm.YUV444, 100) + body + b"\xff\xd9"
    back = dm.entropy_decode(dm.parse(want))
    for c in range(3):
        assert np.array_equal(back[c][..., 0], 8 * (pb[..., c].astype(np.int64) - 128)), c
    rng = np.random.default_rng(7)
    for b in {0, len(coefs) - 1, int(rng.integers(0, len(coefs)))}:
        for step in (-1, 1):
            if 0 <= int(coefs[b, 0]) // 8 + 128 + step <= 255:
                moved = coefs.copy()
                moved[b, 0] += 8 * step
                assert jm.huffman(moved, comp, bpm, R) != body, (b, step)
    # the edge set is in there: ties, both clamps, NaN and the infinities, -0.0, subnormals, the FMA-sensitive inputs
    e = tm.as_float32(grid.reshape(-1), dtype)
    assert np.isnan(e).any() and np.isposinf(e).any() and np.isneginf(e).any() and (np.signbit(e) & (e == 0)).any()
    if dtype == "float16":
        assert ((grid & 0x7C00 == 0) & (grid & 0x03FF != 0)).any()
    assert tm.fma_differs(e[:, None], scale, offset).any()
    assert (pb == 0).any() and (pb == 255).any()
    _trusted[dtype, ti] = want
    return want


@gpu_test
@pytest.mark.parametrize("ti", range(len(TRIPLES)))
@pytest.mark.parametrize("layout", ["contiguous", "channels_last"])
@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_every_block_shows_its_pixel_value(vali, gpu, enc, dtype, layout, ti):
    want = expected_block_file(dtype, ti)
    bits, _ = block_image(dtype)
    ctx = enc.Context(100, vali.YUV444)
    got = run_tensor(vali, enc, ctx, device_tensor(bits, dtype, layout, gpu), *TRIPLES[ti])[0]
    if got != want:
        a = dm.entropy_decode(dm.parse(got))
        b = dm.entropy_decode(dm.parse(want))
        bad = [(c, *np.argwhere(a[c][..., 0] != b[c][..., 0])[0]) for c in range(3) if (a[c][..., 0] != b[c][..., 0]).any()]
        c, y, x = bad[0]
        raise AssertionError(f"{dtype} {layout}: channel {c} block ({x}, {y}): p = {a[c][y, x, 0] / 8 + 128}, "
                             f"the definition gives {b[c][y, x, 0] // 8 + 128}")


# ---- 3. against the independent implementation --------------------------------------------------------------------------------
def _decoded(data, mode):
    im = PIL.open(io.BytesIO(data))
    if mode == "YCbCr":
        im.draft("YCbCr", im.size)
    im.load()
    assert im.mode == mode
    return np.asarray(im)


@gpu_test
@pytest.mark.parametrize("coding", [("RGB", "444"), ("RGB", "422"), ("RGB", "420"), ("YUV444", "444")], ids="-".join)
@pytest.mark.parametrize("dtype", tm.DTYPES)
def test_decodes_like_the_cpu_backend(vali, gpu, enc, cpu_enc, dtype, coding):
    fmt, samp = coding
    w, h, n = 33, 31, 2
    given, (scale, offset) = pair_of(None if dtype == "uint8" else 1, dtype)
    bits = tm.noise_bits(dtype, (n, h, w, 3), scale, offset, seed=11)
    p = tm.quantise(tm.as_float32(bits, dtype), scale, offset)
    mode = "YCbCr" if fmt == "YUV444" else "RGB"
    for layout in ("slice", "channels_last"):                  # one planar and one channels-last tensor
        t = device_tensor(bits, dtype, layout, gpu)
        ctx = enc.Context(90, getattr(vali, fmt), subsampling=samp)
        ours = run_tensor(vali, enc, ctx, t, *given)
        theirs = run_tensor(vali, cpu_enc, ctx, t, *given)
        for i in range(n):
            assert theirs[i] == jm_pillow(fmt, p[i], w, h, samp)
            a, b = _decoded(ours[i], mode), _decoded(theirs[i], mode)
            assert np.array_equal(a, b), (dtype, coding, layout, i)


def jm_pillow(fmt, p, w, h, samp):
    """Pillow's file for the model's pixels: what the cpu backend must have written"""
    import jpeg_subsample_model as sm

    if fmt == "YUV444":
        return jm.pillow_encode(jm.YUV444, host_of(fmt, p), w, h, 90)
    return sm.pillow_encode(jm.RGB, host_of(fmt, p), w, h, 90, samp)


# ---- 4. contract --------------------------------------------------------------------------------------------------------------
class _OnAnotherDevice:
    """a device array that says it lives on GPU 1 (never dereferenced)"""
    device = types.SimpleNamespace(type="cuda", index=1)
    __cuda_array_interface__ = {"shape": (1, 3, 8, 8), "typestr": "<f2", "data": (4096, False), "version": 3}


@gpu_test
def test_subsampled_yuv_contexts_fail(vali, gpu, enc, cpu_enc):
    t = torch.zeros((1, 3, 16, 16), dtype=torch.float16, device=f"cuda:{gpu}")
    for e in (enc, cpu_enc):
        for fmt in (vali.YUV420, vali.YUV422):
            assert e.RunTensor(e.Context(90, fmt), t) == ([], vali.TaskExecInfo.FAIL)


@gpu_test
def test_what_is_no_tensor_of_this_gpu_is_a_value_error(vali, gpu, enc):
    ctx = enc.Context(90, vali.RGB)
    dev = f"cuda:{gpu}"
    good = torch.zeros((2, 3, 8, 10), dtype=torch.float16, device=dev)
    for t, what in ((good.cpu(), "GPU"), (_OnAnotherDevice(), "device 1"),
                    (torch.zeros((2, 4, 8, 10), dtype=torch.float16, device=dev), "C = 4"),
                    (torch.zeros((2, 1, 8, 10), dtype=torch.uint8, device=dev), "C = 1"),
                    (good.transpose(2, 3), "transposed"), (good[:, :, :, ::2], "strided"),
                    (torch.zeros((2, 3, 8, 10), dtype=torch.float64, device=dev), "dtype")):
        with pytest.raises(ValueError, match=what):
            enc.RunTensor(ctx, t)
    for kw in (dict(scale=float("nan")), dict(scale=(255.0, float("inf"), 255.0)), dict(offset=float("-inf"))):
        with pytest.raises(ValueError, match="finite"):
            enc.RunTensor(ctx, good, **kw)


@gpu_test
def test_surfaces_before_and_after_a_tensor_give_the_same_files(vali, gpu):
    """the grown buffers and the cached headers are shared between Run and RunTensor"""
    enc = vali.PyNvJpegEncoder(gpu, backend="hip")
    ctx = enc.Context(90, vali.RGB, subsampling="420")
    w, h = 33, 31
    host = jm.make_host(jm.RGB, w, h, "noise", seed=3)
    small = upload(vali, gpu, "RGB", host, w, h)
    before = run_surfaces(vali, enc, ctx, [small])
    bits = tm.noise_bits("bfloat16", (3, BIG[1], BIG[0], 3), (255.0,) * 3, (0.0,) * 3, seed=4)
    t = device_tensor(bits, "bfloat16", "channels_last", gpu)
    first = run_tensor(vali, enc, ctx, t)                       # grows every buffer
    same = run_tensor(vali, enc, ctx, t[:, :, :h, :w])          # the size `small` has: its header comes from the cache
    assert run_surfaces(vali, enc, ctx, [small]) == before
    assert run_tensor(vali, enc, ctx, t) == first
    p = tm.quantise(tm.as_float32(bits[:, :h, :w], "bfloat16"), 255.0, 0.0)
    assert same == run_surfaces(vali, enc, ctx, [upload(vali, gpu, "RGB", host_of("RGB", p[i]), w, h) for i in range(3)])
    fresh = vali.PyNvJpegEncoder(gpu, backend="hip")
    assert run_surfaces(vali, fresh, ctx, [small]) == before


@gpu_test
def test_a_tensor_freed_right_after_the_call_is_fine(vali, gpu, enc):
    """RunTensor has synchronised and holds every file on the host when it returns (it keeps the tensor alive until
    then itself), so nothing the caller does to the tensor afterwards can reach the files: this pins that the result
    does not alias the tensor, not a race."""
    ctx = enc.Context(90, vali.BGR, subsampling="422")
    w, h = BIG
    bits = tm.noise_bits("float32", (2, h, w, 3), (255.0,) * 3, (0.0,) * 3, seed=9)
    want = run_tensor(vali, enc, ctx, device_tensor(bits, "float32", "contiguous", gpu))
    t = device_tensor(bits, "float32", "contiguous", gpu)
    out, info = enc.RunTensor(ctx, t)
    t.zero_()
    del t
    torch.cuda.synchronize()
    assert info == vali.TaskExecInfo.SUCCESS and [bytes(b.tobytes()) for b in out] == want
