"""PySurfacePostprocessor on the GPU: (N, 3, H, W) tensors straight into NV12, YUV420, YUV444, RGB and RGB_PLANAR surfaces.

Every comparison is bit-exact.  Expected bytes come from (a) the model (tests/postproc_model.py: the pinned quantiser,
then the CPU oracle) and, for the BT.601 matrices, (b) the chain the task replaces, run on the GPU with torch and
PySurfaceConverter.  With S = 16 the strip of pixels a lane owns, the sizes are the smallest that reach every path:
2x2 (narrower than a strip), Sx2 (one whole strip: vector loads, non-temporal stores), (S+2)x4 (a ragged tail),
(64S+S+2)x6 (more than one wave plus a tail), (64S+S)x2 (more than one wave on the aligned paths), and 1x1 and 7x5 for the
destinations that are not 4:2:0."""
import itertools

import numpy as np
import pytest

import jpeg_tensor_model as tm
import postproc_model as pm

torch = pytest.importorskip("torch")

gpu_test = pytest.mark.gpu

S = 16
FORMS = ("contiguous", "channels_last", "slice", "step")
EVEN_SIZES = ((2, 2), (S, 2), (S + 2, 4), (64 * S + S + 2, 6), (64 * S + S, 2))
ODD_SIZES = ((1, 1), (7, 5))
MATRICES = ("601_JPEG", "601_MPEG", "709_JPEG", "709_MPEG")
ESIZE = {"float32": 4, "float16": 2, "bfloat16": 2, "uint8": 1}


def _valid(case):
    dtype, form, dst, channels, matrix, n, (w, h) = case
    return not (dst in ("NV12", "YUV420") and (w | h) & 1)


def _load_paths(dtype, form, w):
    """which load paths a case reaches: "vec" when the rows start on the vector path's alignment (16 bytes, 4 for uint8)
    and a whole strip exists; "elem" for the strip the right edge cuts and for rows off that alignment"""
    es, packed = ESIZE[dtype], form == "channels_last"
    row = (3 * w if packed else w) * es
    aligned = form != "slice" and row % (4 if es == 1 else 16) == 0
    paths = set()
    if aligned and w >= S:
        paths.add("vec")
    if not aligned or w % S:
        paths.add("elem")
    return paths


def _wants(case):
    axes = case[:7]
    pairs = {(a, axes[a], b, axes[b]) for a in range(7) for b in range(a + 1, 7)}
    dtype, form, dst, _, _, _, (w, h) = case
    packed = form == "channels_last"
    kernel = {("kernel", dtype, packed, dst, p) for p in _load_paths(dtype, form, w)}
    store = {("store", dst, w % S == 0)}
    return pairs | kernel | store


def _cases():
    """A pairwise-covering subset of dtype x form x destination x channels x matrix x N x size (greedy, deterministic),
    which also reaches both load paths of every instantiation dtype x layout x destination and both store paths of
    every destination; the (scale, offset) pairs of tests/jpeg_tensor_model.py are dealt round afterwards."""
    space = [c for c in itertools.product(tm.DTYPES, FORMS, pm.DSTS, ("RGB", "BGR"), MATRICES, (1, 3),
                                          EVEN_SIZES + ODD_SIZES) if _valid(c)]
    wants = {c: _wants(c) for c in space}
    todo = set().union(*wants.values())
    cases = []
    while todo:
        best = max(space, key=lambda c: len(wants[c] & todo))
        cases.append(best)
        todo -= wants[best]
    out = []
    for k, c in enumerate(cases):
        pair = k % 4
        if c[0] == "uint8" and k % 3:
            pair = None
        out.append(c + (pair,))
    return out


CASES = _cases()


def _case_id(case):
    dtype, form, dst, channels, matrix, n, (w, h), pair = case
    return f"{dtype}-{form}-{dst}-{channels}-{matrix}-n{n}-{w}x{h}-s{pair}"


def test_cases_cover_every_pair_and_every_instantiation():
    axes = (tm.DTYPES, FORMS, pm.DSTS, ("RGB", "BGR"), MATRICES, (1, 3), EVEN_SIZES + ODD_SIZES)
    for a, b in itertools.combinations(range(7), 2):
        have = {(c[a], c[b]) for c in CASES}
        want = {(c[a], c[b]) for c in itertools.product(*axes) if _valid(c)}
        assert not want - have, (a, b, sorted(want - have, key=str)[:5])
    # every instantiation of k_tensor_to_surface on both of its load paths
    have = set()
    for c in CASES:
        have |= {(c[0], c[1] == "channels_last", c[2], p) for p in _load_paths(c[0], c[1], c[6][0])}
    assert have == set(itertools.product(tm.DTYPES, (False, True), pm.DSTS, ("vec", "elem")))
    # every destination on the non-temporal and on the ragged store path
    assert {(c[2], c[6][0] % S == 0) for c in CASES} == set(itertools.product(pm.DSTS, (False, True)))
    assert all(_valid(c[:7]) for c in CASES)
    assert len(CASES) <= 120


# ---- helpers ----------------------------------------------------------------------------------------------------------
def device_tensor(bits, dtype, form, gpu):
    """a GPU tensor of logical shape (N, 3, H, W) holding `bits` ((N, H, W, 3) bit patterns) in the given form"""
    dev = f"cuda:{gpu}"
    x = tm.torch_tensor(bits, dtype).permute(0, 3, 1, 2).contiguous().to(dev)
    n, _, h, w = x.shape
    if form == "contiguous":
        t = x
    elif form == "channels_last":
        t = x.contiguous(memory_format=torch.channels_last)
    elif form == "slice":
        # rows start one element off every vector boundary: the per-element path everywhere
        big = torch.full((n, 3, h + 2, w + 2), 77, dtype=x.dtype, device=dev)
        t = big[:, :, 1:1 + h, 1:1 + w]
        t.copy_(x)
    else:
        big = torch.full((2 * n, 3, h, w), 77, dtype=x.dtype, device=dev)
        t = big[::2]
        t.copy_(x)
    torch.cuda.synchronize()
    assert t.shape == x.shape
    return t


def noise_bits(dtype, shape, scale, offset, seed):
    """seeded noise (channels LAST) as bit patterns: after scale / offset it spreads over [-0.2, 1.2] x 255"""
    rng = np.random.default_rng(seed)
    if dtype == "uint8":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    want = rng.uniform(-0.2, 1.2, shape) * 255.0
    e = (want - np.asarray(offset, np.float64)) / np.asarray(scale, np.float64)
    t = torch.from_numpy(e.astype(np.float32))
    if dtype == "float32":
        return t.numpy().view(np.uint32)
    return t.to(torch.float16 if dtype == "float16" else torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def pair_of(pair, dtype):
    """(scale, offset) as RunTensorBatch takes them, and as the model does"""
    if pair is None:
        d = 1.0 if dtype == "uint8" else 255.0
        return (None, 0.0), ((d,) * 3, (0.0,) * 3)
    scale, offset = tm.SCALE_OFFSETS[pair]
    if pair < 3:
        return (scale[0], offset[0]), (scale, offset)
    return (scale, offset), (scale, offset)


def make_surfaces(vali, gpu, dst, n, w, h):
    return [vali.Surface.Make(getattr(vali, dst), w, h, gpu) for _ in range(n)]


def download(vali, gpu, s):
    host = np.zeros(s.HostSize, np.uint8)
    ok, info = vali.PySurfaceDownloader(gpu).Run(s, host)
    assert ok, info
    return host


@pytest.fixture(scope="module")
def post(vali, gpu):
    return vali.PySurfacePostprocessor(gpu)


def run(vali, post, t, dsts, scale=None, offset=0.0, cc_ctx=None, channels="RGB"):
    torch.cuda.synchronize()
    fb = post.PrepareTensorBatch(t, dsts)
    ok, info = post.RunTensorBatch(fb, scale, offset, cc_ctx, channels)
    assert ok and info == vali.TaskExecInfo.SUCCESS, info
    return fb


def first_difference(dst, got, want, w, h):
    for k, (a, b) in enumerate(zip(pm.planes_of(dst, got, w, h), pm.planes_of(dst, want, w, h))):
        if not np.array_equal(a, b):
            y, x = np.argwhere(a != b)[0]
            return f"plane {k} byte ({x}, {y}): got {a[y, x]}, the definition gives {b[y, x]}; {np.count_nonzero(a != b)} differ"
    return None


# ---- 1. the covering set against the model ----------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_surfaces_equal_the_model(vali, gpu, oracle, post, case):
    dtype, form, dst, channels, matrix, n, (w, h), pair = case
    given, (scale, offset) = pair_of(pair, dtype)
    bits = noise_bits(dtype, (n, h, w, 3), scale, offset, seed=w * 1000 + h)
    want = pm.model(oracle, bits, dtype, scale, offset, channels, dst, pm.matrices()[matrix])
    dsts = make_surfaces(vali, gpu, dst, n, w, h)
    run(vali, post, device_tensor(bits, dtype, form, gpu), dsts, *given, cc_ctx=pm.cc_ctx_of(vali, matrix),
        channels=channels)
    for i in range(n):
        got = download(vali, gpu, dsts[i])
        assert got.shape == want[i].shape
        assert np.array_equal(got, want[i]), (case, i, first_difference(dst, got, want[i], w, h))


# ---- 2. the values that matter: ties, NaN, infinities, FMA-sensitive inputs, all of uint8 -------------------------------
TRIPLES = (((255.0, tm.SCALE_OFFSETS[3][0][1], 127.5), (0.0, tm.SCALE_OFFSETS[3][1][1], 127.5)), tm.SCALE_OFFSETS[3])
EDGE_W = 66                                   # four whole strips and a ragged one


def edge_image(dtype):
    """(1, H, EDGE_W, 3) bit patterns: the dtype's edge set (every tie k + 0.5 under each (scale, offset) pair and its
    neighbours, NaN, +-inf, +-0, subnormals), the same value in all three channels (they differ in scale and offset)"""
    vals = tm.edge_bits(dtype)
    h = 2 * -(-vals.size // (2 * EDGE_W))
    grid = np.zeros(h * EDGE_W, vals.dtype)
    grid[:vals.size] = vals
    return np.repeat(grid.reshape(1, h, EDGE_W, 1), 3, 3)


@gpu_test
@pytest.mark.parametrize("ti", range(len(TRIPLES)))
@pytest.mark.parametrize("form", ["contiguous", "channels_last", "slice"])
@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_edge_values(vali, gpu, oracle, post, dtype, form, ti):
    scale, offset = TRIPLES[ti]
    bits = edge_image(dtype)
    h, w = bits.shape[1:3]
    e = tm.as_float32(bits[0, :, :, 0].reshape(-1), dtype)
    assert np.isnan(e).any() and np.isposinf(e).any() and np.isneginf(e).any() and (np.signbit(e) & (e == 0)).any()
    assert tm.fma_differs(e[:, None], scale, offset).any()          # a fused multiply-add would show
    p = pm.quantise(bits, dtype, scale, offset)
    assert (p == 0).any() and (p == 255).any()
    t = device_tensor(bits, dtype, form, gpu)
    for dst in ("RGB", "NV12"):
        want = pm.model(oracle, bits, dtype, scale, offset, "RGB", dst, pm.matrices()["601_JPEG"])[0]
        dsts = make_surfaces(vali, gpu, dst, 1, w, h)
        run(vali, post, t, dsts, scale, offset)
        got = download(vali, gpu, dsts[0])
        assert np.array_equal(got, want), (dtype, form, dst, first_difference(dst, got, want, w, h))


# Every exact tie k + 0.5, k = -1 .. 255, exactly representable in every dtype: the elements are small integers (at most
# 8 significant bits, bfloat16's), the scales powers of two and the offsets halves, so e * scale + offset is k + 0.5 with
# no rounding at all -- channel 0: k * 1 + 0.5; channel 1: 2k * 0.5 + 0.5; channel 2: (255 - k) * -1 + 255.5
TIE_SCALE, TIE_OFFSET = (1.0, 0.5, -1.0), (0.5, 0.5, 255.5)


@gpu_test
@pytest.mark.parametrize("form", ["contiguous", "channels_last", "slice"])
@pytest.mark.parametrize("dtype", tm.DTYPES)
def test_every_exact_tie(vali, gpu, oracle, post, dtype, form):
    lo = 0 if dtype == "uint8" else -1
    k = np.arange(lo, 256, dtype=np.float64)
    w = 34
    h = 2 * -(-k.size // (2 * w))
    pad = np.full(h * w - k.size, 100.0)
    kk = np.concatenate([k, pad])
    e = np.stack([kk, 2 * kk if dtype != "uint8" else kk, 255 - kk], -1).reshape(1, h, w, 3)
    scale = TIE_SCALE if dtype != "uint8" else (1.0, 1.0, -1.0)
    if dtype == "uint8":
        bits = e.astype(np.uint8)
    else:
        tt = torch.from_numpy(e.astype(np.float32))
        bits = (tt.numpy().view(np.uint32) if dtype == "float32" else
                tt.to(torch.float16 if dtype == "float16" else torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(tm.as_float32(bits, dtype), e.astype(np.float32))            # nothing was rounded
    p = pm.quantise(bits, dtype, scale, TIE_OFFSET)
    even = np.clip(kk + (kk % 2), 0, 255)                                              # k + 0.5 -> the even neighbour
    for c in range(3):
        assert np.array_equal(p[0, :, :, c].reshape(-1), even), c
    t = device_tensor(bits, dtype, form, gpu)
    for dst in ("RGB", "YUV444"):
        want = pm.model(oracle, bits, dtype, scale, TIE_OFFSET, "RGB", dst, pm.matrices()["601_JPEG"])[0]
        dsts = make_surfaces(vali, gpu, dst, 1, w, h)
        run(vali, post, t, dsts, scale, TIE_OFFSET)
        got = download(vali, gpu, dsts[0])
        assert np.array_equal(got, want), (dtype, form, dst, first_difference(dst, got, want, w, h))


@gpu_test
@pytest.mark.parametrize("form", ["contiguous", "channels_last", "slice"])
def test_uint8_picture_comes_back_exactly(vali, gpu, post, form):
    """a uint8 tensor that holds a picture, written to RGB, gives back exactly that picture: all 256 values, every
    channel"""
    w, h = 48, 18
    k = np.arange(h * w).reshape(h, w)
    pic = np.stack([k % 256, (k * 7 + 3) % 256, 255 - k % 256], -1).astype(np.uint8)
    for c in range(3):
        assert np.unique(pic[..., c]).size == 256
    t = device_tensor(pic[None], "uint8", form, gpu)
    rgb, planar = make_surfaces(vali, gpu, "RGB", 1, w, h), make_surfaces(vali, gpu, "RGB_PLANAR", 1, w, h)
    run(vali, post, t, rgb)
    run(vali, post, t, planar)
    assert np.array_equal(download(vali, gpu, rgb[0]).reshape(h, w, 3), pic)
    assert np.array_equal(download(vali, gpu, planar[0]).reshape(3, h, w), pic.transpose(2, 0, 1))
    bgr = make_surfaces(vali, gpu, "RGB", 1, w, h)
    run(vali, post, t, bgr, channels="BGR")
    assert np.array_equal(download(vali, gpu, bgr[0]).reshape(h, w, 3), pic[..., ::-1])


# ---- 3. the chain itself, on the GPU -----------------------------------------------------------------------------------
def chain(vali, gpu, t, scale, offset, dst, cc_ctx):
    """torch quantise -> Surface.from_dlpack(RGB) -> PySurfaceConverter RGB -> YUV420 (-> NV12) / YUV444, per item"""
    s = torch.tensor(scale, dtype=torch.float32, device=t.device).view(1, 3, 1, 1)
    o = torch.tensor(offset, dtype=torch.float32, device=t.device).view(1, 3, 1, 1)
    p = torch.nan_to_num(t.float() * s + o, nan=0.0).round().clamp(0, 255).to(torch.uint8)
    p = p.permute(0, 2, 3, 1).contiguous()
    n, h, w, _ = p.shape
    torch.cuda.synchronize()
    cvt = vali.PySurfaceConverter(gpu)
    out = []
    for i in range(n):
        rgb = vali.Surface.from_dlpack(p[i].view(h, 3 * w), vali.RGB)
        mid = vali.Surface.Make(vali.YUV444 if dst == "YUV444" else vali.YUV420, w, h, gpu)
        ok, info = cvt.Run(rgb, mid, cc_ctx)
        assert ok, info
        if dst == "NV12":
            nv = vali.Surface.Make(vali.NV12, w, h, gpu)
            ok, info = cvt.Run(mid, nv, cc_ctx)
            assert ok, info
            mid = nv
        out.append(download(vali, gpu, mid))
    return out


@gpu_test
@pytest.mark.parametrize("matrix", ["601_JPEG", "601_MPEG"])
@pytest.mark.parametrize("dst", ["NV12", "YUV420", "YUV444"])
@pytest.mark.parametrize("dtype", tm.DTYPES)
def test_equals_the_chain_it_replaces(vali, gpu, oracle, post, dtype, dst, matrix):
    w, h, n = 64 * S + S + 2, 6, 2
    given, (scale, offset) = pair_of(None if dtype == "uint8" else 1, dtype)
    bits = noise_bits(dtype, (n, h, w, 3), scale, offset, seed=21)
    t = device_tensor(bits, dtype, "contiguous", gpu)
    cc = pm.cc_ctx_of(vali, matrix)
    theirs = chain(vali, gpu, t, scale, offset, dst, cc)
    dsts = make_surfaces(vali, gpu, dst, n, w, h)
    run(vali, post, t, dsts, *given, cc_ctx=cc)
    want = pm.model(oracle, bits, dtype, scale, offset, "RGB", dst, pm.matrices()[matrix])
    for i in range(n):
        ours = download(vali, gpu, dsts[i])
        assert np.array_equal(ours, theirs[i]), (i, first_difference(dst, ours, theirs[i], w, h))
        assert np.array_equal(ours, want[i])


# ---- 4. destinations: views at odd addresses and pitches, and what lies around them --------------------------------------
VIEW_ROWS = {"NV12": lambda h: h * 3 // 2, "RGB": lambda h: h, "RGB_PLANAR": lambda h: 3 * h}
VIEW_COLS = {"NV12": lambda w: w, "RGB": lambda w: 3 * w, "RGB_PLANAR": lambda w: w}


@gpu_test
@pytest.mark.parametrize("size", [(2, 2), (S, 2), (S + 2, 4), (64 * S + S + 2, 6)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dst", ["NV12", "RGB", "RGB_PLANAR"])
def test_views_at_odd_addresses_and_the_guard_band(vali, gpu, oracle, post, dst, size):
    """from_dlpack views whose first byte and pitch are odd: the same bytes as an aligned surface gets, and the bytes
    between a row's end and the pitch, and a guard band around the view, stay as they were"""
    w, h = size
    n = 2
    rows, cols = VIEW_ROWS[dst](h), VIEW_COLS[dst](w)
    bits = noise_bits("float16", (n, h, w, 3), (255.0,) * 3, (0.0,) * 3, seed=w + h)
    want = pm.model(oracle, bits, "float16", (255.0,) * 3, (0.0,) * 3, "RGB", dst, pm.matrices()["709_MPEG"])
    t = device_tensor(bits, "float16", "contiguous", gpu)
    # odd address and odd pitch; odd address and rows that touch; an aligned address with an odd pitch
    for x0, pitch in ((3, (cols + 8) | 1), (1, cols + 1), (0, (cols + 6) | 1)):
        bufs = [torch.full((rows + 4, pitch), 0xA5, dtype=torch.uint8, device=f"cuda:{gpu}") for _ in range(n)]
        views = [b[2:2 + rows, x0:x0 + cols] for b in bufs]
        dsts = [vali.Surface.from_dlpack(v, getattr(vali, dst)) for v in views]
        assert all((d.Width, d.Height) == (w, h) for d in dsts)
        run(vali, post, t, dsts, cc_ctx=pm.cc_ctx_of(vali, "709_MPEG"))
        torch.cuda.synchronize()
        for i in range(n):
            buf = bufs[i].cpu().numpy()
            got = buf[2:2 + rows, x0:x0 + cols]
            assert np.array_equal(got.reshape(-1), want[i]), (x0, pitch, i)
            buf[2:2 + rows, x0:x0 + cols] = 0xA5
            assert (buf == 0xA5).all(), (x0, pitch, i, np.argwhere(buf != 0xA5)[:4])


@gpu_test
@pytest.mark.parametrize("dst", pm.DSTS)
def test_pitched_surfaces_keep_their_padding(vali, gpu, oracle, post, dst):
    """Surface.Make pads every row to its pitch: the bytes between the row's end and the pitch are not written"""
    from vali_amd._native import shim

    w, h = S + 2, 4
    bits = noise_bits("bfloat16", (1, h, w, 3), (255.0,) * 3, (0.0,) * 3, seed=5)
    s = make_surfaces(vali, gpu, dst, 1, w, h)[0]
    stream = post.Stream
    for p in s._planes:
        shim.memset2d_async(gpu, p.GpuMem, p.Pitch, 0x5A, p.Pitch, p.Height, stream)
    shim.stream_sync(gpu, stream)
    run(vali, post, device_tensor(bits, "bfloat16", "channels_last", gpu), [s])
    want = pm.model(oracle, bits, "bfloat16", (255.0,) * 3, (0.0,) * 3, "RGB", dst, pm.matrices()["601_JPEG"])[0]
    assert np.array_equal(download(vali, gpu, s), want)
    for p in s._planes:
        raw = np.zeros((p.Height, p.Pitch), np.uint8)
        hp, _, _ = shim.buffer_info(raw, True)
        shim.memcpy2d_async(gpu, hp, p.Pitch, p.GpuMem, p.Pitch, p.Pitch, p.Height, 1, stream)
        shim.stream_sync(gpu, stream)
        used = p.Width * p.ElemSize
        assert p.Pitch > used
        assert (raw[:, used:] == 0x5A).all()


# ---- 5. round trips ----------------------------------------------------------------------------------------------------
@gpu_test
def test_capture_and_replay(vali, gpu, oracle):
    from vali_amd._native import shim

    w, h, n = 64 * S + S + 2, 6, 3
    stream = shim.stream_create(gpu)
    post = vali.PySurfacePostprocessor(gpu, stream)
    bits = [noise_bits("float16", (n, h, w, 3), (255.0,) * 3, (0.0,) * 3, seed=s) for s in (31, 32)]
    t = device_tensor(bits[0], "float16", "contiguous", gpu)
    dsts = make_surfaces(vali, gpu, "NV12", n, w, h)
    fb = post.PrepareTensorBatch(t, dsts)
    cap = vali.StreamCapture(stream, gpu)
    with cap:
        with pytest.raises(RuntimeError, match="capturing"):
            post.PrepareTensorBatch(t, dsts)
        assert post.RunTensorBatchAsync(fb)[0]              # a prepared batch records fine
    cap.Keep(fb)
    rows = pm.matrices()["601_JPEG"]
    for k in (0, 1, 0):                                   # replayed on new contents of the same tensor
        t.copy_(device_tensor(bits[k], "float16", "contiguous", gpu))
        torch.cuda.synchronize()
        for d in dsts:
            pl = d._planes[0]
            shim.memset2d_async(gpu, pl.GpuMem, pl.Pitch, 0, pl.Width, pl.Height, stream)
        cap.Launch()
        shim.stream_sync(gpu, stream)
        want = pm.model(oracle, bits[k], "float16", (255.0,) * 3, (0.0,) * 3, "RGB", "NV12", rows)
        for i in range(n):
            assert np.array_equal(download(vali, gpu, dsts[i]), want[i]), (k, i)


@gpu_test
def test_nv12_output_feeds_the_preprocessor(vali, gpu, post):
    """the example's loop: NV12 -> float16 tensor -> (a stand-in network) -> NV12 -> float16 tensor again"""
    from conftest import make_nv12

    w, h, n = 64, 32, 2
    pre = vali.PySurfacePreprocessor(gpu)
    srcs = []
    for i in range(n):
        s = vali.Surface.Make(vali.NV12, w, h, gpu)
        assert vali.PyFrameUploader(gpu).Run(make_nv12(w, h, i).reshape(-1), s)[0]
        srcs.append(s)
    x = torch.empty((n, 3, h, w), dtype=torch.float16, device=f"cuda:{gpu}")
    torch.cuda.synchronize()
    assert pre.RunTensorBatch(pre.PrepareTensorBatch(srcs, x))[0]
    y = (1.0 - x).contiguous()                             # the stand-in network
    outs = make_surfaces(vali, gpu, "NV12", n, w, h)
    run(vali, post, y, outs)
    z = torch.empty_like(x)
    torch.cuda.synchronize()
    assert pre.RunTensorBatch(pre.PrepareTensorBatch(outs, z))[0]
    torch.cuda.synchronize()
    assert torch.isfinite(z.float()).all()
    # an inverted picture went round: on average the two tensors mirror each other (colour conversion is lossy)
    assert abs(float((z.float() + x.float()).mean()) - 1.0) < 0.05
