"""The fused preprocessor into ONE batch tensor on the GPU (vali_nv12_preproc_roi_tensor / vali_rgb_preproc_roi_tensor).

The oracle is the library's own surface path: PrepareRoiBatch + RunRoiBatch into RGB_32F_PLANAR surfaces pre-filled with
7.0, stacked, `.to(dtype)` (torch on the host: IEEE round-to-nearest-even, subnormals kept).  The tensor, also pre-filled
with 7.0, must equal it BIT FOR BIT: the comparison is torch.equal on the integer view, no tolerance.  The float32
surface result of a case is computed once and shared by the dtypes and layouts that check against it."""
import numpy as np
import pytest

from conftest import make_nv12

pytestmark = pytest.mark.gpu

FILL = 7.0
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
NORMS = {
    "identity": (1.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
    "imagenet": (1.0, MEAN, STD),
    "tiny": (1.0, (0.0, 0.0, 0.0), (1.0, 1e4, 1e6)),       # float16: subnormals, and values under half the smallest one
    "huge": (1.0, (0.0, 0.0, 0.0), (1e-5, 1.0, 1.0)),      # float16: overflow to inf
}
DTYPES = ("float32", "float16", "bfloat16")
LAYOUTS = ("planar", "packed")
PAD = (114, 114, 114)
# through "huge" R = 200 overflows float16; through "tiny" G = 1 is a float16 subnormal and B = 3 lies under half the smallest
NORM_PAD = (200, 1, 3)


# ---- helpers ---------------------------------------------------------------------------------------------------
def _bits(t):
    import torch

    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    import torch

    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def nv12_source(vali, gpu, w, h, seed):
    s = vali.Surface.Make(vali.NV12, w, h, gpu)
    assert vali.PyFrameUploader(gpu).Run(make_nv12(w, h, seed).reshape(-1), s)[0]
    return s


def rgb_source(vali, gpu, sfmt, w, h, seed):
    """a colour image stored as the source format stores it; the COLOURS are the same for the three formats"""
    img = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    mem = {"RGB": img, "BGR": img[..., ::-1], "RGB_PLANAR": img.transpose(2, 0, 1)}[sfmt]
    s = vali.Surface.Make(getattr(vali.PixelFormat, sfmt), w, h, gpu)
    assert vali.PyFrameUploader(gpu).Run(np.ascontiguousarray(mem).reshape(-1), s)[0]
    return s


def preprocessor(vali, gpu, norm):
    div, mean, std = NORMS[norm]
    return vali.PySurfacePreprocessor(gpu, mean=mean, std=std, div=div)


def surface_path(vali, gpu, pp, srcs, size, src_rects, dst_rects, pad, cc=None, rects=None):
    """the oracle before the conversion: (N, 3, H, W) float32 on the host, 7.0 where nothing was written"""
    import torch

    w, h = size
    seven = np.full(3 * h * w, FILL, np.float32).view(np.uint8)
    up, down = vali.PyFrameUploader(gpu), vali.PySurfaceDownloader(gpu)
    dsts = [vali.Surface.Make(vali.RGB_32F_PLANAR, w, h, gpu) for _ in srcs]
    for d in dsts:
        assert up.Run(seven, d)[0]
    batch = pp.PrepareRoiBatch(srcs, dsts, src_rects, dst_rects)
    assert pp.RunRoiBatch(batch, pad, cc, rects) == (True, vali.TaskExecInfo.SUCCESS)
    out = np.zeros((len(srcs), 3, h, w), np.float32)
    for i, d in enumerate(dsts):
        raw = np.zeros(d.HostSize, np.uint8)
        assert down.Run(d, raw)[0]
        out[i] = raw.view(np.float32).reshape(3, h, w)
    return torch.from_numpy(out)


def new_tensor(n, size, dtype, layout, shape="plain"):
    """(the tensor to fill, the allocation it lives in): 7.0 everywhere.  shape: plain; inner = [:, :, 1:1+H, 1:1+W] of
    a larger allocation (rows start 2 or 4 bytes off the 8-byte grid); every_other = [::2]"""
    import torch

    w, h = size
    dims = {"plain": (n, 3, h, w), "inner": (n, 3, h + 3, w + 3), "every_other": (2 * n, 3, h, w)}[shape]
    big = torch.full(dims, FILL, dtype=getattr(torch, dtype), device="cuda:0")
    if layout == "packed":
        big = big.contiguous(memory_format=torch.channels_last)
    view = {"plain": big, "inner": big[:, :, 1:1 + h, 1:1 + w], "every_other": big[::2]}[shape]
    torch.cuda.synchronize()
    return view, big


def tensor_path(vali, pp, srcs, out, src_rects, dst_rects, pad, cc=None, rects=None):
    import torch

    batch = pp.PrepareTensorBatch(srcs, out, src_rects, dst_rects)
    assert len(batch) == len(srcs)
    assert pp.RunTensorBatch(batch, pad, cc, rects) == (True, vali.TaskExecInfo.SUCCESS)
    torch.cuda.synchronize()
    return out.cpu()


_ORACLES = {}


def oracle_f32(key, make):
    if key not in _ORACLES:
        _ORACLES[key] = make()
    return _ORACLES[key]


def check(vali, gpu, key, norm, srcs, size, src_rects, dst_rects, pad, dtype, layout, shape="plain", cc=None):
    import torch

    pp = preprocessor(vali, gpu, norm)
    ref32 = oracle_f32((key, norm), lambda: surface_path(vali, gpu, pp, srcs, size, src_rects, dst_rects, pad, cc))
    ref = ref32.to(getattr(torch, dtype))
    out, big = new_tensor(len(srcs), size, dtype, layout, shape)
    assert (layout == "packed") == (out.stride(1) == 1)
    got = tensor_path(vali, pp, srcs, out, src_rects, dst_rects, pad, cc)
    assert same_bits(got, ref), f"{int((_bits(got) != _bits(ref)).sum())} elements differ"
    return ref32, ref, got, big


# ---- geometries ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_nv12_tall_tile_letterbox(vali, gpu, dtype, layout):
    sizes = [(64, 48), (130, 34), (322, 50)]
    srcs = [nv12_source(vali, gpu, w, h, seed=i) for i, (w, h) in enumerate(sizes)]
    place = [vali.letterbox_rect(w, h, 64, 32) for w, h in sizes]
    ref32, _, _, _ = check(vali, gpu, "nv12_tall", "imagenet", srcs, (64, 32), None, place, PAD, dtype, layout)
    assert not (ref32 == FILL).any()          # padding on: every element was written


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_nv12_wide_tile_crosses_1024(vali, gpu, dtype, layout):
    srcs = [nv12_source(vali, gpu, 1030, 4, seed=3), nv12_source(vali, gpu, 516, 2, seed=4)]
    check(vali, gpu, "nv12_wide", "imagenet", srcs, (1030, 4), None, None, PAD, dtype, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_nv12_ragged_width(vali, gpu, dtype, layout):
    srcs = [nv12_source(vali, gpu, 64, 48, seed=5), nv12_source(vali, gpu, 60, 30, seed=6)]
    check(vali, gpu, "nv12_ragged", "imagenet", srcs, (66, 34), None, [(2, 2, 60, 30)] * 2, PAD, dtype, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sfmt", ["RGB", "BGR", "RGB_PLANAR"])
def test_rgb_family_without_padding(vali, gpu, sfmt, dtype, layout):
    srcs = [rgb_source(vali, gpu, sfmt, 37, 23, seed=7), rgb_source(vali, gpu, sfmt, 5, 3, seed=8)]
    ref32, _, got, _ = check(vali, gpu, ("rgb", sfmt), "imagenet", srcs, (35, 19), None, [(3, 1, 29, 17)] * 2, None,
                             dtype, layout)
    outside = np.ones((19, 35), bool)
    outside[1:18, 3:32] = False
    assert (got.float().numpy()[:, :, outside] == FILL).all()         # the 7.0 outside the placement survived
    assert not (got.float().numpy()[:, :, ~outside] == FILL).any()
    # the colours are named, not positioned: a BGR source lands as R, G, B -- the same values as the RGB source gives
    rgb32 = oracle_f32((("rgb", "RGB"), "imagenet"), lambda: surface_path(
        vali, gpu, preprocessor(vali, gpu, "imagenet"),
        [rgb_source(vali, gpu, "RGB", 37, 23, seed=7), rgb_source(vali, gpu, "RGB", 5, 3, seed=8)], (35, 19), None,
        [(3, 1, 29, 17)] * 2, None))
    assert same_bits(ref32, rgb32)


# ---- views -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["inner", "every_other"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", ["nv12", "rgb"])
def test_views_of_a_larger_allocation(vali, gpu, family, dtype, layout, shape):
    import torch

    if family == "nv12":
        srcs = [nv12_source(vali, gpu, 64, 48, seed=5), nv12_source(vali, gpu, 60, 30, seed=6)]
        args = ("nv12_ragged", "imagenet", srcs, (66, 34), None, [(2, 2, 60, 30)] * 2, PAD)
    else:
        srcs = [rgb_source(vali, gpu, "RGB", 37, 23, seed=7), rgb_source(vali, gpu, "RGB", 5, 3, seed=8)]
        args = (("rgb", "RGB"), "imagenet", srcs, (35, 19), None, [(3, 1, 29, 17)] * 2, None)
    w, h = args[3]
    _, ref, _, big = check(vali, gpu, *args, dtype, layout, shape)
    # the bytes of the allocation outside the view are unchanged
    expect = torch.full(big.shape, FILL, dtype=big.dtype)
    if shape == "inner":
        expect[:, :, 1:1 + h, 1:1 + w] = ref
    else:
        expect[::2] = ref
    assert same_bits(big.cpu().contiguous(), expect)


# ---- device rectangles -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", ["nv12", "rgb"])
def test_device_rects(vali, gpu, family, dtype, layout):
    import torch

    if family == "nv12":
        srcs = [nv12_source(vali, gpu, 64, 48, seed=i) for i in range(6)]
    else:
        srcs = [rgb_source(vali, gpu, "BGR", 63, 47, seed=i) for i in range(6)]
    size = (40, 24)
    rows = [[0, 0, 64, 48, 0, 0, 40, 24],            # plain
            [50, 40, 40, 40, 30, 20, 40, 40],        # both boxes hang over their frames
            [10, 10, 0, 0, 4, 4, 20, 10],            # an empty crop
            [10, 10, 20, 20, 4, 4, 0, 7],            # an empty placement
            [-6, -4, 30, 20, -8, -2, 30, 20],        # negative coordinates
            [7, 5, 21, 13, 3, 1, 27, 19]]            # odd values (NV12 rounds them to even)
    rects = torch.tensor(rows, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    pp = preprocessor(vali, gpu, "imagenet")
    ref32 = oracle_f32(("rects", family), lambda: surface_path(vali, gpu, pp, srcs, size, None, None, PAD, rects=rects))
    ref = ref32.to(getattr(torch, dtype))
    out, _ = new_tensor(len(srcs), size, dtype, layout)
    got = tensor_path(vali, pp, srcs, out, None, None, PAD, rects=rects)
    assert same_bits(got, ref)
    # and with padding off the empty items stay untouched
    ref32 = oracle_f32(("rects_nopad", family),
                       lambda: surface_path(vali, gpu, pp, srcs, size, None, None, None, rects=rects))
    assert (ref32[2] == FILL).all() and (ref32[3] == FILL).all()
    out, _ = new_tensor(len(srcs), size, dtype, layout)
    got = tensor_path(vali, pp, srcs, out, None, None, None, rects=rects)
    assert same_bits(got, ref32.to(getattr(torch, dtype)))


# ---- normalisations: rounding, subnormals, overflow ------------------------------------------------------------
def _truncated(ref32, dtype):
    """float32 -> dtype by chopping the mantissa (what a kernel that does not round would give); normal range only"""
    import torch

    if dtype == "bfloat16":
        return (ref32.view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16)
    f = ref32.to(torch.float16)
    over = f.float().abs() > ref32.abs()          # rounded away from zero: step one unit back
    return torch.where(over, (f.view(torch.int16) - 1).view(torch.float16), f)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm", list(NORMS))
@pytest.mark.parametrize("family", ["nv12", "rgb"])
def test_normalisations(vali, gpu, family, norm, dtype, layout):
    import torch

    if family == "nv12":
        srcs = [nv12_source(vali, gpu, 64, 48, seed=-1), nv12_source(vali, gpu, 32, 16, seed=9)]
        args = ("norm_nv12", norm, srcs, (48, 20), None, [(4, 2, 40, 16)] * 2, NORM_PAD)
    else:
        srcs = [rgb_source(vali, gpu, "RGB", 37, 23, seed=7), rgb_source(vali, gpu, "RGB", 5, 3, seed=8)]
        args = ("norm_rgb", norm, srcs, (35, 19), None, [(3, 1, 29, 17)] * 2, NORM_PAD)
    ref32, ref, got, _ = check(vali, gpu, *args, dtype, layout)
    if dtype == "float16" and norm == "tiny":
        mag = ref.float().abs()
        assert ((mag > 0) & (mag < 2.0 ** -14)).any(), "no subnormal float16 in the oracle"
        assert ((mag == 0) & (ref32 != 0)).any(), "nothing under half the smallest subnormal in the oracle"
    if dtype == "float16" and norm == "huge":
        assert torch.isinf(ref).any() and not torch.isinf(ref32).any()
    if dtype != "float32" and norm == "imagenet":
        assert not same_bits(_truncated(ref32, dtype), ref), "rounding and truncation agree: the case proves nothing"


# ---- float32: the tensor IS the surface path -------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", [1, 3])
def test_float32_tensor_equals_the_surfaces(vali, gpu, n, layout):
    sizes = [(64, 48), (130, 34), (322, 50)][:n]
    srcs = [nv12_source(vali, gpu, w, h, seed=i) for i, (w, h) in enumerate(sizes)]
    place = [vali.letterbox_rect(w, h, 64, 32) for w, h in sizes]
    cc = vali.ColorspaceConversionContext(vali.ColorSpace.BT_709, vali.ColorRange.MPEG)
    ref32, ref, got, _ = check(vali, gpu, ("f32", n), "imagenet", srcs, (64, 32), None, place, PAD, "float32", layout,
                               cc=cc)
    assert same_bits(got, ref32)


def test_whole_sources_without_records(vali, gpu):
    """d_roi == NULL in the C ABI: every item is its whole source onto the whole canvas (both entry points)"""
    import torch
    from vali_amd._native import shim

    for family in ("nv12", "rgb"):
        if family == "nv12":
            srcs = [nv12_source(vali, gpu, 64, 48, seed=1), nv12_source(vali, gpu, 130, 34, seed=2)]
        else:
            srcs = [rgb_source(vali, gpu, "BGR", 37, 23, seed=7), rgb_source(vali, gpu, "BGR", 5, 3, seed=8)]
        pp = preprocessor(vali, gpu, "imagenet")
        ref = surface_path(vali, gpu, pp, srcs, (34, 18), None, None, None).to(torch.float16)
        out, _ = new_tensor(2, (34, 18), "float16", "planar")
        batch = pp.PrepareTensorBatch(srcs, out)
        entry = shim.nv12_preproc_roi_tensor if family == "nv12" else shim.rgb_preproc_roi_tensor
        fmt = () if family == "nv12" else (int(vali.BGR),)
        assert entry(batch.d_src, 0, *fmt, batch.dst, pp._params(None), False, (0, 0, 0), pp.Stream) == 0
        shim.stream_sync(gpu, pp.Stream)
        assert same_bits(out.cpu(), ref)


# ---- status codes ----------------------------------------------------------------------------------------------
def test_status_codes_are_those_of_the_surface_path(vali, gpu):
    import torch

    srcs = [nv12_source(vali, gpu, 64, 48, seed=1), nv12_source(vali, gpu, 130, 34, seed=2)]
    dsts = [vali.Surface.Make(vali.RGB_32F_PLANAR, 64, 32, gpu) for _ in srcs]
    pp = preprocessor(vali, gpu, "imagenet")
    out, _ = new_tensor(2, (64, 32), "float16", "planar")
    tb, rb = pp.PrepareTensorBatch(srcs, out), pp.PrepareRoiBatch(srcs, dsts)
    bad_cc = vali.ColorspaceConversionContext(vali.ColorSpace.BT_601, vali.ColorRange.MPEG)
    want = pp.RunRoiBatch(rb, None, bad_cc)
    assert want == (False, vali.TaskExecInfo.UNSUPPORTED_FMT_CONV_PARAMS)
    assert pp.RunTensorBatch(tb, None, bad_cc) == want
    assert pp.RunTensorBatch(tb, (1, 2)) == pp.RunRoiBatch(rb, (1, 2)) == (False, vali.TaskExecInfo.INVALID_INPUT)
    assert (out.cpu() == FILL).all()          # nothing ran
    for bad in (torch.zeros((3, 8), dtype=torch.int32, device="cuda:0"),
                torch.zeros((2, 8), dtype=torch.int64, device="cuda:0"),
                torch.zeros((8, 2), dtype=torch.int32, device="cuda:0").t(),
                torch.zeros((2, 8), dtype=torch.int32)):
        with pytest.raises(ValueError):
            pp.RunRoiBatch(rb, rects=bad)
        with pytest.raises(ValueError):
            pp.RunTensorBatch(tb, rects=bad)
    # the tensor's N is the batch's size; one source format per batch; NV12 needs an even canvas
    with pytest.raises(ValueError):
        pp.PrepareTensorBatch(srcs[:1], out)
    with pytest.raises(ValueError, match="one format"):
        pp.PrepareTensorBatch([srcs[0], rgb_source(vali, gpu, "RGB", 8, 8, seed=1)], out)
    odd, _ = new_tensor(2, (63, 32), "float16", "planar")
    with pytest.raises(ValueError):
        pp.PrepareTensorBatch(srcs, odd)
    with pytest.raises(ValueError, match="TensorBatch"):
        pp.RunTensorBatch(rb)
