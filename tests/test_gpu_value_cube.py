"""Every 8-bit colour kernel on ALL 2^24 input triples, byte for byte (tests/value_cube.py has the frames).

The other GPU tests choose shapes that reach code paths and fill them with noise; a slip in the colour arithmetic of one
instantiation (a contraction the definition does not make, rint where it truncates, a saturating pack where it wraps)
moves one byte in 10^4 to 10^6 and can pass them.  Here every case is ONE launch on a 4096 x 4096 frame that holds each
triple once -- or on its 4098 wide twin, which takes the whole cube through the byte-granular instantiation -- and the
comparison is np.array_equal on raw bytes: no tolerance, no excluded pixel.  The reference of each group is the one the
operator's own test file uses.

Instantiations driven through the full cube:
    1  k_nv12_rgb8<LAYOUT>            3 layouts x 4 contexts, + the ragged twin once per context
    2  k_cvt8<SRC, DST>               9 pairs with a colour matrix x every context they accept, + ragged per source format
    3  k_p16_to_nv12                  P10 and P12 on all 65,536 sample values (luma and both chroma members)
    4  k_ud_lean<OUT, 1, ...>         5 outputs, aligned and RAGGED
    5  k_nv12_preproc<true, OUT>      5 outputs x 3 colour variants (x 2 normalisations for the float ones)
    6  k_nv12_preproc_roi             RGB_32F_PLANAR canvas; float16 / bfloat16 tensors, planar and channels last
    7  k_tensor_to_surface<DT, PACKED, DST>   all 24 YUV instantiations, every (matrix, destination), + ragged per destination
    8  k_annotate's blend (div255)    every (v, c, a) in all six formats
"""
import numpy as np
import pytest

import annotate_model as am
import postproc_model as pm
import value_cube as vc
from test_gpu_convert import contexts
from test_gpu_preproc import chain_oracle

pytestmark = pytest.mark.gpu

H = vc.SIDE
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
NORMS = {"identity": (1.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), "imagenet": (1.0, MEAN, STD)}
# the colour variants of an NV12 source (tasks._nv12_variant): context -> (oracle variant number, its constants' name)
NV12_VARIANTS = {"default": (None, 2, "CSC_NPP_709HDTV"), "709_JPEG": (("BT_709", "JPEG"), 2, "CSC_NPP_709HDTV"),
                 "709_MPEG": (("BT_709", "MPEG"), 1, "CSC_NPP_709CSC"), "601_JPEG": (("BT_601", "JPEG"), 0, "CSC_NPP_YUV")}
F32 = ("RGB_32F", "RGB_32F_PLANAR")


@pytest.fixture(scope="module", autouse=True)
def release_the_cubes():
    """up to 1 GiB of cubes and references live while this module runs; the rest of the suite does not need them"""
    yield
    vc.forget()


# ---- helpers ------------------------------------------------------------------------------------------------------------
def cc_of(vali, key):
    if key is None:
        return None
    return vali.ColorspaceConversionContext(getattr(vali.ColorSpace, key[0]), getattr(vali.ColorRange, key[1]))


def upload(vali, gpu, fmt, w, h, host):
    s = vali.Surface.Make(vali.PixelFormat[fmt], w, h, gpu)
    flat = np.asarray(host).reshape(-1).view(np.uint8)
    assert flat.size == s.HostSize, (fmt, w, h, flat.size, s.HostSize)
    ok, info = vali.PyFrameUploader(gpu).Run(flat, s)
    assert ok, info
    return s


def download(vali, gpu, s):
    out = np.zeros(s.HostSize, np.uint8)
    ok, info = vali.PySurfaceDownloader(gpu).Run(s, out)
    assert ok, info
    return out.view(np.float32) if s.Format.name in F32 else out


def nv12_source(vali, gpu, ragged=False):
    nv = vc.nv12_cube(ragged)
    return nv, upload(vali, gpu, "NV12", nv.shape[1], H, nv)


def oracle_nv12_rgb(oracle, variant, layout, ragged):
    nv = vc.nv12_cube(ragged)
    return vc.memo(("nv12_rgb", variant, layout, ragged),
                   lambda: oracle.nv12_to_rgb(nv, nv.shape[1], H, oracle.csc(variant), layout).reshape(-1))


def oracle_chain(oracle, variant, norm):
    """(3, H, W) float32: oracle.nv12_to_rgb, then the float32 numpy statement of divide + Normalize"""
    from vali_amd import tasks

    coeffs = getattr(tasks, {v[1]: v[2] for v in NV12_VARIANTS.values()}[variant])
    return vc.memo(("chain", variant, norm),
                   lambda: chain_oracle(oracle, vc.nv12_cube(), H, H, H, H, coeffs, *NORMS[norm]))


def as_layout(chw, fmt):
    """a (3, H, W) reference as the flat host image of a packed or planar destination"""
    return np.ascontiguousarray(chw.transpose(1, 2, 0)).reshape(-1) if fmt in ("RGB_32F", "RGB") else chw.reshape(-1)


# ---- 1. PySurfaceConverter NV12 -> RGB / BGR / RGB_PLANAR: k_nv12_rgb8<LAYOUT> ---------------------------------------------
RAGGED_LAYOUT = {"default": "RGB", "709_JPEG": "BGR", "709_MPEG": "RGB_PLANAR", "601_JPEG": "RGB"}
NV12_RGB_CASES = [(ctx, layout, False) for ctx in NV12_VARIANTS for layout in ("RGB", "BGR", "RGB_PLANAR")] + \
                 [(ctx, layout, True) for ctx, layout in RAGGED_LAYOUT.items()]


@pytest.mark.parametrize("ctx,layout,ragged", NV12_RGB_CASES,
                         ids=[f"{c}-{l}-{'ragged' if r else 'aligned'}" for c, l, r in NV12_RGB_CASES])
def test_nv12_to_rgb_on_every_triple(vali, gpu, oracle, ctx, layout, ragged):
    key, variant, _ = NV12_VARIANTS[ctx]
    accepted = contexts("NV12", layout)          # tests/test_gpu_convert.py: the four contexts and their oracle variants
    ck = None if key is None else (getattr(vali.ColorSpace, key[0]), getattr(vali.ColorRange, key[1]))
    assert len(accepted) == len(NV12_VARIANTS) and accepted[ck] == dict(csc_variant=variant)
    nv, src = nv12_source(vali, gpu, ragged)
    w = nv.shape[1]
    dst = vali.Surface.Make(vali.PixelFormat[layout], w, H, gpu)
    ok, info = vali.PySurfaceConverter(gpu).Run(src, dst, cc_of(vali, key))
    assert ok and info == vali.TaskExecInfo.SUCCESS, info
    vc.assert_same(download(vali, gpu, dst), oracle_nv12_rgb(oracle, variant, layout, ragged), layout, w, H,
                   vc.nv12_triple_at(nv), f"NV12 -> {layout}, {ctx}")


# ---- 2. PySurfaceConverter, every other pair with a colour matrix: k_cvt8<SRC, DST> ----------------------------------------
CVT_PAIRS = [("YUV420", "RGB"), ("YUV420", "BGR"), ("YUV444", "BGR"), ("YUV444", "RGB"), ("RGB", "YUV444"),
             ("RGB", "YUV420"), ("BGR", "YUV444"), ("RGB_PLANAR", "YUV444"), ("RGB", "Y")]
CVT_RAGGED = [("YUV420", "RGB"), ("YUV444", "BGR"), ("RGB", "YUV420"), ("BGR", "YUV444"), ("RGB_PLANAR", "YUV444")]


def test_the_pairs_are_all_that_take_a_colour_matrix(vali):
    have = set()
    for s, d in vali.PySurfaceConverter.Conversions():
        if any(contexts(s.name, d.name).values()) and s.name != "NV12":
            have.add((s.name, d.name))
    assert have == set(CVT_PAIRS)
    assert {s for s, _ in CVT_RAGGED} == {s for s, _ in CVT_PAIRS}


def source_triple_at(fmt, ragged):
    if fmt == "YUV420":
        return vc.nv12_triple_at(vc.nv12_cube(ragged))
    return vc.rgb_triple_at(vc.rgb_cube(ragged))       # RGB, BGR: the bytes in memory order; YUV444, RGB_PLANAR: plane order


def run_cvt_pair(vali, gpu, oracle, src, dst, ragged):
    w = vc.cube_width(ragged)
    host = vc.host_image(src, ragged)
    s = upload(vali, gpu, src, w, H, host)
    cvt = vali.PySurfaceConverter(gpu)
    for key, okw in contexts(src, dst).items():
        assert okw, (src, dst)
        d = vali.Surface.Make(vali.PixelFormat[dst], w, H, gpu)
        ok, info = cvt.Run(s, d, None if key is None else vali.ColorspaceConversionContext(*key))
        assert ok and info == vali.TaskExecInfo.SUCCESS, (src, dst, key, info)
        want = vc.memo(("convert", src, dst, tuple(sorted(okw.items())), ragged),
                       lambda: oracle.convert(host, src, dst, w, H, oracle.cvt_params(**okw)))
        vc.assert_same(download(vali, gpu, d), want, dst, w, H, source_triple_at(src, ragged),
                       f"{src} -> {dst}, {key}, {okw}")
        del d
        if ragged:
            break          # the twin once per source format: under the first context


@pytest.mark.parametrize("pair", CVT_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_convert_pairs_on_every_triple(vali, gpu, oracle, pair):
    """one launch per context the pair accepts (tests/test_gpu_convert.py: contexts)"""
    run_cvt_pair(vali, gpu, oracle, pair[0], pair[1], False)


@pytest.mark.parametrize("pair", CVT_RAGGED, ids=lambda p: f"{p[0]}-{p[1]}")
def test_convert_pairs_on_every_triple_ragged(vali, gpu, oracle, pair):
    run_cvt_pair(vali, gpu, oracle, pair[0], pair[1], True)


# ---- 3. P10 / P12 -> NV12: k_p16_to_nv12 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("src", ["P10", "P12"])
def test_p16_to_nv12_on_every_sample_value(vali, gpu, oracle, src):
    """all 65,536 sample values, the low bits set too, in the luma plane and in both members of the chroma pairs.  The
    oracle is the definition: min(255, (v + 128) >> 8)"""
    frame = vc.p16_frame()
    w, h = vc.P16_W, vc.P16_H
    host = frame.reshape(-1).view(np.uint8)
    s = upload(vali, gpu, src, w, h, host)
    d = vali.Surface.Make(vali.NV12, w, h, gpu)
    ok, info = vali.PySurfaceConverter(gpu).Run(s, d)
    assert ok and info == vali.TaskExecInfo.SUCCESS, info
    want = oracle.convert(host, src, "NV12", w, h, oracle.cvt_params())
    samples = frame.reshape(-1)
    assert np.array_equal(want, np.minimum((samples.astype(np.uint32) + 128) >> 8, 255).astype(np.uint8))
    report = vc.differences(download(vali, gpu, d), want, lambda i: f"sample {int(samples[i]):#06x} (element {i})")
    assert report is None, f"{src} -> NV12: {report}"


# ---- 4. PySurfaceUD at equal size: k_ud_lean<OUT, 1, ...> ------------------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True], ids=["aligned", "ragged"])
@pytest.mark.parametrize("dst", ["RGB", "RGB_PLANAR", "YUV444", "RGB_32F", "RGB_32F_PLANAR"])
def test_ud_same_size_on_every_source_triple(vali, gpu, oracle, dst, ragged):
    """UD interpolates chroma between the samples of the source even at equal size, so the colour stage's float inputs
    are not the source's bytes: this sweep is exhaustive in the SOURCE triples (every luma value under every chroma
    pair, with the cube's neighbours), not in the inputs of the colour arithmetic"""
    nv, src = nv12_source(vali, gpu, ragged)
    w = nv.shape[1]
    d = vali.Surface.Make(vali.PixelFormat[dst], w, H, gpu)
    ok, info = vali.PySurfaceUD(gpu).Run(src, d)
    assert ok and info == vali.TaskExecInfo.SUCCESS, info
    want = oracle.ud_nv12(nv, w, H, "NV12", w, H, dst).reshape(-1)
    vc.assert_same(download(vali, gpu, d), want, dst, w, H, vc.nv12_triple_at(nv), f"UD NV12 -> {dst}")


# ---- 5. PySurfacePreprocessor.Run at equal size: k_nv12_preproc<true, OUT> -------------------------------------------------
# ordered so that the cases which share a float32 reference are neighbours, the ImageNet ones (group 6 shares them) last
PREPROC_VARIANTS = ("default", "709_MPEG", "601_JPEG")
PREPROC_CASES = [(v, fmt, "identity") for v in PREPROC_VARIANTS for fmt in ("RGB", "BGR", "RGB_PLANAR")] + \
                [(v, fmt, norm) for norm in ("identity", "imagenet") for v in PREPROC_VARIANTS for fmt in F32]


@pytest.mark.parametrize("ctx,fmt,norm", PREPROC_CASES, ids=["-".join(c) for c in PREPROC_CASES])
def test_preproc_same_size_on_every_triple(vali, gpu, oracle, ctx, fmt, norm):
    key, variant, _ = NV12_VARIANTS[ctx]
    nv, src = nv12_source(vali, gpu)
    div, mean, std = NORMS[norm]
    dst = vali.Surface.Make(vali.PixelFormat[fmt], H, H, gpu)
    pp = vali.PySurfacePreprocessor(gpu, mean=mean, std=std, div=div)
    assert pp.Run(src, dst, cc_of(vali, key)) == (True, vali.TaskExecInfo.SUCCESS)
    if fmt in F32:
        want = as_layout(oracle_chain(oracle, variant, norm), fmt)
    else:
        want = oracle_nv12_rgb(oracle, variant, fmt, False)
    vc.assert_same(download(vali, gpu, dst), want, fmt, H, H, vc.nv12_triple_at(nv), f"preproc NV12 -> {fmt}, {ctx}, {norm}")


# ---- 6. RunRoi and RunTensorBatch, whole frame onto whole canvas: k_nv12_preproc_roi ---------------------------------------
def test_preproc_roi_on_every_triple(vali, gpu, oracle):
    key, variant, _ = NV12_VARIANTS["709_MPEG"]
    nv, src = nv12_source(vali, gpu)
    dst = vali.Surface.Make(vali.RGB_32F_PLANAR, H, H, gpu)
    div, mean, std = NORMS["imagenet"]
    pp = vali.PySurfacePreprocessor(gpu, mean=mean, std=std, div=div)
    assert pp.RunRoi(src, dst, None, None, None, cc_of(vali, key)) == (True, vali.TaskExecInfo.SUCCESS)
    want = oracle_chain(oracle, variant, "imagenet").reshape(-1)
    vc.assert_same(download(vali, gpu, dst), want, "RGB_32F_PLANAR", H, H, vc.nv12_triple_at(nv), "RunRoi, 709_MPEG, imagenet")


TENSOR_CASES = [("float16", "planar", "default"), ("bfloat16", "packed", "default"),
                ("float16", "packed", "601_JPEG"), ("bfloat16", "planar", "601_JPEG")]


@pytest.mark.parametrize("dtype,layout,ctx", TENSOR_CASES, ids=["-".join(c) for c in TENSOR_CASES])
def test_preproc_tensor_on_every_triple(vali, gpu, oracle, dtype, layout, ctx):
    """the float32 reference of group 5, then .to(dtype) by torch on the host: round to nearest even
    (tests/test_gpu_preproc_tensor.py)"""
    import torch

    key, variant, _ = NV12_VARIANTS[ctx]
    nv, src = nv12_source(vali, gpu)
    out = torch.full((1, 3, H, H), 7.0, dtype=getattr(torch, dtype), device=f"cuda:{gpu}")
    if layout == "packed":
        out = out.contiguous(memory_format=torch.channels_last)
    assert (layout == "packed") == (out.stride(1) == 1)
    torch.cuda.synchronize()
    div, mean, std = NORMS["imagenet"]
    pp = vali.PySurfacePreprocessor(gpu, mean=mean, std=std, div=div)
    batch = pp.PrepareTensorBatch([src], out)
    assert pp.RunTensorBatch(batch, None, cc_of(vali, key)) == (True, vali.TaskExecInfo.SUCCESS)
    torch.cuda.synchronize()
    ref32 = torch.from_numpy(np.array(oracle_chain(oracle, variant, "imagenet")))
    want = ref32.to(getattr(torch, dtype)).view(torch.int16).numpy().view(np.uint16)
    got = out[0].cpu().contiguous().view(torch.int16).numpy().view(np.uint16)
    vc.assert_same(got, want, "RGB_32F_PLANAR", H, H, vc.nv12_triple_at(nv), f"RunTensorBatch {dtype} {layout}, {ctx} (bits)")


# ---- 7. PySurfacePostprocessor.RunTensorBatch: k_tensor_to_surface<DT, PACKED, DST> ----------------------------------------
MATRICES = ("601_JPEG", "601_MPEG", "709_JPEG", "709_MPEG")
YUV_DSTS = ("NV12", "YUV420", "YUV444")


def _postproc_cases():
    """the 24 instantiations dtype x layout x destination; matrices dealt so that every (matrix, destination) occurs twice,
    once with an RGB and once with a BGR tensor; then the ragged twin once per destination"""
    combos = [(dt, lay) for dt in ("float32", "float16", "bfloat16", "uint8") for lay in ("planar", "packed")]
    cases = []
    for j, dst in enumerate(YUV_DSTS):
        for i, (dt, lay) in enumerate(combos):
            cases.append((dt, lay, dst, MATRICES[(i + j) % 4], "RGB" if i < 4 else "BGR", False))
    cases += [("float16", "planar", "NV12", "709_MPEG", "RGB", True), ("uint8", "packed", "YUV420", "601_JPEG", "BGR", True),
              ("bfloat16", "packed", "YUV444", "709_JPEG", "RGB", True)]
    return cases


POSTPROC_CASES = _postproc_cases()


def test_postproc_cases_cover_every_instantiation_and_every_matrix():
    aligned = [c for c in POSTPROC_CASES if not c[5]]
    assert len({c[:3] for c in aligned}) == 24
    assert {(c[3], c[2]) for c in aligned} == {(m, d) for m in MATRICES for d in YUV_DSTS}
    assert {(c[3], c[2], c[4]) for c in aligned} == {(m, d, ch) for m in MATRICES for d in YUV_DSTS for ch in ("RGB", "BGR")}
    assert sorted(c[2] for c in POSTPROC_CASES if c[5]) == sorted(YUV_DSTS)


@pytest.mark.parametrize("case", POSTPROC_CASES,
                         ids=["-".join(c[:5]) + ("-ragged" if c[5] else "-aligned") for c in POSTPROC_CASES])
def test_postproc_on_every_triple(vali, gpu, oracle, case):
    """a tensor that holds rgb_cube() under scale 1, offset 0: 0 .. 255 are exact in all four dtypes, so the quantiser
    returns them as they are and the colour stage sees every triple"""
    import torch

    dtype, layout, dst, matrix, channels, ragged = case
    cube = vc.rgb_cube(ragged)
    w = cube.shape[1]
    t = torch.from_numpy(np.array(cube)).to(f"cuda:{gpu}").permute(2, 0, 1)[None].to(getattr(torch, dtype))
    t = t.contiguous(memory_format=torch.channels_last) if layout == "packed" else t.contiguous()
    assert (layout == "packed") == (t.stride(1) == 1)
    assert torch.equal(t[0, :, 1234, 567].float().cpu(), torch.from_numpy(cube[1234, 567].astype(np.float32)))
    torch.cuda.synchronize()
    d = vali.Surface.Make(vali.PixelFormat[dst], w, H, gpu)
    post = vali.PySurfacePostprocessor(gpu)
    ok, info = post.RunTensorBatch(post.PrepareTensorBatch(t, [d]), 1.0, 0.0, pm.cc_ctx_of(vali, matrix), channels)
    assert ok and info == vali.TaskExecInfo.SUCCESS, info
    p = cube[..., ::-1] if channels == "BGR" else cube              # the tensor's channels, named
    want = vc.memo(("from_rgb", matrix, dst, channels, ragged), lambda: pm.from_rgb(oracle, p, dst, pm.matrices()[matrix]))
    vc.assert_same(download(vali, gpu, d), want, dst, w, H, vc.rgb_triple_at(p), f"tensor -> {dst}, {matrix}, {channels}")


# ---- 8. PySurfaceAnnotator's blend on every (v, c, a) ----------------------------------------------------------------------
ANN_W = 256                       # row x of a frame holds v = x
ANN_ROWS = am.MAX_MARKS           # marks per call: one row (two for 4:2:0) each
ANN_MATRIX = {"NV12": "601_JPEG", "YUV420": "709_MPEG", "YUV444": "601_MPEG", "RGB": "601_JPEG", "BGR": "601_JPEG",
              "RGB_PLANAR": "601_JPEG"}
ANN_CALLS = 4                     # calls per test: 4 tests x 4 calls x 4096 marks = the 65,536 (c, a) pairs


def ramp_frame(fmt, h):
    """v = x in every stored channel (the 4:2:0 chroma planes are 128 wide: v = x there too)"""
    flat = np.zeros(am.host_size(fmt, ANN_W, h), np.uint8)
    for view, _, _ in am.channels(fmt, flat, ANN_W, h):
        view[...] = np.arange(view.shape[1], dtype=np.uint8)[None, :]
    return flat


@pytest.mark.parametrize("part", range(16 // ANN_CALLS))
@pytest.mark.parametrize("fmt", am.FORMATS)
def test_annotate_blend_on_every_value(vali, gpu, fmt, part):
    """v' = (v * (255 - a) + c * a + 127) / 255 for every v, c, a: mark k = 256 c + a fills row k (rows 2k, 2k + 1 of a
    4:2:0 frame) with the colour (c, c, c) and alpha a.  For the RGB formats c is the colour itself, so (v, c, a) is
    exhaustive; for the YUV formats c is what the matrix makes of that grey, and (v, a) is exhaustive"""
    import torch

    step = 2 if fmt in am.S420 else 1
    h = ANN_ROWS * step
    sizes = [(ANN_W, h)] * ANN_CALLS
    ramp = ramp_frame(fmt, h)
    hosts = [ramp.copy() for _ in sizes]
    surfs = [upload(vali, gpu, fmt, ANN_W, h, ramp) for _ in sizes]
    ann = vali.PySurfaceAnnotator(gpu)
    batch = ann.PrepareBatch(surfs)
    cc = pm.cc_ctx_of(vali, ANN_MATRIX[fmt])
    rows = []
    for f in range(ANN_CALLS):
        k0 = (part * ANN_CALLS + f) * ANN_ROWS
        call = [(f, 0, r * step, ANN_W, step, am.FILL, 0, am.pack_colour((k0 + r) >> 8, (k0 + r) >> 8, (k0 + r) >> 8, (k0 + r) & 255))
                for r in range(ANN_ROWS)]
        marks = torch.from_numpy(np.asarray(call, np.int64).astype(np.int32)).to(f"cuda:{gpu}")
        torch.cuda.synchronize()
        ok, info = ann.RunBatch(batch, marks, cc)
        assert ok and info == vali.TaskExecInfo.SUCCESS, info
        rows += call
    assert len(am.apply(hosts, fmt, sizes, rows, pm.matrices()[ANN_MATRIX[fmt]])) == len(rows)
    for f, s in enumerate(surfs):
        def describe(i, f=f):
            x, y, ch = vc.locate(fmt, ANN_W, h, i)
            k = (part * ANN_CALLS + f) * ANN_ROWS + y // step
            return f"(v {int(ramp[i])}, c {k >> 8}, a {k & 255}) at ({x}, {y}) {ch}"
        report = vc.differences(download(vali, gpu, s), hosts[f], describe)
        assert report is None, f"{fmt} frame {f}: {report}"
