"""PyNvJpegEncoder.RunRoi on the GPU: rectangles of surfaces of any sizes in one call.  File i equals, byte for byte, the
file `Run` writes for an uploaded copy of rectangle i, and the numpy model (tests/jpeg_roi_model.py: crop, then the
models that are pinned to Pillow).  The surfaces are noise, so a neighbour read by mistake changes the file."""
import io
import re
from pathlib import Path

import numpy as np
import pytest

import jpeg_model as jm
import jpeg_roi_model as rm

PIL = pytest.importorskip("PIL.Image")
ROOT = Path(__file__).resolve().parent.parent

gpu_test = pytest.mark.gpu

NAMES = {jm.RGB: "RGB", jm.BGR: "BGR", jm.RGB_PLANAR: "RGB_PLANAR", jm.YUV444: "YUV444", jm.YUV422: "YUV422",
         jm.YUV420: "YUV420"}
# (format, sampling of the files): the RGB layouts at every sampling, planar YUV with its own
CODINGS = [(f, s) for f in rm.RGB_FORMATS for s in ("444", "422", "420")] + [(jm.YUV444, None), (jm.YUV422, None),
                                                                             (jm.YUV420, None)]
SW, SH = 168, 152                       # not a multiple of 16: the surface's own last MCU is partial at every sampling


def rects_for(fmt):
    """One call, in this order: 1 x 1 at the surface's last pixel; 8 x 8 at the origin; 17 x 9 (partial MCUs both ways at
    4:2:0); 136 x 136 (867 blocks at 4:4:4: several workgroups); 16 x 16 at an odd origin; a rectangle that ends on the
    surface's last column and row; the whole surface; one rectangle twice.  Small items stand next to large ones in both
    orders.  Planar 4:2:2 / 4:2:0 sources get the nearest even origins and sizes their chroma planes allow."""
    rects = [(SW - 1, SH - 1, 1, 1), (0, 0, 8, 8), (5, 3, 17, 9), (21, 11, 136, 136), (7, 13, 16, 16),
             (SW - 40, SH - 24, 40, 24), None, (33, 47, 24, 20), (33, 47, 24, 20)]
    ex = fmt in (jm.YUV422, jm.YUV420)
    ey = fmt == jm.YUV420

    def even(r):
        if r is None:
            return None
        x, y, w, h = r
        if ex:
            x, w = x - (x & 1), w + (w & 1)
        if ey:
            y, h = y - (y & 1), h + (h & 1)
        return (x, y, w, h)
    return [even(r) for r in rects]


def upload(vali, gpu, fmt, host, w, h):
    s = vali.Surface.Make(vali.PixelFormat(fmt), w, h, gpu)
    assert s.HostSize == host.size, (s.HostSize, host.size)
    ok, info = vali.PyFrameUploader(gpu).Run(host, s)
    assert ok, info
    return s


_SURFACES = {}


def source(vali, gpu, fmt, w=SW, h=SH, seed=0):
    """(host image, its surface): made once per format and size, never written again"""
    key = (fmt, w, h, seed)
    if key not in _SURFACES:
        host = jm.make_host(fmt, w, h, "noise", seed=1000 * fmt + w + h + seed)
        _SURFACES[key] = (host, upload(vali, gpu, fmt, host, w, h))
    return _SURFACES[key]


def run_roi(vali, enc, ctx, surfaces, rects):
    out, info = enc.RunRoi(ctx, surfaces, rects)
    assert info == vali.TaskExecInfo.SUCCESS
    assert len(out) == len(surfaces)
    return [bytes(b.tobytes()) for b in out]


@gpu_test
@pytest.mark.parametrize("optimize", [False, True], ids=["annexk", "optimize"])
@pytest.mark.parametrize("fmt, samp", CODINGS, ids=lambda v: NAMES.get(v, str(v)))
def test_files_equal_run_on_the_crop_and_the_model(vali, gpu, fmt, samp, optimize):
    host, surf = source(vali, gpu, fmt)
    rects = rects_for(fmt)
    crops = []
    for r in rects:
        x, y, w, h = r or (0, 0, SW, SH)
        crops.append((w, h, upload(vali, gpu, fmt, rm.crop(fmt, host, SW, SH, (x, y, w, h)), w, h)))
    enc = vali.PyNvJpegEncoder(gpu, backend="hip")
    for q in (1, 90, 100):
        ctx = enc.Context(q, vali.PixelFormat(fmt), subsampling=samp, optimize=optimize)
        got = run_roi(vali, enc, ctx, [surf] * len(rects), rects)
        for i, (r, (w, h, c)) in enumerate(zip(rects, crops)):
            alone, info = enc.Run(ctx, [c])
            assert info == vali.TaskExecInfo.SUCCESS
            assert got[i] == bytes(alone[0].tobytes()), (NAMES[fmt], samp, q, i, r)
            assert got[i] == rm.encode(fmt, host, SW, SH, r, q, samp, optimize), (NAMES[fmt], samp, q, i, r)
        assert got[-1] == got[-2]


@gpu_test
@pytest.mark.parametrize("optimize", [False, True], ids=["annexk", "optimize"])
def test_300_random_rectangles_on_three_surfaces(vali, gpu, optimize):
    sizes = [(256, 160), (97, 131), (64, 64)]
    srcs = [source(vali, gpu, jm.RGB, w, h, seed=k) for k, (w, h) in enumerate(sizes)]
    rng = np.random.default_rng(300)
    on, rects = [], []
    for _ in range(300):
        k = int(rng.integers(0, 3))
        w, h = (int(v) for v in rng.integers(1, 65, 2))
        x, y = int(rng.integers(0, sizes[k][0] - w + 1)), int(rng.integers(0, sizes[k][1] - h + 1))
        on.append(k)
        rects.append((x, y, w, h))
    enc = vali.PyNvJpegEncoder(gpu, backend="hip")
    for samp in ("420", "444"):
        ctx = enc.Context(75, vali.RGB, subsampling=samp, optimize=optimize)
        got = run_roi(vali, enc, ctx, [srcs[k][1] for k in on], rects)
        for i, (k, r) in enumerate(zip(on, rects)):
            assert got[i] == rm.encode(jm.RGB, srcs[k][0], *sizes[k], r, 75, samp, optimize), (samp, i, k, r)


@gpu_test
@pytest.mark.parametrize("fmt, samp", [(jm.RGB, "420"), (jm.RGB, "422"), (jm.BGR, "444"), (jm.RGB_PLANAR, "420")],
                         ids=lambda v: NAMES.get(v, str(v)))
def test_pitched_and_misaligned_dlpack_sources(vali, gpu, fmt, samp):
    """surfaces borrowed from a larger tensor: a pitched one (dword loads in the interior of an aligned rectangle) and a
    view whose rows start 7 bytes off a dword (byte loads everywhere)"""
    import torch

    w, h = 200, 121
    host = jm.make_host(fmt, w, h, "noise", seed=77)
    bpp, planes = (3, 1) if fmt != jm.RGB_PLANAR else (1, 3)
    rows = host.reshape(planes * h, bpp * w)
    big = torch.zeros((2 * planes * h + 8, bpp * w + 161), dtype=torch.uint8, device=f"cuda:{gpu}")
    big[:planes * h, :bpp * w] = torch.from_numpy(rows).to(big.device)
    off = planes * h + 5
    big[off:off + planes * h, 7:7 + bpp * w] = torch.from_numpy(rows).to(big.device)
    torch.cuda.synchronize()

    views = [big[:planes * h, :bpp * w], big[off:off + planes * h, 7:7 + bpp * w]]
    surfs = [vali.Surface.from_dlpack(torch.utils.dlpack.to_dlpack(v), vali.PixelFormat(fmt)) for v in views]
    for s in surfs:
        assert (s.Width, s.Height, s.Pitch) == (w, h, bpp * w + 161)
    rects = [(0, 0, 64, 64), (4, 8, 64, 40), (3, 5, 33, 17), (w - 9, h - 7, 9, 7), None, (1, 0, 199, 121)]
    enc = vali.PyNvJpegEncoder(gpu, backend="hip")
    ctx = enc.Context(90, vali.PixelFormat(fmt), subsampling=samp)
    want = [rm.encode(fmt, host, w, h, r, 90, samp) for r in rects]
    for s in surfs:
        assert run_roi(vali, enc, ctx, [s] * len(rects), rects) == want
    # both sources in one call
    assert run_roi(vali, enc, ctx, [surfs[i & 1] for i in range(len(rects))], rects) == want


@gpu_test
@pytest.mark.parametrize("fmt, samp", [(jm.RGB, "420"), (jm.RGB_PLANAR, "444"), (jm.YUV420, None), (jm.YUV422, None)],
                         ids=lambda v: NAMES.get(v, str(v)))
def test_files_decode_to_the_pixels_of_the_cpu_backend(vali, gpu, fmt, samp):
    host, surf = source(vali, gpu, fmt)
    rects = rects_for(fmt)
    hip, cpu = vali.PyNvJpegEncoder(gpu, backend="hip"), vali.PyNvJpegEncoder(gpu, backend="cpu")
    dec = vali.PyNvJpegDecoder(gpu)
    for optimize in (False, True):
        ctx = hip.Context(90, vali.PixelFormat(fmt), subsampling=samp, optimize=optimize)
        ours = run_roi(vali, hip, ctx, [surf] * len(rects), rects)
        theirs = run_roi(vali, cpu, ctx, [surf] * len(rects), rects)
        # the cpu backend is Run on the crop as well: Pillow on the cropped host image
        for r, t in zip(rects, theirs):
            x, y, w, h = r or (0, 0, SW, SH)
            out = io.BytesIO()
            cpu._image(vali.PixelFormat(fmt), w, h, rm.crop(fmt, host, SW, SH, (x, y, w, h))).save(
                out, format="JPEG", quality=90, subsampling={"444": 0, "422": 1, "420": 2}[ctx.Subsampling()],
                optimize=optimize)
            assert t == out.getvalue(), r
        for a, b in zip(ours, theirs):
            pa, pb = PIL.open(io.BytesIO(a)), PIL.open(io.BytesIO(b))
            assert pa.size == pb.size and pa.mode == pb.mode and pa.layer == pb.layer
            assert np.array_equal(np.asarray(pa), np.asarray(pb))
        sa, info = dec.Run(ours, vali.RGB)
        assert info == vali.TaskExecInfo.SUCCESS
        sb, info = dec.Run(theirs, vali.RGB)
        assert info == vali.TaskExecInfo.SUCCESS
        for x, y in zip(sa, sb):
            ga, gb = np.zeros(x.HostSize, np.uint8), np.zeros(y.HostSize, np.uint8)
            assert vali.PySurfaceDownloader(gpu).Run(x, ga)[0] and vali.PySurfaceDownloader(gpu).Run(y, gb)[0]
            assert (x.Width, x.Height) == (y.Width, y.Height) and np.array_equal(ga, gb)


@gpu_test
def test_run_and_run_tensor_are_what_they_were_after_run_roi(vali, gpu):
    """the encoder's buffers are shared: whole-surface calls before and after a RunRoi call on the same encoder"""
    import torch

    import jpeg_subsample_model as sm

    enc = vali.PyNvJpegEncoder(gpu, backend="hip")
    sizes = [(130, 70), (33, 31), (130, 70), (424, 232)]
    hosts = [jm.make_host(jm.RGB, w, h, "noise", seed=i) for i, (w, h) in enumerate(sizes)]
    surfs = [upload(vali, gpu, jm.RGB, hst, w, h) for hst, (w, h) in zip(hosts, sizes)]
    t = torch.from_numpy(np.stack([hosts[0].reshape(70, 130, 3), hosts[2].reshape(70, 130, 3)])).to(f"cuda:{gpu}")
    t = t.permute(0, 3, 1, 2).contiguous()
    torch.cuda.synchronize()
    yhost, ysurf = source(vali, gpu, jm.YUV420)

    def whole_surface_calls():
        out = []
        for samp, opt in (("420", False), ("444", True), ("422", False)):
            ctx = enc.Context(90, vali.RGB, subsampling=samp, optimize=opt)
            files, info = enc.Run(ctx, surfs)
            assert info == vali.TaskExecInfo.SUCCESS
            out += [bytes(f.tobytes()) for f in files]
            files, info = enc.RunTensor(ctx, t)
            assert info == vali.TaskExecInfo.SUCCESS
            out += [bytes(f.tobytes()) for f in files]
        files, info = enc.Run(enc.Context(75, vali.YUV420), [ysurf])
        assert info == vali.TaskExecInfo.SUCCESS
        return out + [bytes(files[0].tobytes())]

    before = whole_surface_calls()
    k = 0
    for samp, opt in (("420", False), ("444", True), ("422", False)):
        for i, (w, h) in enumerate(sizes):
            want = rm.encode_crop(jm.RGB, hosts[i], w, h, 90, samp, opt)
            assert before[k + i] == want, (samp, opt, i)
        assert before[k + 4] == before[k] and before[k + 5] == before[k + 2]      # the tensor's items are surfaces 0 and 2
        k += 6
    assert before[-1] == jm.encode(jm.YUV420, yhost, SW, SH, 75)
    ctx = enc.Context(90, vali.RGB, subsampling="420", optimize=True)
    rects = [(1, 1, 100, 60), None, (5, 5, 9, 9), (200, 100, 224, 132)]
    got = run_roi(vali, enc, ctx, surfs, rects)
    for i, r in enumerate(rects):
        assert got[i] == rm.encode(jm.RGB, hosts[i], *sizes[i], r, 90, "420", True), i
    assert whole_surface_calls() == before
    # refusals leave the encoder usable
    assert enc.RunRoi(ctx, [surfs[0], ysurf]) == ([], vali.TaskExecInfo.FAIL)
    with pytest.raises(ValueError, match="item 1.*does not lie inside"):
        enc.RunRoi(ctx, surfs[:2], [None, (30, 0, 8, 8)])
    with pytest.raises(ValueError, match="item 0.*even"):
        enc.RunRoi(enc.Context(90, vali.YUV420), [ysurf], [(1, 0, 8, 8)])
    assert run_roi(vali, enc, ctx, surfs, rects) == got


def test_the_new_kernels_use_no_scratch_and_the_old_ones_keep_their_occupancy():
    """the compiler's resource remarks of the build: the ten k_jpeg_fdct_roi forms and the four other _roi kernels exist,
    none uses scratch or spills, and every one runs at the occupancy of the kernel it stands beside"""
    report = ROOT / "vali_amd" / "csrc" / "_obj" / "jpeg.resources.txt"
    kernels, name = {}, None
    for line in report.read_text().splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (-?\d+)", line)
        if m and name:
            kernels[name][m.group(1).strip()] = int(m.group(2))

    def one(needle):
        hits = [r for n, r in kernels.items() if needle in n]
        assert len(hits) == 1, (needle, sorted(kernels))
        return hits[0]

    pairs = [(f"k_jpeg_fdct_roiILi{src}ELi{cs}EE", f"k_jpeg_fdctILi{src}ELi{cs}EE") for src in (1, 2, 3)
             for cs in (0, 1, 2)] + [("k_jpeg_fdct_roiILi0ELi0EE", "k_jpeg_fdctILi0ELi0EE")]
    pairs += [(f"k_jpeg_{k}_roiE", f"k_jpeg_{k}E") for k in ("hist", "huff", "offsets", "assemble")]
    for new, old in pairs:
        r, o = one(new), one(old)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (new, r)
        assert r["Occupancy"] >= o["Occupancy"], (new, r, o)
        assert r["LDS Size"] == o["LDS Size"], (new, r, o)
    assert not [n for n in kernels if re.search(r"k_jpeg_fdct_roiILi0ELi[12]EE", n)]
