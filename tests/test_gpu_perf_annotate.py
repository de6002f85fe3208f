"""Speed of PySurfaceAnnotator on 16 x 1080p NV12 with 512 marks (32 per frame, boxes of 40 .. 400 pixels a side: outlines
of thickness 4, translucent fills, pixelation with cells of 16), against two things that are not the code under test (in
one process, alternating three times, the minimum of each side; tests/test_gpu_perf_roi.py's harness):

1. the chain it replaces: torch slice assignments on DLPack views of the Y and UV planes for the outline and fill marks
   of the set (pixelate marks are left out of BOTH sides), with the boxes already on the host, which favours the chain.
   No slower than the chain; no further margin is taken: the chain cannot take fewer than one launch per mark and plane,
   the annotator issues two.  Both must have written the same bytes first.
2. untouched frames cost no pixel traffic: the same call with all 512 rows of kind 0 against
   PySurfacePostprocessor.RunTensorBatchAsync writing the same 16 frames from a uint8 tensor, which moves every pixel.
3. print only (-s): the mixed set, 512 pixelate marks and 4096 marks, NV12 and RGB, with the bytes the marks cover (read
   and written once each) over the time as a fraction of 8 TB/s."""
import numpy as np
import pytest

import annotate_model as am
import postproc_model as pm
from test_gpu_perf_roi import _alternate, _timed

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

N, W, H = 16, 1920, 1080
PEAK = 8e12
ROWS = "601_JPEG"


def _marks(m, kinds, seed=3):
    """m rows, m / N per frame, even coordinates, wholly inside the frame"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(m):
        w, h = (int(v) & ~1 for v in rng.integers(40, 401, 2))
        x, y = int(rng.integers(0, W - w)) & ~1, int(rng.integers(0, H - h)) & ~1
        kind = kinds[i % len(kinds)]
        arg, a = {am.BOX: (4, 255), am.FILL: (0, int(rng.integers(60, 200))), am.PIXELATE: (16, 255)}[kind]
        rows.append((i % N, x, y, w, h, kind, arg, am.pack_colour(*(int(v) for v in rng.integers(0, 256, 3)), a)))
    return rows


def _frames(vali, gpu, fmt="NV12", seed=2):
    """N frames as torch tensors (so the chain can write them) and as surfaces that view them"""
    g = torch.Generator(device=f"cuda:{gpu}").manual_seed(seed)
    rows, cols = am.plane_shapes(fmt, W, H)[0]
    bufs = [torch.randint(0, 256, (rows, cols), dtype=torch.uint8, device=f"cuda:{gpu}", generator=g) for _ in range(N)]
    torch.cuda.synchronize()
    return bufs, [vali.Surface.from_dlpack(b, getattr(vali, fmt)) for b in bufs]


def _device(rows, gpu):
    t = torch.tensor(np.asarray(rows, np.int64).astype(np.int32), dtype=torch.int32, device=f"cuda:{gpu}")
    torch.cuda.synchronize()
    return t


def _covered(rows, fmt):
    """bytes the marks cover, read once and written once"""
    per_px = 1.5 if fmt == "NV12" else 3.0
    total = 0.0
    for _, _, _, w, h, kind, arg, _ in rows:
        area = w * h if kind != am.BOX else w * h - max(w - 2 * arg, 0) * max(h - 2 * arg, 0)
        total += 2 * per_px * area
    return total


def test_no_slower_than_the_chain_it_replaces(vali, gpu):
    stream = torch.cuda.current_stream(gpu).cuda_stream         # torch's work and ours on one stream
    rows = [r for r in _marks(512, (am.BOX, am.FILL, am.PIXELATE)) if r[5] != am.PIXELATE]
    marks = _device(rows, gpu)
    bufs_a, surfs = _frames(vali, gpu)
    bufs_c = [b.clone() for b in bufs_a]
    ann = vali.PySurfaceAnnotator(gpu, stream)
    ab = ann.PrepareBatch(surfs)
    matrix = pm.matrices()[ROWS]
    host = [(f, x, y, w, h, kind, t, am.unpack_colour(c)[3], am.yuv_of(*am.unpack_colour(c)[:3], matrix))
            for f, x, y, w, h, kind, t, c in rows]
    ys = [b[:H] for b in bufs_c]
    uvs = [b[H:].view(H // 2, W // 2, 2) for b in bufs_c]
    uv_cols = {yuv: torch.tensor(yuv[1:], dtype=torch.uint8, device=f"cuda:{gpu}") for *_, yuv in host}

    def blend(view, c, a):
        view.copy_(((view.to(torch.int32) * (255 - a) + c * a + 127) // 255).to(torch.uint8))

    def chain():
        for f, x, y, w, h, kind, t, a, yuv in host:
            Y, UV = ys[f], uvs[f]
            x2, y2, w2, h2, t2 = x // 2, y // 2, w // 2, h // 2, t // 2
            if kind == am.FILL:
                blend(Y[y:y + h, x:x + w], yuv[0], a)
                blend(UV[y2:y2 + h2, x2:x2 + w2, 0], yuv[1], a)
                blend(UV[y2:y2 + h2, x2:x2 + w2, 1], yuv[2], a)
            else:       # opaque outline: four slice assignments per plane
                Y[y:y + t, x:x + w] = yuv[0]
                Y[y + h - t:y + h, x:x + w] = yuv[0]
                Y[y:y + h, x:x + t] = yuv[0]
                Y[y:y + h, x + w - t:x + w] = yuv[0]
                c = uv_cols[yuv]
                UV[y2:y2 + t2, x2:x2 + w2] = c
                UV[y2 + h2 - t2:y2 + h2, x2:x2 + w2] = c
                UV[y2:y2 + h2, x2:x2 + t2] = c
                UV[y2:y2 + h2, x2 + w2 - t2:x2 + w2] = c

    # the two write the same bytes
    assert ann.RunBatchAsync(ab, marks)[0]
    chain()
    torch.cuda.synchronize()
    for a, c in zip(bufs_a, bufs_c):
        assert torch.equal(a, c)
    t_ann, t_chain = _alternate(gpu, stream, lambda: ann.RunBatchAsync(ab, marks), chain)
    torch.cuda.synchronize()
    print(f"\nannotate 16 x 1080p NV12, {len(rows)} outline and fill marks: {t_ann * 1e3:.1f} us, torch chain "
          f"{t_chain * 1e3:.1f} us, ratio {t_ann / t_chain:.4f}")
    assert t_ann <= t_chain, f"annotator {t_ann * 1e3:.1f} us vs chain {t_chain * 1e3:.1f} us"


def test_untouched_frames_cost_no_pixel_traffic(vali, gpu):
    post = vali.PySurfacePostprocessor(gpu)
    stream = post.Stream
    ann = vali.PySurfaceAnnotator(gpu, stream)
    rows = [(f, x, y, w, h, am.NONE, arg, c) for f, x, y, w, h, _, arg, c in _marks(512, (am.BOX, am.FILL, am.PIXELATE))]
    marks = _device(rows, gpu)
    bufs, surfs = _frames(vali, gpu)
    before = [b.clone() for b in bufs]
    ab = ann.PrepareBatch(surfs)
    t = torch.randint(0, 256, (N, 3, H, W), dtype=torch.uint8, device=f"cuda:{gpu}")
    outs = [vali.Surface.Make(vali.NV12, W, H, gpu) for _ in range(N)]
    torch.cuda.synchronize()
    fb = post.PrepareTensorBatch(t, outs)
    t_skip, t_post = _alternate(gpu, stream, lambda: ann.RunBatchAsync(ab, marks), lambda: post.RunTensorBatchAsync(fb))
    torch.cuda.synchronize()
    for a, b in zip(bufs, before):
        assert torch.equal(a, b)
    print(f"\nannotate 16 x 1080p NV12, 512 rows of kind 0: {t_skip * 1e3:.1f} us; postprocessor writing the same frames "
          f"{t_post * 1e3:.1f} us; ratio {t_skip / t_post:.3f}")
    assert t_skip <= t_post, f"skipping {t_skip * 1e3:.1f} us vs postprocessor {t_post * 1e3:.1f} us"


def test_print_every_form(vali, gpu):
    """no assertion on speed: the table of profiles/annotate.md (run with -s)"""
    ann = vali.PySurfaceAnnotator(gpu)
    sets = {"mixed 512": _marks(512, (am.BOX, am.FILL, am.PIXELATE)), "pixelate 512": _marks(512, (am.PIXELATE,)),
            "mixed 4096": _marks(4096, (am.BOX, am.FILL, am.PIXELATE))}
    print()
    for fmt in ("NV12", "RGB"):
        bufs, surfs = _frames(vali, gpu, fmt)
        ab = ann.PrepareBatch(surfs)
        for name, rows in sets.items():
            marks = _device(rows, gpu)
            ms = _timed(gpu, ann.Stream, lambda: ann.RunBatchAsync(ab, marks))
            cov = _covered(rows, fmt)
            print(f"{fmt:5s} {name:13s} {ms * 1e3:8.1f} us  {cov / 1e6:8.1f} MB covered  {cov / (ms * 1e-3) / PEAK:.3f} of 8 TB/s")
            assert ms > 0
        del ab, surfs, bufs
