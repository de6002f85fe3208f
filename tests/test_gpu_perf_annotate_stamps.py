"""Speed of MARK_STAMP on 16 x 1080p NV12 (tests/test_gpu_perf_annotate.py's geometry, tests/test_gpu_perf_roi.py's harness:
one process, alternating three times, the minimum of each side):

1. 512 stamps of label size (40 .. 160 x 12 .. 24) against the chain they replace (measured: 25.5 us against 71.3 ms):
   per mark and plane
   view = (view * (255 - ae) + c * ae + 127) // 255 in torch, with `ae` precomputed per mark from slices of the atlas, the
   boxes already on the host and even positions and sizes, so that the chain's chroma weight is a plain 2 x 2 mean -- all
   of which favours the chain.  No slower than the chain; no further margin is taken: the chain cannot take fewer than
   one launch per mark and plane, the annotator issues two.  Both must have written the same bytes first.
2. an atlas in the call does not slow the other kinds: the mixed 512-mark set of the existing test (BOX, FILL, PIXELATE)
   with an atlas and no STAMP row -- k_annotate<NV12, true>, five waves per SIMD where k_annotate<NV12, false> has seven
   -- against the same call without an atlas, which runs the instantiation that stamps did not change.
   Measured on an MI355X: 63.7 us with an atlas against 53.0 us without, ratio 1.20 (profiles/annotate_stamps.md).  The
   guard is 1.5: the measured ratio plus the margin this project gives the spread between machines (1.03 measured
   guards 1.3, 1.18 measured guards 1.5).
3. print only (-s): 512 and 4096 stamps, NV12 and RGB, with the bytes the stamps cover (read and written once each) over
   the time as a fraction of 8 TB/s."""
import numpy as np
import pytest

import annotate_model as am
import annotate_stamp_model as sm
import postproc_model as pm
from test_gpu_perf_annotate import H, N, PEAK, ROWS, W, _device, _frames, _marks
from test_gpu_perf_roi import _alternate, _timed

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

AW, AH = 256, 64
GUARD = 1.5         # an atlas in the call against none, on marks that are no stamps: measured 1.20


def _atlas(vali, gpu, seed=4):
    host = np.random.default_rng(seed).integers(0, 256, (AH, AW), dtype=np.uint8)
    t = torch.from_numpy(host).to(f"cuda:{gpu}")
    torch.cuda.synchronize()
    return host, t, vali.Surface.from_dlpack(t, vali.Y)


def _stamps(m, seed=3):
    """m rows, m / N per frame, label-sized, even positions and sizes, wholly inside the frame and the atlas"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(m):
        w, h = int(rng.integers(40, 161)) & ~1, int(rng.integers(12, 25)) & ~1
        x, y = int(rng.integers(0, W - w)) & ~1, int(rng.integers(0, H - h)) & ~1
        u, v = int(rng.integers(0, AW - w + 1)), int(rng.integers(0, AH - h + 1))
        rows.append((i % N, x, y, w, h, sm.STAMP, sm.pack_uv(u, v),
                     am.pack_colour(*(int(c) for c in rng.integers(0, 256, 3)), int(rng.integers(60, 256)))))
    return rows


def test_stamps_are_no_slower_than_the_chain_they_replace(vali, gpu):
    stream = torch.cuda.current_stream(gpu).cuda_stream         # torch's work and ours on one stream
    rows = _stamps(512)
    marks = _device(rows, gpu)
    _, atlas_t, atlas = _atlas(vali, gpu)
    bufs_a, surfs = _frames(vali, gpu)
    bufs_c = [b.clone() for b in bufs_a]
    ann = vali.PySurfaceAnnotator(gpu, stream)
    ab = ann.PrepareBatch(surfs)
    matrix = pm.matrices()[ROWS]
    ys = [b[:H] for b in bufs_c]
    uvs = [b[H:].view(H // 2, W // 2, 2) for b in bufs_c]
    cov = atlas_t.to(torch.int32)
    host = []
    for f, x, y, w, h, _, arg, c in rows:
        u, v = sm.unpack_uv(arg)
        a = am.unpack_colour(c)[3]
        k = cov[v:v + h, u:u + w]
        k2 = (k[0::2, 0::2] + k[0::2, 1::2] + k[1::2, 0::2] + k[1::2, 1::2] + 2) >> 2
        host.append((f, x, y, w, h, (k * a + 127) // 255, (k2 * a + 127) // 255, am.yuv_of(*am.unpack_colour(c)[:3], matrix)))
    torch.cuda.synchronize()

    def blend(view, c, ae):
        view.copy_(((view.to(torch.int32) * (255 - ae) + c * ae + 127) // 255).to(torch.uint8))

    def chain():
        for f, x, y, w, h, ae, ae2, yuv in host:
            x2, y2, w2, h2 = x // 2, y // 2, w // 2, h // 2
            blend(ys[f][y:y + h, x:x + w], yuv[0], ae)
            blend(uvs[f][y2:y2 + h2, x2:x2 + w2, 0], yuv[1], ae2)
            blend(uvs[f][y2:y2 + h2, x2:x2 + w2, 1], yuv[2], ae2)

    # the two write the same bytes
    assert ann.RunBatchAsync(ab, marks, atlas=atlas)[0]
    chain()
    torch.cuda.synchronize()
    for a, c in zip(bufs_a, bufs_c):
        assert torch.equal(a, c)
    t_ann, t_chain = _alternate(gpu, stream, lambda: ann.RunBatchAsync(ab, marks, atlas=atlas), chain)
    torch.cuda.synchronize()
    print(f"\nannotate 16 x 1080p NV12, {len(rows)} stamps: {t_ann * 1e3:.1f} us, torch chain {t_chain * 1e3:.1f} us, "
          f"ratio {t_ann / t_chain:.4f}")
    assert t_ann <= t_chain, f"annotator {t_ann * 1e3:.1f} us vs chain {t_chain * 1e3:.1f} us"


def test_an_atlas_in_the_call_does_not_slow_the_other_kinds(vali, gpu):
    ann = vali.PySurfaceAnnotator(gpu)
    rows = _marks(512, (am.BOX, am.FILL, am.PIXELATE))
    marks = _device(rows, gpu)
    _, _, atlas = _atlas(vali, gpu)
    bufs, surfs = _frames(vali, gpu)
    ab = ann.PrepareBatch(surfs)
    t_with, t_without = _alternate(gpu, ann.Stream, lambda: ann.RunBatchAsync(ab, marks, atlas=atlas),
                                   lambda: ann.RunBatchAsync(ab, marks))
    print(f"\nannotate 16 x 1080p NV12, 512 mixed marks: with an atlas {t_with * 1e3:.1f} us, without {t_without * 1e3:.1f} us, "
          f"ratio {t_with / t_without:.4f}")
    assert t_with <= GUARD * t_without, f"with an atlas {t_with * 1e3:.1f} us vs without {t_without * 1e3:.1f} us"


def test_print_stamp_rates(vali, gpu):
    """no assertion on speed: the table of profiles/annotate_stamps.md (run with -s)"""
    ann = vali.PySurfaceAnnotator(gpu)
    _, _, atlas = _atlas(vali, gpu)
    print()
    for fmt in ("NV12", "RGB"):
        bufs, surfs = _frames(vali, gpu, fmt)
        ab = ann.PrepareBatch(surfs)
        for m in (512, 4096):
            rows = _stamps(m)
            marks = _device(rows, gpu)
            ms = _timed(gpu, ann.Stream, lambda: ann.RunBatchAsync(ab, marks, atlas=atlas))
            cov = sum(2 * (1.5 if fmt == "NV12" else 3.0) * r[3] * r[4] for r in rows)
            print(f"{fmt:5s} {m:4d} stamps {ms * 1e3:8.1f} us  {cov / 1e6:8.1f} MB covered  {cov / (ms * 1e-3) / PEAK:.3f} of 8 TB/s")
            assert ms > 0
        del ab, surfs, bufs
