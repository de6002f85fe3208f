"""Semantic maps without a GPU: the numpy model (tests/semantic_model.py) against independent statements -- the mask
model's sampler, the stamp model, torch's interpolate + argmax --, ties and non-finite values, the conditions the shared
fixtures (tests/semantic_cases.py) must hold, the Python checks, and what the C entry point refuses before any device is
touched."""
import numpy as np
import pytest

import annotate_model as am
import annotate_stamp_model as asm
import mask_model as mm
import postproc_model as pm
import semantic_cases as sc
import semantic_model as sm

ROWS_601 = "601_JPEG"


# ---- the model against the mask model's sampler --------------------------------------------------------------------------
@pytest.mark.parametrize("ws,hs", sc.LOGIT_SIZES)
def test_the_values_are_the_mask_samplers_on_every_plane(ws, hs):
    logits = sc.logits(5, ws, hs)
    for i, size in enumerate(sc.SIZES):
        box = sm.region(sc.RECTS[i], size)
        v = sm.values(logits[i], box, sc.RECTS[i], sc.NET)
        for c in range(5):
            want, _ = mm.sample(logits[i, c], box, sc.RECTS[i], sc.NET)
            assert np.array_equal(v[c], want), (i, c)
    assert sm.region(sc.RECTS[1], sc.SIZES[1]) == (10, 6, 28, 21)            # a non-zero, non-even origin


# ---- the model's frames against the stamp model -------------------------------------------------------------------------------
def four_class_blocks(n, c, hs, ws):
    """logits whose arg-max changes with every cell: with the identity placement every 2 x 2 block of a frame of the
    logits' size holds four different classes"""
    out = np.full((n, c, hs, ws), -4.0, np.float32)
    y, x = np.mgrid[0:hs, 0:ws]
    for k in range(c):
        out[:, k][:, (2 * (y % 2) + x % 2 + 4 * ((x // 2 + y // 2) % 2)) % c == k] = 4.0
    return out


@pytest.mark.parametrize("fmt", am.FORMATS)
def test_painting_is_stamping_one_mask_per_class_from_an_atlas(fmt):
    rows = pm.matrices()[ROWS_601]
    cases = [(sc.logits(19, 24, 20), sc.RECTS, sc.SIZES, sc.NET, sc.palette(7), 128),
             (sc.logits(3, 16, 16), sc.RECTS, sc.SIZES, sc.NET, sc.PALETTE_OWN_ALPHA, None),
             # the identity placement on frames of the logits' size: single pixels of four classes in every chroma block
             (four_class_blocks(2, 8, 50, 70), [(0, 0, 70, 50, 0, 0, 70, 50), (1, 1, 67, 47, 1, 1, 67, 47)],
              [(70, 50), (70, 50)], (70, 50), sc.palette(8), 255)]
    for logits, rects, sizes, net, colours, alpha in cases:
        a = [am.noise_frame(fmt, w, h, 7100 + i) for i, (w, h) in enumerate(sizes)]
        b = [f.copy() for f in a]
        before = [f.copy() for f in a]
        maps = sm.apply(a, fmt, sizes, logits, rects, colours, alpha, net, rows)
        atlas, marks = sm.stamp_atlas(maps, colours, alpha)
        assert asm.apply(b, fmt, sizes, marks, rows, atlas) == list(range(len(marks)))
        assert [m[5] for m in marks] == [asm.STAMP] * len(marks)
        for i in range(len(sizes)):
            assert np.array_equal(a[i], b[i]), (fmt, alpha, i)
            assert not np.array_equal(a[i], before[i])
    # the last case: a chroma block with four different classes, and a region with odd bounds on both frames
    m = maps[0]
    four = [len({int(m[y, x]), int(m[y, x + 1]), int(m[y + 1, x]), int(m[y + 1, x + 1])}) for y in range(0, 50, 2)
            for x in range(0, 70, 2)]
    assert min(four) == 4
    assert (maps[1][0] == 255).all() and (maps[1][:, 0] == 255).all() and (maps[1][1:48, 1:68] != 255).all()


# ---- the model against torch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("frame,size,c", [((96, 80), (16, 16), 19), ((70, 50), (24, 20), 5), ((70, 50), (160, 120), 19),
                                          ((96, 80), (24, 20), 255)])
def test_the_labels_are_torchs_interpolate_and_argmax_away_from_ties(frame, size, c, dtype):
    torch = pytest.importorskip("torch")
    F = torch.nn.functional
    W, H = frame
    logits = sc.logits(c, size[0], size[1], dtype, n=1, seed=3)
    up = F.interpolate(torch.from_numpy(logits), (H, W), mode="bilinear", align_corners=False)
    top = up.topk(2, dim=1).values[0]
    clear = ((top[0] - top[1]) > 1e-3).numpy()
    share = clear.mean()
    print(f"{frame} {size} C={c} {dtype}: share above the margin {share:.3f}")
    assert share >= 0.90                                       # a condition on the inputs
    net = (4 * size[0], 4 * size[1])
    got = sm.label_map(logits[0], frame, (0, 0, W, H, 0, 0, net[0], net[1]), net)
    want = up.argmax(1)[0].numpy()
    wrong = (got != want) & clear
    print(f"  disagreements above the margin: {int(wrong.sum())}, below: {int(((got != want) & ~clear).sum())}")
    assert not wrong.any()


# ---- ties and non-finite values -----------------------------------------------------------------------------------------------
def labels_of(planes, frame=(12, 10)):
    planes = np.asarray(planes, np.float32)
    return sm.label_map(planes, frame, (0, 0, frame[0], frame[1], 0, 0, 32, 32), (32, 32))


def test_ties_and_non_finite_values():
    rng = np.random.default_rng(5)
    plane = rng.standard_normal((6, 7)).astype(np.float32)
    low = np.full((6, 7), -9.0, np.float32)
    nan, pinf, ninf = (np.full((6, 7), v, np.float32) for v in (np.nan, np.inf, -np.inf))
    assert (labels_of([low, plane, plane]) == 1).all()                       # identical planes: the lower wins
    assert (labels_of([plane, plane, plane]) == 0).all()                     # all equal
    assert (labels_of([nan, low, plane]) == 2).all()                         # a NaN never wins
    # an infinite plane interpolates to inf - inf = NaN, as the mask sampler does: it never wins either
    assert (labels_of([plane, pinf, nan]) == 0).all() and (labels_of([ninf, plane, ninf]) == 1).all()
    assert (labels_of([nan, nan, nan]) == 0).all() and (labels_of([ninf, ninf]) == 0).all()
    assert (labels_of([ninf, nan, ninf, nan]) == 0).all()
    # +inf in one column of cells: NaN wherever a tap touches it, so the finite class has those pixels
    mixed = plane.copy()
    mixed[:, 3] = np.inf
    got = labels_of([low, mixed])
    assert (got == 1).any() and (got == 0).any() and (got[:, :2] == 1).all()
    # C = 1: the sign; 0.0, -0.0 and NaN are class 0
    for v, want in ((0.0, 0), (-0.0, 0), (np.nan, 0), (1e-30, 1), (-1.0, 0), (np.inf, 0)):      # (inf - inf = NaN)
        assert (labels_of([np.full((6, 7), v, np.float32)]) == want).all(), v
    assert set(np.unique(labels_of([plane])).tolist()) == {0, 1}


def test_skipped_records_and_extreme_records():
    logits = sc.logits(5, 16, 16)
    maps = [sm.label_map(logits[i], sc.SIZES[i], sc.RECTS_DST_W_0[i], sc.NET) for i in range(2)]
    assert (maps[0] != 255).all() and (maps[1] == 255).all()
    assert sm.region(sc.EXTREME_RECTS[0], sc.SIZES[0]) == (0, 3, 44, 80)
    assert sm.region(sc.EXTREME_RECTS[1], sc.SIZES[1]) == (8, 0, 70, 39)
    assert all(sm.region(r, s) is None for r, s in zip(sc.EXTREME_RECTS_MISS, sc.SIZES))
    for bad in [(0, 0, 0, 5, 0, 0, 5, 5), (0, 0, 5, -1, 0, 0, 5, 5), (0, 0, 5, 5, 0, 0, 0, 5), (0, 0, 5, 5, 0, 0, 5, sc.I32_MIN)]:
        assert sm.region(bad, (96, 80)) is None


# ---- conditions on the fixtures -----------------------------------------------------------------------------------------------
def test_the_fixtures_take_the_paths_their_names_say():
    def paths(size):
        return [sm.tile_paths(s, r, size[1], size[0], sc.NET) for s, r in zip(sc.SIZES, sc.RECTS)]

    for size in sc.LOGIT_SIZES[:2]:
        assert all(set(p.values()) == {"staged"} for p in paths(size))
    p = paths((160, 120))
    assert set(p[0].values()) == {"staged"} and len(p[0]) == 6     # 96 x 80: 2 x 2 tiles, the lower two of one pass (rows 64 .. 79)
    assert p[1] == {(0, 0, 0): "direct"}                                           # 70 x 50: the region is in one pass
    assert paths(sc.SWITCH_SIZES[0])[1] == {(0, 0, 0): "staged"} and paths(sc.SWITCH_SIZES[1])[1] == {(0, 0, 0): "direct"}
    # the cells of that pass either side of the stage
    cells = []
    for ws, hs in sc.SWITCH_SIZES:
        i0, i1, _ = mm.taps(np.array([10, 27]), 10, 18, 2, 60, ws, 64)
        j0, j1, _ = mm.taps(np.array([6, 20]), 6, 15, 3, 50, hs, 64)
        cells.append((int(j1[1] - j0[0]) + 1) * ((int(i1[1] - i0[0]) + 1) | 1))
    assert cells == [8175, 8325] and cells[0] <= sm.STAGE_CELLS < cells[1]


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_the_fixtures_show_several_classes_on_every_frame(dtype):
    for (ws, hs) in sc.LOGIT_SIZES:
        logits = sc.logits(19, ws, hs, dtype)
        for i, size in enumerate(sc.SIZES):
            m = sm.label_map(logits[i], size, sc.RECTS[i], sc.NET)
            assert len(set(np.unique(m).tolist()) - {255}) >= 3, (ws, hs, i)
    nf = sc.nonfinite_logits(6, 24, 20, dtype)
    assert np.isnan(nf[0, 1]).all() and np.isneginf(nf[0, 5]).all() and np.isposinf(nf[0, 2]).any()
    assert np.isnan(nf[1]).any() and np.isinf(nf[1]).any()


# ---- the Python checks -------------------------------------------------------------------------------------------------------------
F32, F16, BF16 = (2, 32), (2, 16), (4, 16)


def test_layouts_say_what_is_wrong(vali):
    from vali_amd.semantic import logits_layout, paint_spec, semantic_spec

    good = logits_layout((2, 19, 128, 128), None, *F16)
    assert good == (1, (2, 19, 128, 128), (19 * 128 * 128, 128 * 128, 128, 1))
    # a (1, C, Hs, Ws) tensor expanded over N, a slice of a larger head with a row pitch
    assert logits_layout((16, 19, 128, 128), (0, 130 * 136, 136, 1), *BF16)[2] == (0, 130 * 136, 136, 1)
    for shape in [(1, 1, 1, 1), (1024, 255, 4096, 4096)]:                      # every limit at its edge
        assert logits_layout(shape, None, *F32)[1] == shape
    assert logits_layout((2, 3, 4, 1), (12, 4, 1, 7), *F32)[2] == (12, 4, 1, 7)          # Ws = 1: any x stride
    for args, text in [(((2, 19, 128), None, *F32), "4-D"), (((2, 19, 128, 128), None, 0, 32), "dtype"),
                       (((2, 19, 128, 128), None, 2, 64), "dtype"),
                       (((0, 19, 128, 128), None, *F32), "N = 0 is outside 1..1024"),
                       (((1025, 1, 1, 1), None, *F32), "N = 1025 is outside 1..1024"),
                       (((2, 0, 128, 128), None, *F32), "C = 0 is outside 1..255"),
                       (((2, 256, 128, 128), None, *F32), "C = 256 is outside 1..255"),
                       (((2, 19, 4097, 128), None, *F32), "Hs x Ws = 4097 x 128 is outside 1..4096"),
                       (((2, 19, 128, 4097), None, *F32), "Hs x Ws = 128 x 4097 is outside 1..4096"),
                       (((2, 19, 0, 128), None, *F32), "Hs x Ws"), (((2, 19, 128, 0), None, *F32), "Hs x Ws"),
                       (((2, 19, 128, 128), (1, 2, 3, 2), *F32), "the x stride must be 1, got 2"),
                       (((2, 19, 128, 128), (1, 2, -3, 1), *F32), "negative strides"),
                       (((2, 19, 128, 128), (2**40 + 1, 2, 3, 1), *F32), "beyond 2.40")]:
        with pytest.raises(ValueError, match=text):
            logits_layout(*args)
    assert logits_layout((2, 19, 128, 128), (2**40, 0, 0, 1), *F32)[2] == (2**40, 0, 0, 1)

    sizes = [(96, 80), (70, 50)]
    assert semantic_spec(sizes, good) == (2, 19, 128, 128, 512, 512)
    assert semantic_spec(sizes, good, None, (1, 65535)) == (2, 19, 128, 128, 1, 65535)
    ok_labels = [(vali.Y, 96, 80), (vali.Y, 70, 50)]
    assert semantic_spec(sizes, good, ok_labels, (64, 64))[4:] == (64, 64)
    for kw, text in [(dict(frame_sizes=sizes + sizes[:1]), "3 surfaces for logits of N = 2"),
                     (dict(net_size=(0, 64)), "net_size"), (dict(net_size=(64, 65536)), "net_size"),
                     (dict(net_size=64), "net_size"), (dict(label_views=ok_labels[:1]), "labels: 1 surfaces for 2 frames"),
                     (dict(label_views=[ok_labels[0], (vali.Y, 70, 52)]), "labels: surface 1 is 70x52, its frame 70x50"),
                     (dict(label_views=[ok_labels[0], (vali.NV12, 70, 50)]), "labels: surface 1 has format .*need Y")]:
        a = dict(frame_sizes=sizes, logits_view=good, label_views=None, net_size=(64, 64))
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            semantic_spec(**a)

    assert paint_spec([1, -2], 128, False) == ([1, -2], 128) and paint_spec((7,), None, True) == ([7], -1)
    assert paint_spec(None, 128, True) == (None, 128)
    for args, text in [(([], 128, True), "at least one"), (([1], 256, True), "alpha"), (([1], -1, True), "alpha"),
                       (([2**31], 0, True), "int32"), ((5, 0, True), "colours"),
                       ((None, 128, False), "colours=None paints nothing and only writes labels")]:
        with pytest.raises(ValueError, match=text):
            paint_spec(*args)


def test_the_names_are_exported():
    import python_vali
    import vali_amd

    for name in ("PySemanticPainter", "SemanticBatch"):
        assert getattr(python_vali, name) is getattr(vali_amd, name)


# ---- the C entry point without a device ----------------------------------------------------------------------------------------------
def test_the_entry_point_refuses_before_any_device_is_touched(vali):
    """the pointers below are dummies that are never read"""
    from vali_amd._native import shim

    def call(fmt="NV12", sizes=((64, 48), (2, 2)), descs=None, d_frames=0x1000, logits=(0x2000, 1, 100, 10, 16), c=5, hs=16,
             ws=16, net=(64, 64), rects=0x5000, labels=True, label_sizes=None, label_fmt="Y", d_labels=0x8000, colours=0x6000,
             nc=3, alpha=128, params=True, plane=0x7000, pitch=None, label_plane=0x9000, label_pitch=None):
        f = int(getattr(vali, fmt)) if isinstance(fmt, str) else fmt
        if descs is None:
            descs = [shim.SurfaceDesc([plane] * 3, [pitch or 3 * w] * 3, w, h, f) for w, h in sizes]
        lab = []
        if labels:
            lab = [shim.SurfaceDesc([label_plane, 0, 0], [label_pitch or w, 0, 0], w, h, int(getattr(vali, label_fmt)))
                   for w, h in (label_sizes or sizes)]
        prm = shim.CvtParams(None, [[0.25, 0.5, 0.25, 0.0]] * 3) if params else None
        rc = shim.semantic_paint(descs, d_frames, f, logits, c, hs, ws, net[0], net[1], rects, lab, d_labels, colours, nc,
                                 alpha, prm, 0)
        return rc, shim.last_error()

    cases = [
        (dict(d_frames=0), "null argument"), (dict(rects=0), "null argument"), (dict(descs=[], labels=False, d_labels=0),
                                                                                "null argument"),
        (dict(d_labels=0), "both or neither"), (dict(labels=False), "both or neither"),
        (dict(labels=False, d_labels=0, colours=0), "neither labels nor colours"),
        (dict(sizes=[(2, 2)] * 1025), "n outside"), (dict(c=0), "c outside 1..255"), (dict(c=256), "c outside 1..255"),
        (dict(hs=0), "hs or ws"), (dict(ws=4097), "hs or ws"), (dict(hs=4097), "hs or ws"),
        (dict(net=(0, 64)), "net_w or net_h"), (dict(net=(64, 65536)), "net_w or net_h"),
        (dict(logits=(0, 1, 100, 10, 16)), "logits has a null pointer"), (dict(logits=(0x2000, 3, 100, 10, 16)), "dtype 3"),
        (dict(logits=(0x2000, -1, 100, 10, 16)), "dtype -1"), (dict(logits=(0x2001, 1, 100, 10, 16)), "not aligned to its element"),
        (dict(logits=(0x2002, 0, 100, 10, 16)), "not aligned to its element"), (dict(logits=(0x2000, 1, -1, 10, 16)), "strides"),
        (dict(logits=(0x2000, 1, 1, 2**40 + 1, 16)), "strides"), (dict(logits=(0x2000, 1, 1, 1, -5)), "strides"),
        (dict(nc=0), "n_colours below 1"), (dict(alpha=256), "alpha outside"), (dict(alpha=-2), "alpha outside"),
        (dict(rects=0x5001), "not 4-byte aligned"), (dict(colours=0x6002), "not 4-byte aligned"),
        (dict(sizes=((64, 48), (3, 2))), "even width and height"), (dict(sizes=((64, 48), (0, 2))), "outside 1..65535"),
        (dict(sizes=((64, 48), (65536, 2)), fmt="RGB"), "outside 1..65535"), (dict(plane=0), "plane 0 is null"),
        (dict(pitch=63), "shorter than a row"), (dict(params=False), "needs params"),
        (dict(label_fmt="NV12"), "label surface 0 has format"), (dict(label_sizes=((64, 48), (2, 4))), "label surface 1 is 2x4"),
        (dict(label_plane=0), "label surface 0: plane 0 is null"), (dict(label_pitch=1), "label surface 0: pitch 1 is shorter"),
    ]
    for kw, text in cases:
        rc, err = call(**kw)
        assert rc == shim.ERR_INVALID_ARG and text in err and "vali_semantic_paint" in err, (kw, rc, err)
    mixed = [shim.SurfaceDesc([0x7000] * 3, [192] * 3, 64, 48, int(vali.NV12)),
             shim.SurfaceDesc([0x7000] * 3, [192] * 3, 64, 48, int(vali.YUV420))]
    rc, err = call(descs=mixed, sizes=((64, 48), (64, 48)))
    assert rc == shim.ERR_INVALID_ARG and "one format per batch" in err
    rc, err = call(fmt=int(vali.Y))
    assert rc == shim.ERR_UNSUPPORTED and "format" in err
    with pytest.raises(ValueError, match="as many label descriptors"):
        call(label_sizes=((64, 48),))
