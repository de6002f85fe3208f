"""Instance masks without a GPU: the numpy model (tests/mask_model.py) against an independent float64 restatement and
against the stamp model, the conditions the shared fixtures (tests/mask_cases.py) must hold, the Python checks, and what
the C entry point refuses before any device is touched."""
import numpy as np
import pytest

import annotate_model as am
import annotate_stamp_model as sm
import mask_cases as mc
import mask_model as mm
import postproc_model as pm

ROWS_601 = "601_JPEG"


# ---- the model against float64 ------------------------------------------------------------------------------------------
def mask64(row, i, size, protos, coeffs, rect, net_size):
    """steps 2 to 4 in float64, pixel by pixel, written apart from the model: (v over the clipped box, logit range)"""
    frame, x, y, w, h, _, _, k = (int(v) for v in row)
    W, H = size
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)
    L = np.tensordot(coeffs[i, k].astype(np.float64), protos[i].astype(np.float64), axes=1)
    hp, wp = L.shape
    sx, sy, sw, sh, dx, dy, dw, dh = rect
    v = np.zeros((y1 - y0, x1 - x0))
    for py in range(y0, y1):
        fy = ((py + 0.5 - sy) * (dh / sh) + dy) * (hp / net_size[1]) - 0.5
        j = int(np.floor(fy))
        ty = fy - j
        j0, j1 = min(max(j, 0), hp - 1), min(max(j + 1, 0), hp - 1)
        for px in range(x0, x1):
            fx = ((px + 0.5 - sx) * (dw / sw) + dx) * (wp / net_size[0]) - 0.5
            c = int(np.floor(fx))
            tx = fx - c
            c0, c1 = min(max(c, 0), wp - 1), min(max(c + 1, 0), wp - 1)
            top = L[j0, c0] + tx * (L[j0, c1] - L[j0, c0])
            bot = L[j1, c0] + tx * (L[j1, c1] - L[j1, c0])
            v[py - y0, px - x0] = top + ty * (bot - top)
    return v, float(L.max() - L.min())


@pytest.mark.parametrize("wp,hp", mc.PROTO_SIZES)
@pytest.mark.parametrize("m", [1, 5, 32])
def test_the_model_equals_float64_away_from_the_threshold(m, wp, hp):
    protos, coeffs = mc.protos(m, wp, hp), mc.coeffs(m)
    checked = 0
    for idx, row in enumerate(mc.PLACEMENTS):
        i = idx // mc.D
        box, inside = mm.row_mask(row, i, mc.SIZES[i], protos, coeffs, mc.RECTS[i], mc.NET)
        v, span = mask64(row, i, mc.SIZES[i], protos, coeffs, mc.RECTS[i], mc.NET)
        assert v.shape == inside.shape
        differ = inside != (v > 0)
        assert (np.abs(v[differ]) < 1e-4 * span).all(), (idx, np.abs(v[differ]).max() / span)
        checked += inside.size
    assert checked > 20000


# ---- conditions on the fixtures ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("wp,hp", mc.PROTO_SIZES)
@pytest.mark.parametrize("m", mc.MS)
def test_every_fixture_mask_covers_5_to_95_percent_of_its_box(m, wp, hp, dtype):
    """an all-empty or all-full mask would hide a wrong sampler"""
    protos, coeffs = mc.protos(m, wp, hp, dtype), mc.coeffs(m, dtype)
    for rows, painted in ((mc.PLACEMENTS, set(range(8))), (mc.SKIPS, mc.SKIPS_PAINTED)):
        for idx, row in enumerate(rows):
            i = idx // mc.D
            got = mm.row_mask(row, i, mc.SIZES[i], protos, coeffs, mc.RECTS[i], mc.NET)
            assert (got is not None) == (idx in painted), (idx, row)
            if got is not None:
                share = got[1].mean()
                assert 0.05 <= share <= 0.95, (idx, row, share)


def test_the_quantised_fixtures_are_exact_in_their_dtype():
    torch = pytest.importorskip("torch")
    a = mc.protos(5, 16, 16, "float32")
    for name, dt in (("float16", torch.float16), ("bfloat16", torch.bfloat16)):
        want = torch.from_numpy(a).to(dt).float().numpy()
        assert np.array_equal(mc.quantise(a, name), want), name


def test_the_fixtures_are_what_their_names_say():
    # frame 0: about 6 frame pixels a prototype pixel at 16 x 16; frame 1: more than one prototype pixel a frame pixel at 24 x 20
    i0, _, _ = mm.taps(np.arange(96), 0, 96, 0, 64, 16, 64)
    assert (np.bincount(i0)[1:-1] == 6).all()                 # (the first and last are clamped: edge replication)
    i0, _, _ = mm.taps(np.arange(70), 10, 18, 2, 60, 24, 64)
    inner = i0[(i0 > 0) & (i0 < 23)]
    assert (np.diff(inner) >= 1).all() and (np.diff(inner) == 2).any()
    assert any(r[1] & 1 and r[2] & 1 and r[3] & 1 and r[4] & 1 for r in mc.PLACEMENTS)           # odd everything
    for i, (w, h) in enumerate(mc.SIZES):                                                            # over every edge
        assert any(r[0] == i and r[1] < 0 and r[2] < 0 and r[1] + r[3] > w and r[2] + r[4] > h for r in mc.PLACEMENTS)
    c = mc.nonfinite_coeffs(5)
    assert np.isnan(c[:, 1]).any() and np.isposinf(c[:, 2]).any() and np.isneginf(c[:, 3]).any()


def test_non_finite_logits_are_never_in_the_mask_unless_the_definition_says_so():
    protos, coeffs = mc.protos(5, 16, 16), mc.nonfinite_coeffs(5)
    # candidate 1 has a NaN coefficient: every logit is NaN, nothing is in
    box, inside = mm.row_mask(mc.NONFINITE[1], 0, mc.SIZES[0], protos, coeffs, mc.RECTS[0], mc.NET)
    assert not inside.any()
    # candidate 2 has +inf: logits are +-inf; a pixel between two equal infinities takes inf - inf = NaN and is out
    box, inside = mm.row_mask(mc.NONFINITE[2], 0, mc.SIZES[0], protos, coeffs, mc.RECTS[0], mc.NET)
    assert not inside.all()


# ---- the model's frames against the stamp model ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", am.FORMATS)
def test_painting_is_stamping_the_masks_from_an_atlas(fmt):
    protos, coeffs = mc.protos(5, 24, 20), mc.coeffs(5)
    rows = pm.matrices()[ROWS_601]
    for dets, alpha in ((mc.PLACEMENTS, 128), (mc.SKIPS, None), (mc.PLACEMENTS, 255)):
        a, b = mc.noise_frames(fmt), mc.noise_frames(fmt)
        drawn = mm.apply(a, fmt, mc.SIZES, dets, mc.D, protos, coeffs, mc.RECTS, mc.COLOURS, alpha, mc.NET, rows)
        assert len(drawn) == (8 if dets is mc.PLACEMENTS else 2)
        atlas, marks = mm.stamp_atlas(drawn, dets)
        assert sm.apply(b, fmt, mc.SIZES, marks, rows, atlas) == list(range(len(marks)))
        for i in range(2):
            assert np.array_equal(a[i], b[i]), (fmt, alpha, i)
            assert not np.array_equal(a[i], mc.noise_frames(fmt)[i])


def test_the_order_of_overlapping_masks_is_visible():
    protos, coeffs = mc.protos(5, 16, 16), mc.coeffs(5)
    a, b = mc.noise_frames("RGB"), mc.noise_frames("RGB")
    swapped = list(mc.PLACEMENTS)
    swapped[0], swapped[1] = swapped[1], swapped[0]
    mm.apply(a, "RGB", mc.SIZES, mc.PLACEMENTS, mc.D, protos, coeffs, mc.RECTS, mc.COLOURS, 128, mc.NET)
    mm.apply(b, "RGB", mc.SIZES, swapped, mc.D, protos, coeffs, mc.RECTS, mc.COLOURS, 128, mc.NET)
    assert not np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_a_record_with_dst_w_0_paints_nothing_on_its_frame():
    protos, coeffs = mc.protos(5, 16, 16), mc.coeffs(5)
    a = mc.noise_frames("NV12")
    drawn = mm.apply(a, "NV12", mc.SIZES, mc.PLACEMENTS, mc.D, protos, coeffs, mc.RECTS_DST_W_0, mc.COLOURS, 128, mc.NET,
                     pm.matrices()[ROWS_601])
    assert [d[0] for d in drawn] == [0, 1, 2, 3] and np.array_equal(a[1], mc.noise_frames("NV12")[1])


def test_launch_1_range_covers_every_read():
    """the range from the box's first and last pixel (what k_mask_logits stores) holds every index the box's pixels read"""
    for (wp, hp) in mc.PROTO_SIZES:
        L = np.zeros((hp, wp), np.float32)
        for rows in (mc.PLACEMENTS, mc.SKIPS):
            for idx, row in enumerate(rows):
                i = idx // mc.D
                box = mm.resolve(row, i, mc.SIZES[i], mc.K, mc.RECTS[i])
                if box is None:
                    continue
                _, (c0, c1, r0, r1) = mm.sample(L, box, mc.RECTS[i], mc.NET)
                sx, sy, sw, sh, dx, dy, dw, dh = mc.RECTS[i]
                ends = np.array([box[0], box[2] - 1])
                a0, a1, _ = mm.taps(ends, sx, sw, dx, dw, wp, mc.NET[0])
                assert (a0[0], a1[1]) == (c0, c1)
                ends = np.array([box[1], box[3] - 1])
                a0, a1, _ = mm.taps(ends, sy, sh, dy, dh, hp, mc.NET[1])
                assert (a0[0], a1[1]) == (r0, r1)


# ---- the Python checks -------------------------------------------------------------------------------------------------------------
F32, F16, BF16 = (2, 32), (2, 16), (4, 16)


def test_layouts_say_what_is_wrong():
    from vali_amd.mask import coeffs_layout, mask_spec, paint_spec, protos_layout

    good_p = protos_layout((2, 32, 160, 160), None, *F16)
    assert good_p == (1, (2, 32, 160, 160), (32 * 160 * 160, 160 * 160, 160, 1))
    # a (1, M, Hp, Wp) tensor expanded over N, rows with a pitch; a YOLOv8-seg head (N, 4 + C + M, K) transposed
    assert protos_layout((16, 32, 160, 160), (0, 160 * 168, 168, 1), *BF16)[2][0] == 0
    good_c = coeffs_layout((2, 8400, 32), (116 * 8400, 1, 8400), *F32)
    assert good_c == (0, (2, 8400, 32), (116 * 8400, 1, 8400))
    for args, text in [(((2, 32, 160), None, *F32), "4-D"), (((2, 32, 160, 160), None, 0, 32), "dtype"),
                       (((0, 32, 160, 160), None, *F32), "N = 0"), (((1025, 1, 1, 1), None, *F32), "N = 1025"),
                       (((2, 65, 160, 160), None, *F32), "M = 65"), (((2, 0, 160, 160), None, *F32), "M = 0"),
                       (((2, 32, 1025, 160), None, *F32), "1025"), (((2, 32, 160, 0), None, *F32), "Hp x Wp"),
                       (((2, 32, 160, 160), (1, 2, 3, 2), *F32), "x stride"),
                       (((2, 32, 160, 160), (1, 2, -3, 1), *F32), "negative strides"),
                       (((2, 32, 160, 160), (2**41, 2, 3, 1), *F32), "beyond 2.40")]:
        with pytest.raises(ValueError, match=text):
            protos_layout(*args)
    for args, text in [(((2, 8400), None, *F32), "3-D"), (((2, 8400, 32), None, 1, 8), "dtype"),
                       (((2, 0, 32), None, *F32), "K = 0"), (((2, 2**20 + 1, 32), None, *F32), "K ="),
                       (((2, 8400, 65), None, *F32), "M = 65"), (((2, 8400, 32), (1, -1, 1), *F32), "negative")]:
        with pytest.raises(ValueError, match=text):
            coeffs_layout(*args)
    assert mask_spec(2, good_p, good_c, 100, (640, 640)) == (2, 32, 160, 160, 8400, 100, 640, 640)
    for kw, text in [(dict(n_frames=3), "3 surfaces"), (dict(max_det=0), "max_det = 0"), (dict(max_det=1025), "max_det = 1025"),
                     (dict(net_size=(0, 640)), "net_size"), (dict(net_size=(640, 65536)), "net_size"),
                     (dict(net_size=640), "net_size"), (dict(coeffs=coeffs_layout((2, 8400, 16), None, *F32)), "disagree"),
                     (dict(coeffs=coeffs_layout((3, 8400, 32), None, *F32)), "disagree")]:
        a = dict(n_frames=2, protos=good_p, coeffs=good_c, max_det=100, net_size=(640, 640))
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            mask_spec(a["n_frames"], a["protos"], a["coeffs"], a["max_det"], a["net_size"])
    big_p, big_c = protos_layout((1024, 1, 1, 1), None, *F32), coeffs_layout((1024, 1, 1), None, *F32)
    with pytest.raises(ValueError, match="exceeds 65535"):
        mask_spec(1024, big_p, big_c, 64, (640, 640))
    assert paint_spec([1, -2], 128) == ([1, -2], 128) and paint_spec((7,), None) == ([7], -1)
    for args, text in [(([], 128), "at least one"), (([1], 256), "alpha"), (([1], -1), "alpha"), (([2**31], 0), "int32"),
                       ((5, 0), "colours")]:
        with pytest.raises(ValueError, match=text):
            paint_spec(*args)


def test_the_names_are_exported():
    import python_vali
    import vali_amd

    for name in ("PyInstanceMasker", "MaskBatch"):
        assert getattr(python_vali, name) is getattr(vali_amd, name)


# ---- the C entry points without a device ---------------------------------------------------------------------------------------------
def test_workspace_size():
    from vali_amd._native import shim

    assert shim.mask_workspace_size(16, 100, 160, 160) == 16 * 100 * 160 * 160 * 4
    assert shim.mask_workspace_size(1, 1, 1, 1) == 4
    assert shim.mask_workspace_size(63, 1024, 1024, 1024) == 63 * 1024 * 2**20 * 4
    for bad in [(0, 1, 1, 1), (1025, 1, 1, 1), (1, 0, 1, 1), (1, 1025, 1, 1), (64, 1024, 1, 1), (1, 1, 0, 1), (1, 1, 1025, 1),
                (1, 1, 1, 0), (1, 1, 1, 1025)]:
        assert shim.mask_workspace_size(*bad) == 0, bad


def test_the_entry_point_refuses_before_any_device_is_touched(vali):
    """the pointers below are dummies that are never read"""
    from vali_amd._native import shim

    def call(fmt="NV12", sizes=((64, 48), (2, 2)), descs=None, d_frames=0x1000, protos=(0x2000, 1, 100, 10, 1),
             coeffs=(0x3000, 0, 100, 10, 1), m=5, hp=16, wp=16, k=12, D=4, net=(64, 64), dets=0x4000, rects=0x5000,
             colours=0x6000, nc=3, alpha=128, params=True, ws=0x10000, ws_bytes=None, plane=0x7000, pitch=None):
        f = int(getattr(vali, fmt)) if isinstance(fmt, str) else fmt
        if descs is None:
            descs = [shim.SurfaceDesc([plane] * 3, [pitch or 3 * w] * 3, w, h, f) for w, h in sizes]
        if ws_bytes is None:
            ws_bytes = len(descs) * D * hp * wp * 4
        prm = shim.CvtParams(None, [[0.25, 0.5, 0.25, 0.0]] * 3) if params else None
        rc = shim.mask_paint(descs, d_frames, f, protos, coeffs, m, hp, wp, k, D, net[0], net[1], dets, rects, colours, nc,
                             alpha, prm, ws, ws_bytes, 0)
        return rc, shim.last_error()

    cases = [
        (dict(d_frames=0), "null argument"), (dict(dets=0), "null argument"), (dict(rects=0), "null argument"),
        (dict(colours=0), "null argument"), (dict(ws=0), "null argument"), (dict(descs=[]), "null argument"),
        (dict(sizes=[(2, 2)] * 1025), "n outside"), (dict(m=0), "m outside"), (dict(m=65), "m outside"),
        (dict(hp=0), "hp or wp"), (dict(wp=1025), "hp or wp"), (dict(k=0), "k outside"), (dict(k=2**20 + 1), "k outside"),
        (dict(D=0), "max_det outside"), (dict(D=1025), "max_det outside"),
        (dict(sizes=[(2, 2)] * 1024, D=64, ws_bytes=2**40), "exceeds 65535"),
        (dict(net=(0, 64)), "net_w or net_h"), (dict(net=(64, 65536)), "net_w or net_h"),
        (dict(protos=(0, 1, 100, 10, 1)), "protos has a null pointer"), (dict(coeffs=(0, 0, 1, 1, 1)), "coeffs has a null pointer"),
        (dict(protos=(0x2000, 3, 100, 10, 1)), "dtype 3"), (dict(coeffs=(0x3000, -1, 1, 1, 1)), "dtype -1"),
        (dict(protos=(0x2001, 1, 100, 10, 1)), "not aligned to its element"), (dict(coeffs=(0x3002, 0, 1, 1, 1)), "not aligned"),
        (dict(protos=(0x2000, 1, -1, 10, 1)), "strides"), (dict(coeffs=(0x3000, 0, 1, 2**41, 1)), "strides"),
        (dict(nc=0), "n_colours below 1"), (dict(alpha=256), "alpha outside"), (dict(alpha=-2), "alpha outside"),
        (dict(dets=0x4002), "not 4-byte aligned"), (dict(rects=0x5001), "not 4-byte aligned"),
        (dict(colours=0x6002), "not 4-byte aligned"),
        (dict(sizes=((64, 48), (3, 2))), "even width and height"), (dict(sizes=((64, 48), (0, 2))), "outside 1..65535"),
        (dict(sizes=((64, 48), (65536, 2)), fmt="RGB"), "outside 1..65535"), (dict(plane=0), "plane 0 is null"),
        (dict(pitch=63), "shorter than a row"), (dict(params=False), "needs params"),
        (dict(ws=0x10008), "not 16-byte aligned"), (dict(ws_bytes=2 * 4 * 16 * 16 * 4 - 1), "workspace is smaller"),
    ]
    for kw, text in cases:
        rc, err = call(**kw)
        assert rc == shim.ERR_INVALID_ARG and text in err and "vali_mask_paint" in err, (kw, rc, err)
    mixed = [shim.SurfaceDesc([0x7000] * 3, [192] * 3, 64, 48, int(vali.NV12)),
             shim.SurfaceDesc([0x7000] * 3, [192] * 3, 64, 48, int(vali.YUV420))]
    rc, err = call(descs=mixed)
    assert rc == shim.ERR_INVALID_ARG and "one format per batch" in err
    rc, err = call(fmt=int(vali.Y))
    assert rc == shim.ERR_UNSUPPORTED and "format" in err
