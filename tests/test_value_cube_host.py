"""The frames of tests/value_cube.py hold what they claim (every triple, every 16-bit value), and the two CPU statements
of RGB -> YUV (tests/postproc_model.py) agree on all 2^24 colours: the reference side of tests/test_gpu_value_cube.py,
settled without a GPU."""
import numpy as np
import pytest

import postproc_model as pm
import value_cube as vc


# ---- the cubes ----------------------------------------------------------------------------------------------------------
def test_nv12_cube_layout_and_every_triple_once():
    a = vc.nv12_cube()
    assert a.shape == (6144, 4096) and a.dtype == np.uint8
    # the layout as the definition words it, at a few chroma samples
    for c in (0, 1, 63, 64, 2047, 2048, (1 << 14) - 1, 1 << 14, 123456, (1 << 22) - 1):
        cy, cx = divmod(c, 2048)
        assert (a[4096 + cy, 2 * cx], a[4096 + cy, 2 * cx + 1]) == ((c >> 6) & 255, c >> 14)
        for dy in (0, 1):
            for dx in (0, 1):
                assert a[2 * cy + dy, 2 * cx + dx] == 4 * (c & 63) + 2 * dy + dx
    counts = vc.triple_counts(*vc.nv12_triples(a))
    assert counts.size == 1 << 24 and (counts == 1).all()


def test_rgb_cube_layout_and_every_triple_once():
    p = vc.rgb_cube()
    assert p.shape == (4096, 4096, 3) and p.dtype == np.uint8
    for k in (0, 1, 255, 256, 65535, 65536, 0xabcdef, (1 << 24) - 1):
        assert tuple(p[k // 4096, k % 4096]) == (k >> 16, (k >> 8) & 255, k & 255)
    counts = vc.triple_counts(p[..., 0], p[..., 1], p[..., 2])
    assert (counts == 1).all()


def test_ragged_twins_are_the_cubes_plus_two_columns():
    a, r = vc.nv12_cube(), vc.nv12_cube(ragged=True)
    assert r.shape == (6144, 4098) and np.array_equal(r[:, :4096], a) and np.array_equal(r[:, 4096:], a[:, :2])
    counts = vc.triple_counts(*vc.nv12_triples(r))
    assert counts.min() == 1 and counts.sum() == 4096 * 4098
    p, q = vc.rgb_cube(), vc.rgb_cube(ragged=True)
    assert q.shape == (4096, 4098, 3) and np.array_equal(q[:, :4096], p) and np.array_equal(q[:, 4096:], p[:, :2])
    counts = vc.triple_counts(q[..., 0], q[..., 1], q[..., 2])
    assert counts.min() == 1 and counts.sum() == 4096 * 4098


@pytest.mark.parametrize("ragged", [False, True])
def test_host_images_hold_every_triple(ragged):
    w, h = vc.cube_width(ragged), vc.SIDE
    for fmt in ("YUV444", "RGB_PLANAR"):
        planes = vc.host_image(fmt, ragged).reshape(3, h, w)
        assert vc.triple_counts(*planes).min() == 1
    flat = vc.host_image("YUV420", ragged)
    assert flat.size == w * h * 3 // 2
    y, u, v = flat[:w * h].reshape(h, w), flat[w * h:w * h * 5 // 4], flat[w * h * 5 // 4:]
    nv = vc.nv12_cube(ragged)
    assert np.array_equal(y, nv[:h]) and np.array_equal(u.reshape(h // 2, w // 2), nv[h:, 0::2])
    assert np.array_equal(v.reshape(h // 2, w // 2), nv[h:, 1::2])
    for fmt in ("RGB", "BGR"):
        px = vc.host_image(fmt, ragged).reshape(h, w, 3)
        assert vc.triple_counts(px[..., 0], px[..., 1], px[..., 2]).min() == 1


def test_p16_frame_holds_every_value_in_each_plane():
    f = vc.p16_frame()
    assert f.shape == (384, 512) and f.dtype == np.uint16
    luma = np.bincount(f[:256].reshape(-1), minlength=1 << 16)
    chroma = np.bincount(f[256:].reshape(-1), minlength=1 << 16)
    assert luma.size == 1 << 16 and (luma == 2).all()
    assert chroma.size == 1 << 16 and (chroma == 1).all()
    # both members of the interleaved pairs see low bits set
    assert (f[256:, 0::2] & 63).any() and (f[256:, 1::2] & 63).any()


def test_the_cubes_are_shared_and_read_only():
    assert vc.rgb_cube() is vc.rgb_cube() and vc.nv12_cube() is vc.nv12_cube()
    with pytest.raises(ValueError):
        vc.rgb_cube()[0, 0, 0] = 1


# ---- locating an element ------------------------------------------------------------------------------------------------
def test_locate_names_the_pixel_of_an_element():
    w, h = 6, 4
    assert vc.locate("RGB", w, h, 3 * (2 * w + 5) + 1) == (5, 2, "G")
    assert vc.locate("BGR", w, h, 3 * (2 * w + 5)) == (5, 2, "B")
    assert vc.locate("RGB_32F", w, h, 3 * (1 * w + 2) + 2) == (2, 1, "B")
    assert vc.locate("RGB_PLANAR", w, h, 2 * w * h + 3 * w + 1) == (1, 3, "B")
    assert vc.locate("YUV444", w, h, w * h + 1) == (1, 0, "U")
    assert vc.locate("NV12", w, h, 2 * w + 3) == (3, 2, "Y")
    assert vc.locate("NV12", w, h, w * h + w + 3) == (2, 2, "V")
    assert vc.locate("YUV420", w, h, w * h + 4) == (2, 2, "U")
    assert vc.locate("YUV420", w, h, w * h + 6 + 5) == (4, 2, "V")


def test_a_difference_is_reported_as_triples_not_as_arrays():
    nv = vc.nv12_cube()
    want = np.zeros(4096 * 4096 * 3, np.uint8)
    got = want.copy()
    i = 3 * (5 * 4096 + 130) + 2
    got[i], got[-1] = 7, 9
    with pytest.raises(AssertionError) as e:
        vc.assert_same(got, want, "RGB", 4096, 4096, vc.nv12_triple_at(nv), "case")
    msg = str(e.value)
    y, u, v = int(nv[5, 130]), int(nv[4096 + 2, 130]), int(nv[4096 + 2, 131])
    assert "2 of 50331648 elements differ" in msg and f"({y}, {u}, {v}) at (130, 5) B -> got 7, want 0" in msg
    assert len(msg) < 400
    vc.assert_same(want, want.copy(), "RGB", 4096, 4096, vc.nv12_triple_at(nv), "case")
    # floats are compared by their bits: -0.0 is not 0.0, a NaN equals itself
    a = np.array([0.0, np.nan], np.float32)
    assert vc.differences(a, a.copy(), str) is None
    assert "1 of 2" in vc.differences(a, np.array([-0.0, np.nan], np.float32), str)


# ---- the two CPU statements of RGB -> YUV ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dst", ["YUV444", "NV12"])
@pytest.mark.parametrize("matrix", ["601_JPEG", "601_MPEG", "709_JPEG", "709_MPEG"])
def test_oracle_and_numpy_statements_agree_on_every_colour(oracle, matrix, dst):
    """from_rgb (the C oracle) and numpy_yuv (float64 products rounded once per fmaf) on all 2^24 colours: a disagreement
    would be a finding about the reference side, to settle by include/vali_hip.h before any GPU result is judged"""
    p = vc.rgb_cube()
    rows = pm.matrices()[matrix]
    a = pm.from_rgb(oracle, p, dst, rows)
    b = pm.numpy_yuv(p, rows, dst)
    vc.assert_same(a, b, dst, vc.SIDE, vc.SIDE, vc.rgb_triple_at(p), f"from_rgb against numpy_yuv, {matrix} {dst}")
