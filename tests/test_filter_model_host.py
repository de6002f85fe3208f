"""The CPU oracle's resizers and rotation against the float64 statement of their definitions (tests/filter_model.py).

Every other test of these operators asks that two co-designed float32 restatements -- oracle and kernel -- agree.  These ask
that the oracle computes the filter its comments describe: whole planes, every element type and channel count, every branch of
the definition (both pass orders, clamped borders, planes smaller than the tap span, saturation at both ends of the range).
Integer outputs must EQUAL quantise(model) except within a measured window around rounding ties; float outputs stay within a
measured multiple of float32 epsilon times the abs-weighted sum.  `python tests/test_filter_model_host.py` prints the
measurements the constants of filter_model.py were taken from."""
import itertools
import zlib

import numpy as np
import pytest

import filter_model as fm

KINDS = ("linear", "cubic", "lanczos")
VALUE_RANGES = ("u8", "u10", "u16", "f32")

# (name, sw, sh, dw, dh, rings): rings = the longer filters must overshoot BOTH ends of the value range in the model (every
# geometry but the two that are a single point sample, where the value itself sits at the ends)
RESIZE_GEOMS = [("shrink_both", 97, 61, 41, 29, True), ("shrink_both_b", 130, 70, 58, 34, True), ("grow_both", 41, 29, 97, 61, True),
                ("shrink_x_grow_y", 97, 29, 41, 61, True), ("grow_x_shrink_y", 41, 61, 97, 29, True),
                ("rows_kept", 97, 61, 41, 61, True), ("columns_kept", 41, 29, 41, 61, True),
                ("1x1_to_5x3", 1, 1, 5, 3, False), ("3x2_to_1x1", 3, 2, 1, 1, False), ("4x1_to_9x3", 4, 1, 9, 3, True),
                ("narrower_than_the_taps", 2, 2, 14, 10, True)]

ROT_W, ROT_H, ROT_DW, ROT_DH = 131, 77, 140, 90


def centred(angle, w=ROT_W, h=ROT_H, dw=ROT_DW, dh=ROT_DH):
    """shifts (to 1/100) that put the source's centre on the destination's"""
    r = np.deg2rad(angle)
    cx, cy = (w - 1) / 2, (h - 1) / 2
    return (round((dw - 1) / 2 - (np.cos(r) * cx + np.sin(r) * cy), 2), round((dh - 1) / 2 - (-np.sin(r) * cx + np.cos(r) * cy), 2))


# (name, angle, sx, sy)
ROTATE_CASES = [(f"{a}deg", a, *centred(a)) for a in (30.0, -47.3, 163.0, 10.0, 271.5)] + [("mostly_outside", 30.0, 118.0, 40.0)]


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def resize_inputs(name, sw, sh, channels, value_range):
    """one noise plane, or for planes too small to hold both levels next to noise the two-level pattern and its swap"""
    small = sw < 8
    return [fm.noise_plane(np.random.default_rng(seed_of(name, channels, value_range, v)), sh, sw, channels, value_range, v)
            for v in ((0, 1) if small else (0,))]


def plant_corner(plane, channels, value_range):
    """plateaus of hi | 0 in the source's top left corner: what "mostly_outside" leaves inside the destination"""
    hi = fm.RANGES[value_range][1]
    p = plane.reshape(plane.shape[0], -1, channels)
    p[0:6, 0:4], p[0:6, 4:8] = hi, 0
    return plane


def rotate_input(name, channels, value_range):
    plane = fm.noise_plane(np.random.default_rng(seed_of(name, channels, value_range)), ROT_H, ROT_W, channels, value_range)
    return plant_corner(plane, channels, value_range) if name == "mostly_outside" else plane


def check_ends(ms, kind, value_range, rings):
    """every integer case reaches both ends of its range in the model: the stored value is 0 somewhere and `hi` (or above)
    somewhere; where the filter has negative lobes the model moreover leaves the range on both sides by more than half an
    LSB, so that the store clips below and -- at the full range of the type -- above (a 10-bit plane must NOT be clipped at
    1023: the model's overshoot is stored as it is)."""
    hi = fm.RANGES[value_range][1]
    lo_m, hi_m = min(m.min() for m in ms), max(m.max() for m in ms)
    assert lo_m < 0.5 and hi_m >= hi - 0.5, (lo_m, hi_m)
    if rings and kind != "linear":
        assert lo_m < -0.5 and hi_m > hi + 0.5, (lo_m, hi_m)


def each(check, oracle, *axes):
    """the full product of the axes through one check; a failure names the combination"""
    for combo in itertools.product(*axes):
        try:
            check(oracle, *combo)
        except AssertionError as e:
            raise AssertionError(combo) from e


@pytest.mark.parametrize("geom", RESIZE_GEOMS, ids=[g[0] for g in RESIZE_GEOMS])
def test_resize(oracle, geom):
    """every filter, 1 / 2 / 3 channels, every value range at one geometry"""
    each(check_resize, oracle, [geom], KINDS, (1, 2, 3), VALUE_RANGES)


def check_resize(oracle, geom, kind, channels, value_range):
    name, sw, sh, dw, dh, rings = geom
    dt = fm.RANGES[value_range][0]
    ms = []
    for plane in resize_inputs(name, sw, sh, channels, value_range):
        got = oracle.resize_plane(plane, channels, dw, dh, kind)
        m, big = fm.resize(plane, channels, dw, dh, kind)
        ms.append(m)
        if dt == np.float32:
            fm.compare_float(got, m, big, fm.C_FLOAT["resize", kind])
        else:
            share = fm.compare(got, m, dt, fm.TAU["resize", kind, value_range])
            assert share <= fm.NEAR_TIE_CAP[value_range], share
    if dt != np.float32:
        check_ends(ms, kind, value_range, rings)


def rotate_both_fills(oracle, plane, channels, dw, dh, angle, sx, sy):
    """the oracle's output over two different backgrounds -> (values, mask of the pixels it wrote)"""
    outs = [oracle.rotate_plane(plane, channels, dw, dh, angle, sx, sy, fill=f) for f in (3, 200)]
    untouched = (outs[0] != outs[1]).reshape(dh, dw, channels)
    assert np.array_equal(untouched.any(-1), untouched.all(-1))            # a pixel is written whole or not at all
    assert np.all(outs[0][np.repeat(untouched.any(-1), channels, axis=1)] == 3)
    return outs[0], ~untouched.any(-1)


@pytest.mark.parametrize("case", ROTATE_CASES, ids=[c[0] for c in ROTATE_CASES])
def test_rotate(oracle, case):
    """1 and 3 channels, every value range at one angle"""
    each(check_rotate, oracle, [case], (1, 3), VALUE_RANGES)


def check_rotate(oracle, case, channels, value_range):
    name, angle, sx, sy = case
    dt, hi = fm.RANGES[value_range]
    plane = rotate_input(name, channels, value_range)
    got, written = rotate_both_fills(oracle, plane, channels, ROT_DW, ROT_DH, angle, sx, sy)
    m, inside, big = fm.rotate(plane, channels, ROT_DW, ROT_DH, angle, sx, sy)
    assert np.array_equal(written, inside)                                 # the untouched pixels are exactly the model's outside set
    if name == "mostly_outside":
        assert 0.02 < inside.mean() < 0.5
    else:
        assert inside.mean() > 0.5
    keep = np.repeat(inside, channels, axis=1)
    if dt == np.float32:
        fm.compare_float(got[keep], m[keep], big[keep], fm.C_FLOAT["rotate", "bilinear"])
        return
    share = fm.compare(got[keep], m[keep], dt, fm.TAU["rotate", "bilinear", value_range])
    assert share <= fm.NEAR_TIE_CAP[value_range], share
    q = fm.quantise(m[keep], dt)
    assert q.min() == 0 and q.max() == hi                                  # both ends of the range stored


def test_rotate_exact_translation_pins_round_half_even(oracle):
    each(check_exact_translation, oracle, (1, 3), VALUE_RANGES)


def check_exact_translation(oracle, channels, value_range):
    """angle 0, shift (3.5, 7.25): the weights are 1/2 and 1/4 or 3/4, every float32 operation is exact, one sample in eight
    is a rounding tie -- the stored value must be the model's rounded half to even, with no window"""
    dt, hi = fm.RANGES[value_range]
    plane = rotate_input("translation", channels, value_range)
    if dt == np.float32:
        plane = np.floor(plane)                                            # integers: the products stay exact
    got, written = rotate_both_fills(oracle, plane, channels, ROT_DW, ROT_DH, 0.0, 3.5, 7.25)
    m, inside, _ = fm.rotate(plane, channels, ROT_DW, ROT_DH, 0.0, 3.5, 7.25)
    assert np.array_equal(written, inside) and inside.mean() > 0.5
    keep = np.repeat(inside, channels, axis=1)
    assert np.all(m[keep] * 8 == np.rint(m[keep] * 8))
    if dt == np.float32:
        assert np.array_equal(got[keep].astype(np.float64), m[keep])
        return
    ties = fm.tie_distance(m[keep]) == 0
    assert ties.mean() > 0.05
    assert np.array_equal(got[keep], fm.quantise(m[keep], dt))
    assert np.any(got[keep][ties] % 2 == 0) and not np.any(got[keep][ties] % 2 == 1)    # the ties went to the even neighbour


def test_resize_exact_ties_bilinear_doubling(oracle):
    each(check_exact_doubling, oracle, (1, 2, 3), VALUE_RANGES)


def check_exact_doubling(oracle, channels, value_range):
    """bilinear 2x growth of integer data: weights 0, 1/2, 1 -- exact in float32, ties on a good part of the samples, no window"""
    dt, hi = fm.RANGES[value_range]
    sw, sh = 24, 16
    plane = fm.noise_plane(np.random.default_rng(seed_of("doubling", channels, value_range)), sh, sw, channels, value_range)
    if dt == np.float32:
        plane = np.floor(plane)
    got = oracle.resize_plane(plane, channels, 2 * sw, 2 * sh, "linear")
    m, _ = fm.resize(plane, channels, 2 * sw, 2 * sh, "linear")
    assert np.all(m * 4 == np.rint(m * 4))
    if dt == np.float32:
        assert np.array_equal(got.astype(np.float64), m)
        return
    assert (fm.tie_distance(m) == 0).mean() > 0.2
    assert np.array_equal(got, fm.quantise(m, dt))


# ---- the measurements behind filter_model's constants -------------------------------------------------------------------------
def measure():
    """Oracle against model over every case of this file and, on the CPU as well, over the inputs of the GPU file
    (tests/test_gpu_filter_model.py: other geometries, whole surfaces): what filter_model.TAU and C_FLOAT are set from."""
    from oracle import oracle as o
    import test_gpu_filter_model as g

    o.lib()
    tie, c_float, differing, share = {}, {}, {}, {}

    def note(op, kind, vr, got, m, big):
        dt = fm.RANGES[vr][0]
        if dt == np.float32:
            ok = big > 0
            assert np.all(got[~ok] == 0)
            ratio = (np.abs(got.astype(np.float64) - m)[ok] / (2.0 ** -23 * big[ok])).max(initial=0.0)
            c_float[op, kind] = max(c_float.get((op, kind), 0.0), float(ratio))
            return
        key = (op, kind, vr)
        d = got.astype(np.int64) - fm.quantise(m, dt).astype(np.int64)
        assert np.abs(d).max(initial=0) <= 1, key
        tie[key] = max(tie.get(key, 0.0), float(fm.tie_distance(m)[d != 0].max(initial=0.0)))
        differing[key] = max(differing.get(key, 0.0), float((d != 0).mean()))
        if m.size >= 500:
            share[key] = max(share.get(key, 0.0), float((fm.tie_distance(m) < fm.TAU[key]).mean()))

    for (name, sw, sh, dw, dh, _), kind, ch, vr in itertools.product(RESIZE_GEOMS, KINDS, (1, 2, 3), VALUE_RANGES):
        for plane in resize_inputs(name, sw, sh, ch, vr):
            m, big = fm.resize(plane, ch, dw, dh, kind)
            note("resize", kind, vr, o.resize_plane(plane, ch, dw, dh, kind), m, big)
    for (name, angle, sx, sy), ch, vr in itertools.product(ROTATE_CASES, (1, 3), VALUE_RANGES):
        plane = rotate_input(name, ch, vr)
        m, inside, big = fm.rotate(plane, ch, ROT_DW, ROT_DH, angle, sx, sy)
        keep = np.repeat(inside, ch, axis=1)
        got = o.rotate_plane(plane, ch, ROT_DW, ROT_DH, angle, sx, sy)
        note("rotate", "bilinear", vr, got[keep], m[keep], big[keep])
    for p in g.resize_params():
        geom, fmt, kind, point = p.values
        (sw, sh, dw, dh), planes, host, vr, want = g.resize_case(geom, fmt, kind, point, o)
        for w, pl, (qw, qh, ch) in zip(g.split(want, fmt, dw, dh, o), planes, o.host_planes(fmt, dw, dh)):
            m, big = fm.resize(pl, ch, qw, qh, kind)
            note("resize", kind, vr, w, m, big)
    for p in g.rotate_params():
        fmt, geom, angle, sx, sy, exact = p.values
        if exact:                     # (the translation by halves and quarters: all ties, no noise -- nothing to measure)
            continue
        (sw, sh, dw, dh), planes, host, vr, wants = g.rotate_case(fmt, geom, angle, sx, sy, exact, o)
        for w, pl, (qw, qh, ch) in zip(g.split(wants[0], fmt, dw, dh, o), planes, o.host_planes(fmt, dw, dh)):
            m, inside, big = fm.rotate(pl, ch, qw, qh, angle, sx, sy)
            keep = np.repeat(inside, ch, axis=1)
            note("rotate", "bilinear", vr, w[keep], m[keep], big[keep])
    print("largest distance from a tie of a sample that differs from quantise(model), in LSB (0 = none differs):")
    for k in tie:
        print(f"  {k}: {tie[k]:.3e}   largest share differing {differing[k]:.3%}   largest share inside TAU (planes >= 500 samples) {share.get(k, 0):.2%}")
    print("largest |oracle - model| / (2^-23 A) of a float32 sample:")
    for k in c_float:
        print(f"  {k}: {c_float[k]:.2f}")


if __name__ == "__main__":
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    measure()

