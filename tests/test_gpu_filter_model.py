"""PySurfaceResizer and PySurfaceRotator on the GPU against the float64 statement of their definitions (tests/filter_model.py),
one case per kernel form at the smallest geometry that reaches it, under the rule and the constants of the host test
(tests/test_filter_model_host.py): integer samples EQUAL quantise(model) outside a measured window around rounding ties, float
samples stay within a measured multiple of epsilon times the abs-weighted sum.  The same inputs must also give the oracle's
bytes: 16-bit planes here span the whole 0 .. 65535 (the bit-exact suites draw 0 .. 999), with plateaus of 65535 against
plateaus of 0, so the stores saturate at both ends and the intermediates use all 16 bits.

Which kernel a case reaches is read from the dispatch (vali_amd/csrc/resize.hip launch_resize and the *_fits / launch_*
functions of resize_cols.hip, resize_rows.hip, resize_up2.hip, resize_taps.hip; rotate.hip vali_rotate) and named in the
case's id.  Geometries are PLANE sizes (test_gpu_resize.plane_geometry turns them into surface sizes for subsampled formats)."""
import zlib

import numpy as np
import pytest

import filter_model as fm
from test_filter_model_host import ROTATE_CASES, ROT_DH, ROT_DW, ROT_H, ROT_W, check_ends, plant_corner
from test_gpu_resize import plane_geometry, roundtrip

pytestmark = pytest.mark.gpu

VALUE_RANGE = {"P10": "u16", "YUV444_10bit": "u16", "RGB_32F": "f32"}       # every other format: 8 bits


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def make_surface(fmt, sw, sh, oracle, key, point=None, gap=0):
    """flat host image of a `fmt` surface: every plane a fm.noise_plane.  point = (kx, ky): the plane is about to be point
    sampled at that stride, so source row ky carries both ends of the range at the sampled columns."""
    vr = VALUE_RANGE.get(fmt, "u8")
    dt, hi = fm.RANGES[vr]
    planes = []
    for k, (pw, ph, ch) in enumerate(oracle.host_planes(fmt, sw, sh)):
        p = fm.noise_plane(np.random.default_rng(seed_of(key, k)), ph, pw, ch, vr, gap=gap)
        if point:
            kx, ky = point
            p3 = p.reshape(ph, pw, ch)
            p3[ky] = np.where((np.arange(pw) // kx) % 2 == 0, hi, 0).astype(dt)[:, None]
        planes.append(p)
    return planes, np.concatenate([p.reshape(-1) for p in planes]), vr


def split(flat, fmt, w, h, oracle):
    out, off = [], 0
    for pw, ph, ch in oracle.host_planes(fmt, w, h):
        out.append(flat[off: off + pw * ph * ch].reshape(ph, pw * ch))
        off += pw * ph * ch
    assert off == flat.size
    return out


def check_resize(got, planes, want, fmt, dw, dh, kind, vr, rings, oracle):
    """got, want: flat destination images (GPU, oracle); planes: the source planes"""
    dt = fm.RANGES[vr][0]
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))                     # the oracle's bytes, at the full range
    ms, near, total = [], 0.0, 0
    for g, p, (qw, qh, ch) in zip(split(got, fmt, dw, dh, oracle), planes, oracle.host_planes(fmt, dw, dh)):
        m, big = fm.resize(p, ch, qw, qh, kind)
        if dt == np.float32:
            fm.compare_float(g, m, big, fm.C_FLOAT["resize", kind])
            continue
        # the forms for 3:2 and 1:2 sample at phases 0 and 1/2, where the bicubic weights are sixteenths: on 8-bit planes every
        # float32 operation is then exact and one sample in thirty a true tie -- no window there, round half to even or fail
        ph, pw = p.shape[0], p.shape[1] // ch
        sixteenths = kind == "cubic" and vr == "u8" and 2 * pw % qw == 0 and 2 * ph % qh == 0
        near += fm.compare(g, m, dt, 0.0 if sixteenths else fm.TAU["resize", kind, vr]) * m.size
        total += m.size
        ms.append(m)
    if dt != np.float32:
        assert near / total <= fm.NEAR_TIE_CAP[vr], near / total
        check_ends(ms, kind, vr, rings)


# ---- resize: (kernel form, plane geometry, formats, filters[, point stride]) ------------------------------------------------------
INT8_16 = ("Y", "NV12", "P10", "YUV444_10bit")
RESIZE_CASES = [
    # bilinear, any ratio: k_resize<T, MAXC>
    ("k_resize", (130, 70, 58, 34), ("Y", "NV12", "RGB", "P10", "YUV444_10bit", "RGB_32F"), ("linear",)),
    ("k_resize", (41, 29, 97, 61), ("Y", "NV12", "RGB", "P10", "YUV444_10bit", "RGB_32F"), ("linear",)),
    # integer ratios: every filter is the point sample.  3:1 / 2:1 along x on 8-bit planes of 1 / 2 channels: k_resize_pointk<3>, <2>;
    # 12:1 (and 16-bit, 3-channel planes): the point form of k_resize
    ("k_resize_pointk", (1002, 36, 334, 18), ("Y", "NV12"), ("lanczos", "cubic"), (3, 2)),
    ("k_resize_pointk", (84, 40, 42, 40), ("Y",), ("lanczos",), (2, 1)),
    ("k_resize_point", (1200, 64, 100, 16), ("Y", "RGB", "P10", "YUV444_10bit"), ("lanczos",), (12, 4)),
    # planes that shrink down the rows: columns first (resize_cols.hip).  3:2 along x on every plane, 8 | dst row: _x32;
    # 2:1 along x: _x2; any other ratio, packed RGB and float planes: the specialised waves, _ws
    ("k_resize_cols_x32", (24, 100, 16, 50), ("Y", "NV12", "P10", "YUV444_10bit"), ("lanczos", "cubic")),
    ("k_resize_cols_x2", (636, 364, 318, 310), ("Y", "NV12", "P10", "YUV444_10bit"), ("lanczos", "cubic")),
    ("k_resize_cols_ws", (1282, 360, 640, 250), ("Y", "NV12", "RGB", "P10", "RGB_32F"), ("lanczos", "cubic")),
    ("k_resize_cols_ws", (1000, 700, 1400, 300), ("Y", "RGB"), ("lanczos",)),                      # shrink rows, stretch columns
    ("k_resize_cols_ws", (700, 540, 334, 540), ("Y", "RGB", "P10"), ("lanczos", "cubic")),          # rows kept
    # planes that grow down the rows: rows first (resize_rows.hip).  1 / 2 channels of 8 or 16 bits: k_resize_rows.  8-bit planes
    # under Lanczos whose rows grow by less than 3x from at least 16 pixels (rows_reg_fits) filter from registers: k_resize_rows_reg
    # for 1 / 2 channels, k_resize_rows_rgb for packed RGB
    ("k_resize_rows_reg", (100, 40, 250, 90), ("Y", "NV12"), ("lanczos",)),
    ("k_resize_rows_reg", (16, 8, 40, 17), ("Y",), ("lanczos",)),
    ("k_resize_rows_reg", (130, 30, 259, 61), ("Y", "NV12"), ("lanczos",)),
    ("k_resize_rows_rgb", (100, 40, 250, 90), ("RGB",), ("lanczos",)),
    ("k_resize_rows_rgb", (16, 8, 40, 17), ("RGB",), ("lanczos",)),                                # one tile, both image edges in it
    ("k_resize_rows_rgb", (130, 30, 259, 61), ("RGB",), ("lanczos",)),                             # an odd last pixel
    ("k_resize_rows", (100, 40, 250, 90), ("P10", "YUV444_10bit"), ("lanczos", "cubic")),
    ("k_resize_rows", (100, 40, 250, 90), ("Y", "NV12"), ("cubic",)),
    ("k_resize_rows", (62, 30, 201, 67), INT8_16, ("lanczos", "cubic")),
    ("k_resize_rows", (2, 2, 14, 10), INT8_16, ("lanczos", "cubic")),                              # narrower than the tap span
    ("k_resize_rows", (4, 1, 9, 3), INT8_16, ("lanczos", "cubic")),
    ("k_resize_rows", (130, 66, 516, 67), INT8_16, ("lanczos",)),
    # exactly 2:3 on both axes: k_resize_rows_x23 (packed 8-bit RGB: k_resize_rows_x23_rgb)
    ("k_resize_rows_x23", (8, 6, 12, 9), INT8_16, ("lanczos", "cubic")),
    ("k_resize_rows_x23", (258, 10, 387, 15), INT8_16, ("lanczos",)),
    ("k_resize_rows_x23", (100, 66, 150, 99), INT8_16, ("lanczos", "cubic")),
    ("k_resize_rows_x23_rgb", (8, 6, 12, 9), ("RGB",), ("lanczos", "cubic")),
    ("k_resize_rows_x23_rgb", (258, 10, 387, 15), ("RGB",), ("lanczos",)),
    ("k_resize_rows_x23_rgb", (100, 66, 150, 99), ("RGB",), ("lanczos",)),
    # planes of 1 / 2 channels exactly doubled both ways, rows a multiple of 4 elements: k_resize_up2
    ("k_resize_up2", (16, 6, 32, 12), INT8_16, ("lanczos", "cubic")),
    # (36 x 4 without NV12: its chroma plane has two rows, and between two clamped rows the doubled filter is their exact mean --
    # a rounding tie on every other sample of that output row)
    ("k_resize_up2", (36, 4, 72, 8), ("Y", "P10", "YUV444_10bit"), ("lanczos",)),
    ("k_resize_up2", (248, 20, 496, 40), INT8_16, ("lanczos", "cubic")),
    ("k_resize_up2", (500, 37, 1000, 74), INT8_16, ("lanczos",)),
    # what grows down the rows and fits none of the forms above: k_resize_taps -- float planes, packed RGB under bicubic or
    # outside the register form's ratios, and planes of 1 / 2 channels whose rows shrink 3:1 (more source groups per tile than
    # a wave has lanes)
    ("k_resize_taps", (100, 40, 250, 90), ("RGB_32F",), ("lanczos", "cubic")),
    ("k_resize_taps", (100, 40, 250, 90), ("RGB",), ("cubic",)),
    ("k_resize_taps", (62, 30, 201, 67), ("RGB",), ("lanczos",)),
    ("k_resize_taps", (2, 2, 14, 10), ("RGB", "RGB_32F"), ("lanczos",)),
    ("k_resize_taps", (130, 66, 516, 67), ("RGB",), ("lanczos",)),
    ("k_resize_taps", (300, 50, 100, 65), ("P10", "NV12"), ("lanczos", "cubic")),
]


def resize_params():
    for case in RESIZE_CASES:
        form, geom, fmts, kinds = case[:4]
        for fmt in fmts:
            for kind in kinds:
                yield pytest.param(geom, fmt, kind, case[4] if len(case) > 4 else None,
                                   id=f"{form}-{'x'.join(map(str, geom[:2]))}to{'x'.join(map(str, geom[2:]))}-{fmt}-{kind}")


def resize_case(geom, fmt, kind, point, oracle):
    """(surface sizes, source planes, flat host image, value range, oracle's output)"""
    sw, sh, dw, dh = plane_geometry(fmt, *geom, min_w=8 if 3 * geom[0] == 2 * geom[2] else 0)
    doubled = (dw, dh) == (2 * sw, 2 * sh)         # midway between a plateau of hi and one of 0 lies an exact tie: part them
    planes, host, vr = make_surface(fmt, sw, sh, oracle, ("resize", geom, fmt, kind), point, gap=2 if doubled else 0)
    return (sw, sh, dw, dh), planes, host, vr, oracle.resize_surface(host, fmt, sw, sh, dw, dh, kind)


FORMS = list(dict.fromkeys(case[0] for case in RESIZE_CASES))


@pytest.mark.parametrize("form", FORMS)
def test_resize(vali, gpu, oracle, form):
    """one test per kernel form (a few seconds each); a failure names the case"""
    for p in resize_params():
        if p.id.split("-")[0] != form:
            continue
        geom, fmt, kind, point = p.values
        (sw, sh, dw, dh), planes, host, vr, want = resize_case(geom, fmt, kind, point, oracle)
        got = roundtrip(vali, gpu, fmt, host, sw, sh, dw, dh, interp=vali.Interpolation[kind.upper()])
        try:
            check_resize(got, planes, want, fmt, dw, dh, kind, vr, point is None, oracle)
        except AssertionError as e:
            raise AssertionError(p.id) from e


# ---- rotation by any angle: k_rotate_affine_lds (planes narrower than a staged row: the gather form k_rotate_affine) -----------
ROT_FORMATS = ("RGB", "BGR", "Y", "YUV444", "YUV420", "YUV444_10bit", "RGB_32F")
NARROW_ANGLE = (38.0, 60.0, 20.0)                        # source widths around the staged rows, x 150 -> 200 x 180
MOSTLY_OUTSIDE = next((sx, sy) for name, _, sx, sy in ROTATE_CASES if name == "mostly_outside")


def rotate_params():
    for name, angle, sx, sy in ROTATE_CASES:
        for fmt in ROT_FORMATS:
            yield pytest.param(fmt, (ROT_W, ROT_H, ROT_DW, ROT_DH), angle, sx, sy, False, id=f"k_rotate_affine_lds-{name}-{fmt}")
    for sw in (47, 48, 49, 95, 96, 100):
        for fmt in ("RGB", "Y", "YUV444_10bit", "RGB_32F"):
            yield pytest.param(fmt, (sw, 150, 200, 180), *NARROW_ANGLE, False, id=f"k_rotate_affine_lds-width{sw}-{fmt}")
    for fmt in ROT_FORMATS:
        yield pytest.param(fmt, (ROT_W, ROT_H, ROT_DW, ROT_DH), 0.0, 3.5, 7.25, True, id=f"k_rotate_affine_lds-translation-{fmt}")


def rotate_case(fmt, geom, angle, sx, sy, exact, oracle):
    sw, sh, dw, dh = plane_geometry("NV12" if fmt == "YUV420" else fmt, *geom)
    planes, host, vr = make_surface(fmt, sw, sh, oracle, ("rotate", geom, fmt, angle))
    if exact and vr == "f32":
        planes = [np.floor(p) for p in planes]
    if (sx, sy) == MOSTLY_OUTSIDE:
        planes = [plant_corner(p, ch, vr) for p, (_, _, ch) in zip(planes, oracle.host_planes(fmt, sw, sh))]
    host = np.concatenate([p.reshape(-1) for p in planes])
    wants = [np.concatenate([oracle.rotate_plane(p, ch, qw, qh, angle, sx, sy, fill=f).reshape(-1)
                             for p, (qw, qh, ch) in zip(planes, oracle.host_planes(fmt, dw, dh))]) for f in (3, 200)]
    return (sw, sh, dw, dh), planes, host, vr, wants


def check_rotate(gots, planes, wants, fmt, dw, dh, angle, sx, sy, vr, exact, oracle):
    """gots, wants: the flat destination images over backgrounds of 3 and of 200"""
    dt, hi = fm.RANGES[vr]
    for g, w in zip(gots, wants):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8))                      # the oracle's bytes
    near, total, qs = 0.0, 0, []
    for g3, g200, p, (qw, qh, ch) in zip(split(gots[0], fmt, dw, dh, oracle), split(gots[1], fmt, dw, dh, oracle), planes,
                                         oracle.host_planes(fmt, dw, dh)):
        m, inside, big = fm.rotate(p, ch, qw, qh, angle, sx, sy)
        untouched = (g3 != g200).reshape(qh, qw, ch)
        assert np.array_equal(untouched.all(-1), ~inside) and np.array_equal(untouched.any(-1), ~inside)   # exactly the model's outside set
        keep = np.repeat(inside, ch, axis=1)
        assert np.all(g3[~keep] == 3)
        if exact:
            assert np.array_equal(g3[keep].astype(np.float64), m[keep] if dt == np.float32 else fm.quantise(m[keep], dt))
            continue
        if dt == np.float32:
            fm.compare_float(g3[keep], m[keep], big[keep], fm.C_FLOAT["rotate", "bilinear"])
            continue
        near += fm.compare(g3[keep], m[keep], dt, fm.TAU["rotate", "bilinear", vr]) * keep.sum()
        total += keep.sum()
        qs.append(fm.quantise(m[keep], dt))
    if qs:
        assert near / total <= fm.NEAR_TIE_CAP[vr], near / total
        assert min(q.min() for q in qs) == 0 and max(q.max() for q in qs) == hi         # both ends of the range stored


def run_rotation(vali, gpu, oracle, fmt, geom, angle, sx, sy, exact):
    (sw, sh, dw, dh), planes, host, vr, wants = rotate_case(fmt, geom, angle, sx, sy, exact, oracle)
    dt = fm.RANGES[vr][0]
    pf = vali.PixelFormat[fmt]
    src = vali.Surface.Make(pf, sw, sh, gpu)
    assert vali.PyFrameUploader(gpu).Run(host.view(np.uint8), src)[0]
    gots = []
    for fill in (3, 200):
        dst = vali.Surface.Make(pf, dw, dh, gpu)
        assert vali.PyFrameUploader(gpu).Run(np.full(wants[0].size, fill, dt).view(np.uint8), dst)[0]
        assert vali.PySurfaceRotator(gpu).Run(src, dst, angle, sx, sy) == (True, vali.TaskExecInfo.SUCCESS)
        out = np.zeros(dst.HostSize, np.uint8)
        assert vali.PySurfaceDownloader(gpu).Run(dst, out)[0]
        gots.append(out.view(dt))
    check_rotate(gots, planes, wants, fmt, dw, dh, angle, sx, sy, vr, exact, oracle)


@pytest.mark.parametrize("group", ["angles", "widths", "translation"])
def test_rotate(vali, gpu, oracle, group):
    """the host test's angles / source widths around the staged rows / the exact translation; a failure names the case"""
    for p in rotate_params():
        kind = p.id.split("-")[-2]
        if (group == "translation") != (kind == "translation") or (group == "widths") != kind.startswith("width"):
            continue
        try:
            run_rotation(vali, gpu, oracle, *p.values)
        except AssertionError as e:
            raise AssertionError(p.id) from e
