"""The tensor rules of the C ABI, without a GPU: what each of the eleven entry points that take a tensor answers to every
single-fault mutation of its tensor(s), and which of two faults it reports first.  Every input below is refused before the
entry point touches a device (the pointers are dummies that are never read); the code and the WHOLE text of each refusal
are compared with strings recorded from the library, kept in EXPECTED at the end of this file."""
import pytest

INF, NAN = float("inf"), float("nan")
BIG = 2 ** 40 + 1            # one past the largest stride of a head tensor
Y, RGB, NV12, YUV420 = 1, 2, 3, 4       # the vali_format values used below


def shim():
    from vali_amd._native import shim as s

    return s


def frames(fmt, plane=0x7000):
    return [shim().SurfaceDesc([plane] * 3, [3 * w] * 3, w, h, fmt) for w, h in ((64, 48), (34, 26))]


def preproc_params():
    s = shim()
    return s.PreprocParams(s.Csc(0.0, 1.0, 1.5, -0.2, -0.5, 1.8), 1.0, [0.0] * 3, [1.0] * 3)


def cvt_params():
    return shim().CvtParams(None, [[0.25, 0.5, 0.25, 0.0]] * 3)


# ---- the entry points: every argument has a legal default, a case overrides one or two ----------------------------------
DST = dict(data=0x8000, dtype=1, packed=0, n=6, w=16, h=16, sn=768, sc=256, sy=16)
SRC = dict(data=0x8000, dtype=1, packed=0, n=2, w=16, h=16, sn=768, sc=256, sy=16)
T_KEYS = ("data", "dtype", "packed", "n", "w", "h", "sn", "sc", "sy")


def tensor(cls, base, kw):
    t = dict(base)
    t.update({k: kw.pop(k) for k in T_KEYS if k in kw})
    return cls(*(t[k] for k in T_KEYS))


def nv12_preproc_roi_tensor(**kw):
    s = shim()
    t = tensor(s.TensorDst, DST, kw)
    assert not kw
    return s.nv12_preproc_roi_tensor(0x1000, 0, t, preproc_params(), True, (1, 2, 3), 0)


def rgb_preproc_roi_tensor(src_format=RGB, **kw):
    s = shim()
    t = tensor(s.TensorDst, DST, kw)
    assert not kw
    return s.rgb_preproc_roi_tensor(0x1000, 0, src_format, t, preproc_params(), True, (1, 2, 3), 0)


def warp_tensor(mats=0x6000, plane=0x7000, **kw):
    s = shim()
    t = tensor(s.TensorDst, DST, kw)
    assert not kw
    return s.warp_tensor(frames(NV12, plane), 0x1000, NV12, mats, t, preproc_params(), True, (1, 2, 3), 0)


def warp_fit(kpts=(0x2000, 1, 1000, 15, 3, 1), mp=2, tmpl=0x3000, thr=0.5):
    return shim().warp_fit(0x1000, 2, kpts, 3, 40, 5, 3, mp, tmpl, thr, 0x4000, 0x5000, 0x6000, 0)


def jpeg_encode_tensor(scale=(1.0, 1.0, 1.0), offset=(0.0, 0.0, 0.0), fmt=RGB, ws=0x10000, **kw):
    s = shim()
    t = tensor(s.TensorSrc, SRC, kw)
    assert not kw
    return s.jpeg_encode_tensor(t, scale, offset, s.jpeg_params_init(90, fmt), ws, 1 << 30, 0x20000, 1 << 20, 0x30000, 0)


def tensor_to_surfaces(scale=(1.0, 1.0, 1.0), offset=(0.0, 0.0, 0.0), bgr=0, dst_format=NV12, params=True, **kw):
    s = shim()
    t = tensor(s.TensorSrc, SRC, kw)
    assert not kw
    return s.tensor_to_surfaces(t, scale, offset, bgr, 0x1000, dst_format, cvt_params() if params else None, 0)


def detect_select(boxes=(0x2000, 1, 4000, 4, 1), scores=(0x3000, 1, 8000, 8, 1), c=8, T=100):
    return shim().detect_select(boxes, scores, 2, 1000, c, T, 10, 0.25, 0.5, 0, 0, (0, 0, 0, 0), 2, 255, 0, 0, 0, 0x5000,
                                0x6000, 0x6100, 0, 0, 0, 0, 0x10000, 1 << 30, 0)


def mask_paint(protos=(0x2000, 1, 100, 10, 1), coeffs=(0x3000, 0, 100, 10, 1), net_w=64, nc=3):
    return shim().mask_paint(frames(NV12), 0x1000, NV12, protos, coeffs, 5, 16, 16, 12, 4, net_w, 64, 0x4000, 0x5000, 0x6000,
                             nc, 128, cvt_params(), 0x10000, 1 << 30, 0)


def semantic_paint(logits=(0x2000, 1, 100, 10, 16), net_w=64, nc=3):
    return shim().semantic_paint(frames(NV12), 0x1000, NV12, logits, 5, 16, 16, net_w, 64, 0x5000, [], 0, 0x6000, nc, 128,
                                 cvt_params(), 0)


def pose_paint(kpts=(0x2000, 1, 1000, 15, 3, 1), limbs=0x3000, lc=0x6000):
    return shim().pose_paint(frames(NV12), 0x1000, NV12, kpts, 3, 12, 5, 4, limbs, 6, 0x4000, 0x5000, lc, 3, 0x6100, 2, 0.5, 3,
                             7, -1, 0x8000, cvt_params(), 0x10000, 1 << 30, 0)


def kpt_decode(dtype=1, heat=(0x2000, 4000, 800, 20), simcc=(0, 0, 0, 0, 0, 0), m=6, d_frames=0x1000):
    return shim().kpt_decode(d_frames, 2, dtype, heat, simcc, (m, 5, 16, 20), 64, 48, 0, 0, 0.5, 3, 0, 0x5000, 0x6000, 0, 0)


ENTRY = {f.__name__: f for f in (nv12_preproc_roi_tensor, rgb_preproc_roi_tensor, warp_tensor, warp_fit, jpeg_encode_tensor,
                                 tensor_to_surfaces, detect_select, mask_paint, semantic_paint, pose_paint, kpt_decode)}


# ---- the inputs ----------------------------------------------------------------------------------------------------------
def put(base, i, v):
    """the tuple `base` with element i replaced"""
    return base[:i] + (v,) + base[i + 1:]


def dst_faults(even):
    """every single fault of a vali_tensor_dst"""
    f = [dict(data=0), dict(dtype=-1), dict(dtype=3), dict(packed=2), dict(n=0), dict(n=65536), dict(w=0), dict(h=0),
         dict(sn=0), dict(sn=-1), dict(sc=0), dict(sc=-1), dict(sy=0), dict(sy=-1), dict(sy=15), dict(packed=1, sy=47),
         dict(data=0x8001), dict(dtype=0, data=0x8001), dict(dtype=0, data=0x8002),
         dict(dtype=0, sy=2 ** 29), dict(sy=2 ** 30),                    # a row pitch of 2 GiB
         dict(dtype=0, sy=16384, h=65536), dict(sy=32768, h=65536)]      # a plane of 4 GiB
    if even:
        f += [dict(w=15), dict(h=15), dict(w=1, h=1)]
    return f


# two faults at once: the first of the rule's order is the one reported
DST_PAIRS = [dict(data=0, dtype=3), dict(dtype=3, packed=2), dict(packed=2, n=0), dict(n=0, w=0), dict(w=0, sn=0),
             dict(sc=0, sy=15), dict(sy=15, data=0x8001), dict(data=0x8001, sy=2 ** 30)]


def src_faults():
    """every single fault of a vali_tensor_src and its scale / offset"""
    return [dict(data=0), dict(dtype=-1), dict(dtype=4), dict(packed=2), dict(n=0), dict(n=65536), dict(w=0), dict(h=0),
            dict(w=65536, sy=65536), dict(h=65536), dict(sn=0), dict(sn=-1), dict(sc=0), dict(sc=-1), dict(sy=0), dict(sy=-1),
            dict(sy=15), dict(packed=1, sy=47), dict(data=0x8001), dict(dtype=0, data=0x8001), dict(dtype=0, data=0x8002),
            dict(scale=(NAN, 1.0, 1.0)), dict(scale=(1.0, INF, 1.0)), dict(scale=(1.0, 1.0, -INF)),
            dict(offset=(NAN, 0.0, 0.0)), dict(offset=(0.0, -INF, 0.0)), dict(offset=(0.0, 0.0, INF))]


SRC_PAIRS = [dict(data=0, dtype=4), dict(dtype=4, packed=2), dict(packed=2, n=0), dict(n=0, w=0), dict(w=0, sn=0),
             dict(sc=0, sy=15), dict(sy=15, data=0x8001), dict(data=0x8001, scale=(NAN, 1.0, 1.0)),
             dict(scale=(1.0, INF, 1.0), offset=(NAN, 0.0, 0.0))]


def head_faults(name, base):
    """every single fault of a head tensor (pointer, dtype, strides ...) passed as the argument `name`"""
    f = [put(base, 0, 0), put(base, 1, -1), put(base, 1, 3), put(put(base, 1, 1), 0, base[0] + 1),
         put(put(base, 1, 0), 0, base[0] + 1), put(put(base, 1, 0), 0, base[0] + 2)]
    for i in range(2, len(base)):
        f += [put(base, i, -1), put(base, i, BIG)]
    return [{name: t} for t in f]


def head_pairs(name, base):
    """null before dtype before alignment before strides"""
    return [{name: t} for t in (put(put(base, 0, 0), 1, 3), put(put(base, 1, 3), 0, base[0] + 1),
                                put(put(put(base, 1, 0), 0, base[0] + 2), 2, -1), put(put(base, 2, BIG), 3, -1))]


KPTS, BOXES, SCORES = (0x2000, 1, 1000, 15, 3, 1), (0x2000, 1, 4000, 4, 1), (0x3000, 1, 8000, 8, 1)
PROTOS, COEFFS, LOGITS = (0x2000, 1, 100, 10, 1), (0x3000, 0, 100, 10, 1), (0x2000, 1, 100, 10, 16)
HEAT, SIMCC = (0x2000, 4000, 800, 20), (0x2000, 4000, 800, 0x3000, 4000, 800)
NO_HEAT = (0, 0, 0, 0)


def cases():
    c = []
    add = lambda entry, kws: c.extend((entry, kw) for kw in kws)
    add("nv12_preproc_roi_tensor", dst_faults(True) + DST_PAIRS)
    add("rgb_preproc_roi_tensor", dst_faults(False) + DST_PAIRS + [dict(src_format=NV12, data=0)])
    add("warp_tensor", dst_faults(False) + DST_PAIRS + [dict(plane=0, data=0), dict(data=0, mats=0x6002), dict(sy=2 ** 30, mats=0x6002)])
    add("warp_fit", head_faults("kpts", KPTS) + head_pairs("kpts", KPTS))
    add("warp_fit", [dict(tmpl=0), dict(kpts=put(KPTS, 0, 0), tmpl=0), dict(tmpl=0, kpts=put(KPTS, 1, 3)),
                     dict(tmpl=0, kpts=put(KPTS, 0, 0x2001)), dict(mp=1, kpts=put(KPTS, 0, 0)),
                     dict(kpts=put(KPTS, 5, -1), thr=NAN), dict(kpts=put(KPTS, 2, BIG), tmpl=0x3002)])
    add("jpeg_encode_tensor", src_faults() + SRC_PAIRS)
    add("jpeg_encode_tensor", [dict(ws=0, data=0), dict(data=0, fmt=YUV420), dict(dtype=0, data=0x8002, fmt=YUV420),
                               dict(offset=(0.0, 0.0, INF), fmt=YUV420)])
    add("tensor_to_surfaces", src_faults() + SRC_PAIRS)
    add("tensor_to_surfaces", [dict(dst_format=Y, data=0), dict(params=False, data=0), dict(data=0, bgr=2),
                               dict(scale=(1.0, 1.0, -INF), bgr=2), dict(sy=15, w=15), dict(offset=(NAN, 0.0, 0.0), w=15, h=15)])
    for name, base in (("boxes", BOXES), ("scores", SCORES)):
        add("detect_select", head_faults(name, base) + head_pairs(name, base))
    add("detect_select", [dict(c=0, boxes=put(BOXES, 0, 0)), dict(boxes=put(BOXES, 1, 3), scores=put(SCORES, 0, 0)),
                          dict(boxes=put(BOXES, 4, -1), scores=put(SCORES, 1, -1)), dict(scores=put(SCORES, 3, BIG), T=0)])
    for name, base in (("protos", PROTOS), ("coeffs", COEFFS)):
        add("mask_paint", head_faults(name, base) + head_pairs(name, base))
    add("mask_paint", [dict(net_w=0, protos=put(PROTOS, 0, 0)), dict(protos=put(PROTOS, 2, -1), coeffs=put(COEFFS, 0, 0)),
                       dict(coeffs=put(COEFFS, 4, BIG), nc=0)])
    add("semantic_paint", head_faults("logits", LOGITS) + head_pairs("logits", LOGITS))
    add("semantic_paint", [dict(net_w=0, logits=put(LOGITS, 0, 0)), dict(net_w=0, logits=put(LOGITS, 1, 3)),
                           dict(logits=put(LOGITS, 0, 0x2001), nc=0), dict(logits=put(LOGITS, 4, -1), nc=0)])
    add("pose_paint", head_faults("kpts", KPTS) + head_pairs("kpts", KPTS))
    add("pose_paint", [dict(limbs=0, kpts=put(KPTS, 0, 0)), dict(kpts=put(KPTS, 5, BIG), lc=0)])
    # vali_kpt_decode: one dtype for the heatmaps or the two SimCC vectors, its own words
    k = [dict(heat=NO_HEAT), dict(simcc=SIMCC), dict(dtype=-1), dict(dtype=3), dict(heat=put(HEAT, 0, 0x2001)),
         dict(dtype=0, heat=put(HEAT, 0, 0x2001)), dict(dtype=0, heat=put(HEAT, 0, 0x2002))]
    for i in (1, 2, 3):
        k += [dict(heat=put(HEAT, i, -1)), dict(heat=put(HEAT, i, BIG))]
    k += [dict(heat=NO_HEAT, simcc=put(SIMCC, 0, 0)), dict(heat=NO_HEAT, simcc=put(SIMCC, 3, 0)),
          dict(heat=NO_HEAT, simcc=put(SIMCC, 0, 0x2001)), dict(heat=NO_HEAT, simcc=put(SIMCC, 3, 0x3001)),
          dict(heat=NO_HEAT, dtype=0, simcc=put(SIMCC, 0, 0x2002)), dict(heat=NO_HEAT, dtype=0, simcc=put(SIMCC, 3, 0x3002))]
    for i in (1, 2, 4, 5):
        k += [dict(heat=NO_HEAT, simcc=put(SIMCC, i, -1)), dict(heat=NO_HEAT, simcc=put(SIMCC, i, BIG))]
    k += [dict(simcc=SIMCC, dtype=3), dict(dtype=3, m=0), dict(m=0, heat=put(HEAT, 0, 0x2001)),
          dict(heat=put(put(HEAT, 0, 0x2001), 1, -1)), dict(heat=put(HEAT, 3, BIG), d_frames=0x1002),
          dict(heat=NO_HEAT, simcc=put(put(SIMCC, 3, 0x3001), 5, -1)), dict(heat=NO_HEAT, simcc=put(SIMCC, 4, BIG), d_frames=0x1002)]
    add("kpt_decode", k)
    return c


def key(entry, kw):
    return entry + " " + ", ".join(f"{k}={kw[k]!r}" for k in sorted(kw))


CASES = cases()


def test_every_entry_point_that_takes_a_tensor_is_covered():
    assert {e for e, _ in CASES} == set(ENTRY) and len(ENTRY) == 11
    keys = [key(e, kw) for e, kw in CASES]
    assert len(set(keys)) == len(keys) and set(keys) == set(EXPECTED)


@pytest.mark.parametrize("entry", sorted(ENTRY))
def test_the_first_refusal_is_the_recorded_one(vali, entry):
    """the code and the whole text, for every input of this entry point"""
    s = shim()
    assert (Y, RGB, NV12, YUV420) == (int(vali.Y), int(vali.RGB), int(vali.NV12), int(vali.YUV420))
    mine = [(e, kw) for e, kw in CASES if e == entry]
    assert len(mine) >= 20
    for e, kw in mine:
        want = EXPECTED[key(e, kw)]
        assert want[0] in (s.ERR_INVALID_ARG, s.ERR_UNSUPPORTED), (kw, want)       # never an input that would reach a device
        rc = ENTRY[e](**dict(kw))
        assert (rc, s.last_error()) == want, (e, kw)


# ---- the refusals, as the library words them -------------------------------------------------------------------------------
EXPECTED = {
    'nv12_preproc_roi_tensor data=0': (-1, 'vali_nv12_preproc_roi_tensor: null tensor data'),
    'nv12_preproc_roi_tensor dtype=-1': (-1, 'vali_nv12_preproc_roi_tensor: dtype must be VALI_DTYPE_F32, _F16 or _BF16'),
    'nv12_preproc_roi_tensor dtype=3': (-1, 'vali_nv12_preproc_roi_tensor: dtype must be VALI_DTYPE_F32, _F16 or _BF16'),
    'nv12_preproc_roi_tensor packed=2': (-1, 'vali_nv12_preproc_roi_tensor: packed must be 0 or 1'),
    'nv12_preproc_roi_tensor n=0': (-1, 'vali_nv12_preproc_roi_tensor: batch size out of range (1..65535)'),
    'nv12_preproc_roi_tensor n=65536': (-1, 'vali_nv12_preproc_roi_tensor: batch size out of range (1..65535)'),
    'nv12_preproc_roi_tensor w=0': (-1, 'vali_nv12_preproc_roi_tensor: bad geometry'),
    'nv12_preproc_roi_tensor h=0': (-1, 'vali_nv12_preproc_roi_tensor: bad geometry'),
    'nv12_preproc_roi_tensor sn=0': (-1, 'vali_nv12_preproc_roi_tensor: strides must be positive'),
    'nv12_preproc_roi_tensor sn=-1': (-1, 'vali_nv12_preproc_roi_tensor: strides must be positive'),
    'nv12_preproc_roi_tensor sc=0': (-1, 'vali_nv12_preproc_roi_tensor: strides must be positive'),
    'nv12_preproc_roi_tensor sc=-1': (-1, 'vali_nv12_preproc_roi_tensor: strides must be positive'),
    'nv12_preproc_roi_tensor sy=0': (-1, 'vali_nv12_preproc_roi_tensor: strides must be positive'),
    'nv12_preproc_roi_tensor sy=-1': (-1, 'vali_nv12_preproc_roi_tensor: strides must be positive'),
    'nv12_preproc_roi_tensor sy=15': (-1, 'vali_nv12_preproc_roi_tensor: stride_y is shorter than a row'),
    'nv12_preproc_roi_tensor packed=1, sy=47': (-1, 'vali_nv12_preproc_roi_tensor: stride_y is shorter than a row'),
    'nv12_preproc_roi_tensor data=32769': (-1, 'vali_nv12_preproc_roi_tensor: data is not aligned to its element'),
    'nv12_preproc_roi_tensor data=32769, dtype=0': (-1, 'vali_nv12_preproc_roi_tensor: data is not aligned to its element'),
    'nv12_preproc_roi_tensor data=32770, dtype=0': (-1, 'vali_nv12_preproc_roi_tensor: data is not aligned to its element'),
    'nv12_preproc_roi_tensor dtype=0, sy=536870912': (-1, 'vali_nv12_preproc_roi_tensor: row pitch of 2 GiB or plane of 4 GiB or more'),
    'nv12_preproc_roi_tensor sy=1073741824': (-1, 'vali_nv12_preproc_roi_tensor: row pitch of 2 GiB or plane of 4 GiB or more'),
    'nv12_preproc_roi_tensor dtype=0, h=65536, sy=16384': (-1, 'vali_nv12_preproc_roi_tensor: row pitch of 2 GiB or plane of 4 GiB or more'),
    'nv12_preproc_roi_tensor h=65536, sy=32768': (-1, 'vali_nv12_preproc_roi_tensor: row pitch of 2 GiB or plane of 4 GiB or more'),
    'nv12_preproc_roi_tensor w=15': (-1, 'vali_nv12_preproc_roi_tensor: bad geometry'),
    'nv12_preproc_roi_tensor h=15': (-1, 'vali_nv12_preproc_roi_tensor: bad geometry'),
    'nv12_preproc_roi_tensor h=1, w=1': (-1, 'vali_nv12_preproc_roi_tensor: bad geometry'),
    'nv12_preproc_roi_tensor data=0, dtype=3': (-1, 'vali_nv12_preproc_roi_tensor: null tensor data'),
    'nv12_preproc_roi_tensor dtype=3, packed=2': (-1, 'vali_nv12_preproc_roi_tensor: dtype must be VALI_DTYPE_F32, _F16 or _BF16'),
    'nv12_preproc_roi_tensor n=0, packed=2': (-1, 'vali_nv12_preproc_roi_tensor: packed must be 0 or 1'),
    'nv12_preproc_roi_tensor n=0, w=0': (-1, 'vali_nv12_preproc_roi_tensor: batch size out of range (1..65535)'),
    'nv12_preproc_roi_tensor sn=0, w=0': (-1, 'vali_nv12_preproc_roi_tensor: bad geometry'),
    'nv12_preproc_roi_tensor sc=0, sy=15': (-1, 'vali_nv12_preproc_roi_tensor: strides must be positive'),
    'nv12_preproc_roi_tensor data=32769, sy=15': (-1, 'vali_nv12_preproc_roi_tensor: stride_y is shorter than a row'),
    'nv12_preproc_roi_tensor data=32769, sy=1073741824': (-1, 'vali_nv12_preproc_roi_tensor: data is not aligned to its element'),
    'rgb_preproc_roi_tensor data=0': (-1, 'vali_rgb_preproc_roi_tensor: null tensor data'),
    'rgb_preproc_roi_tensor dtype=-1': (-1, 'vali_rgb_preproc_roi_tensor: dtype must be VALI_DTYPE_F32, _F16 or _BF16'),
    'rgb_preproc_roi_tensor dtype=3': (-1, 'vali_rgb_preproc_roi_tensor: dtype must be VALI_DTYPE_F32, _F16 or _BF16'),
    'rgb_preproc_roi_tensor packed=2': (-1, 'vali_rgb_preproc_roi_tensor: packed must be 0 or 1'),
    'rgb_preproc_roi_tensor n=0': (-1, 'vali_rgb_preproc_roi_tensor: batch size out of range (1..65535)'),
    'rgb_preproc_roi_tensor n=65536': (-1, 'vali_rgb_preproc_roi_tensor: batch size out of range (1..65535)'),
    'rgb_preproc_roi_tensor w=0': (-1, 'vali_rgb_preproc_roi_tensor: bad geometry'),
    'rgb_preproc_roi_tensor h=0': (-1, 'vali_rgb_preproc_roi_tensor: bad geometry'),
    'rgb_preproc_roi_tensor sn=0': (-1, 'vali_rgb_preproc_roi_tensor: strides must be positive'),
    'rgb_preproc_roi_tensor sn=-1': (-1, 'vali_rgb_preproc_roi_tensor: strides must be positive'),
    'rgb_preproc_roi_tensor sc=0': (-1, 'vali_rgb_preproc_roi_tensor: strides must be positive'),
    'rgb_preproc_roi_tensor sc=-1': (-1, 'vali_rgb_preproc_roi_tensor: strides must be positive'),
    'rgb_preproc_roi_tensor sy=0': (-1, 'vali_rgb_preproc_roi_tensor: strides must be positive'),
    'rgb_preproc_roi_tensor sy=-1': (-1, 'vali_rgb_preproc_roi_tensor: strides must be positive'),
    'rgb_preproc_roi_tensor sy=15': (-1, 'vali_rgb_preproc_roi_tensor: stride_y is shorter than a row'),
    'rgb_preproc_roi_tensor packed=1, sy=47': (-1, 'vali_rgb_preproc_roi_tensor: stride_y is shorter than a row'),
    'rgb_preproc_roi_tensor data=32769': (-1, 'vali_rgb_preproc_roi_tensor: data is not aligned to its element'),
    'rgb_preproc_roi_tensor data=32769, dtype=0': (-1, 'vali_rgb_preproc_roi_tensor: data is not aligned to its element'),
    'rgb_preproc_roi_tensor data=32770, dtype=0': (-1, 'vali_rgb_preproc_roi_tensor: data is not aligned to its element'),
    'rgb_preproc_roi_tensor dtype=0, sy=536870912': (-1, 'vali_rgb_preproc_roi_tensor: row pitch of 2 GiB or plane of 4 GiB or more'),
    'rgb_preproc_roi_tensor sy=1073741824': (-1, 'vali_rgb_preproc_roi_tensor: row pitch of 2 GiB or plane of 4 GiB or more'),
    'rgb_preproc_roi_tensor dtype=0, h=65536, sy=16384': (-1, 'vali_rgb_preproc_roi_tensor: row pitch of 2 GiB or plane of 4 GiB or more'),
    'rgb_preproc_roi_tensor h=65536, sy=32768': (-1, 'vali_rgb_preproc_roi_tensor: row pitch of 2 GiB or plane of 4 GiB or more'),
    'rgb_preproc_roi_tensor data=0, dtype=3': (-1, 'vali_rgb_preproc_roi_tensor: null tensor data'),
    'rgb_preproc_roi_tensor dtype=3, packed=2': (-1, 'vali_rgb_preproc_roi_tensor: dtype must be VALI_DTYPE_F32, _F16 or _BF16'),
    'rgb_preproc_roi_tensor n=0, packed=2': (-1, 'vali_rgb_preproc_roi_tensor: packed must be 0 or 1'),
    'rgb_preproc_roi_tensor n=0, w=0': (-1, 'vali_rgb_preproc_roi_tensor: batch size out of range (1..65535)'),
    'rgb_preproc_roi_tensor sn=0, w=0': (-1, 'vali_rgb_preproc_roi_tensor: bad geometry'),
    'rgb_preproc_roi_tensor sc=0, sy=15': (-1, 'vali_rgb_preproc_roi_tensor: strides must be positive'),
    'rgb_preproc_roi_tensor data=32769, sy=15': (-1, 'vali_rgb_preproc_roi_tensor: stride_y is shorter than a row'),
    'rgb_preproc_roi_tensor data=32769, sy=1073741824': (-1, 'vali_rgb_preproc_roi_tensor: data is not aligned to its element'),
    'rgb_preproc_roi_tensor data=0, src_format=3': (-2, 'rgb_preproc_roi_tensor: sources must be RGB, BGR or RGB_PLANAR (got 3)'),
    'warp_tensor data=0': (-1, 'vali_warp_tensor: null tensor data'),
    'warp_tensor dtype=-1': (-1, 'vali_warp_tensor: dtype must be VALI_DTYPE_F32, _F16 or _BF16'),
    'warp_tensor dtype=3': (-1, 'vali_warp_tensor: dtype must be VALI_DTYPE_F32, _F16 or _BF16'),
    'warp_tensor packed=2': (-1, 'vali_warp_tensor: packed must be 0 or 1'),
    'warp_tensor n=0': (-1, 'vali_warp_tensor: batch size out of range (1..65535)'),
    'warp_tensor n=65536': (-1, 'vali_warp_tensor: batch size out of range (1..65535)'),
    'warp_tensor w=0': (-1, 'vali_warp_tensor: bad geometry'),
    'warp_tensor h=0': (-1, 'vali_warp_tensor: bad geometry'),
    'warp_tensor sn=0': (-1, 'vali_warp_tensor: strides must be positive'),
    'warp_tensor sn=-1': (-1, 'vali_warp_tensor: strides must be positive'),
    'warp_tensor sc=0': (-1, 'vali_warp_tensor: strides must be positive'),
    'warp_tensor sc=-1': (-1, 'vali_warp_tensor: strides must be positive'),
    'warp_tensor sy=0': (-1, 'vali_warp_tensor: strides must be positive'),
    'warp_tensor sy=-1': (-1, 'vali_warp_tensor: strides must be positive'),
    'warp_tensor sy=15': (-1, 'vali_warp_tensor: stride_y is shorter than a row'),
    'warp_tensor packed=1, sy=47': (-1, 'vali_warp_tensor: stride_y is shorter than a row'),
    'warp_tensor data=32769': (-1, 'vali_warp_tensor: data is not aligned to its element'),
    'warp_tensor data=32769, dtype=0': (-1, 'vali_warp_tensor: data is not aligned to its element'),
    'warp_tensor data=32770, dtype=0': (-1, 'vali_warp_tensor: data is not aligned to its element'),
    'warp_tensor dtype=0, sy=536870912': (-1, 'vali_warp_tensor: row pitch of 2 GiB or plane of 4 GiB or more'),
    'warp_tensor sy=1073741824': (-1, 'vali_warp_tensor: row pitch of 2 GiB or plane of 4 GiB or more'),
    'warp_tensor dtype=0, h=65536, sy=16384': (-1, 'vali_warp_tensor: row pitch of 2 GiB or plane of 4 GiB or more'),
    'warp_tensor h=65536, sy=32768': (-1, 'vali_warp_tensor: row pitch of 2 GiB or plane of 4 GiB or more'),
    'warp_tensor data=0, dtype=3': (-1, 'vali_warp_tensor: null tensor data'),
    'warp_tensor dtype=3, packed=2': (-1, 'vali_warp_tensor: dtype must be VALI_DTYPE_F32, _F16 or _BF16'),
    'warp_tensor n=0, packed=2': (-1, 'vali_warp_tensor: packed must be 0 or 1'),
    'warp_tensor n=0, w=0': (-1, 'vali_warp_tensor: batch size out of range (1..65535)'),
    'warp_tensor sn=0, w=0': (-1, 'vali_warp_tensor: bad geometry'),
    'warp_tensor sc=0, sy=15': (-1, 'vali_warp_tensor: strides must be positive'),
    'warp_tensor data=32769, sy=15': (-1, 'vali_warp_tensor: stride_y is shorter than a row'),
    'warp_tensor data=32769, sy=1073741824': (-1, 'vali_warp_tensor: data is not aligned to its element'),
    'warp_tensor data=0, plane=0': (-1, 'vali_warp_tensor: frame 0: plane 0 is null'),
    'warp_tensor data=0, mats=24578': (-1, 'vali_warp_tensor: null tensor data'),
    'warp_tensor mats=24578, sy=1073741824': (-1, 'vali_warp_tensor: row pitch of 2 GiB or plane of 4 GiB or more'),
    'warp_fit kpts=(0, 1, 1000, 15, 3, 1)': (-1, 'vali_warp_fit: kpts has a null pointer'),
    'warp_fit kpts=(8192, -1, 1000, 15, 3, 1)': (-1, 'vali_warp_fit: kpts: dtype -1 is not float32, float16 or bfloat16'),
    'warp_fit kpts=(8192, 3, 1000, 15, 3, 1)': (-1, 'vali_warp_fit: kpts: dtype 3 is not float32, float16 or bfloat16'),
    'warp_fit kpts=(8193, 1, 1000, 15, 3, 1)': (-1, 'vali_warp_fit: kpts is not aligned to its element size'),
    'warp_fit kpts=(8193, 0, 1000, 15, 3, 1)': (-1, 'vali_warp_fit: kpts is not aligned to its element size'),
    'warp_fit kpts=(8194, 0, 1000, 15, 3, 1)': (-1, 'vali_warp_fit: kpts is not aligned to its element size'),
    'warp_fit kpts=(8192, 1, -1, 15, 3, 1)': (-1, 'vali_warp_fit: kpts: strides (-1, 15, 3, 1) outside 0..2^40'),
    'warp_fit kpts=(8192, 1, 1099511627777, 15, 3, 1)': (-1, 'vali_warp_fit: kpts: strides (1099511627777, 15, 3, 1) outside 0..2^40'),
    'warp_fit kpts=(8192, 1, 1000, -1, 3, 1)': (-1, 'vali_warp_fit: kpts: strides (1000, -1, 3, 1) outside 0..2^40'),
    'warp_fit kpts=(8192, 1, 1000, 1099511627777, 3, 1)': (-1, 'vali_warp_fit: kpts: strides (1000, 1099511627777, 3, 1) outside 0..2^40'),
    'warp_fit kpts=(8192, 1, 1000, 15, -1, 1)': (-1, 'vali_warp_fit: kpts: strides (1000, 15, -1, 1) outside 0..2^40'),
    'warp_fit kpts=(8192, 1, 1000, 15, 1099511627777, 1)': (-1, 'vali_warp_fit: kpts: strides (1000, 15, 1099511627777, 1) outside 0..2^40'),
    'warp_fit kpts=(8192, 1, 1000, 15, 3, -1)': (-1, 'vali_warp_fit: kpts: strides (1000, 15, 3, -1) outside 0..2^40'),
    'warp_fit kpts=(8192, 1, 1000, 15, 3, 1099511627777)': (-1, 'vali_warp_fit: kpts: strides (1000, 15, 3, 1099511627777) outside 0..2^40'),
    'warp_fit kpts=(0, 3, 1000, 15, 3, 1)': (-1, 'vali_warp_fit: kpts has a null pointer'),
    'warp_fit kpts=(8193, 3, 1000, 15, 3, 1)': (-1, 'vali_warp_fit: kpts: dtype 3 is not float32, float16 or bfloat16'),
    'warp_fit kpts=(8194, 0, -1, 15, 3, 1)': (-1, 'vali_warp_fit: kpts is not aligned to its element size'),
    'warp_fit kpts=(8192, 1, 1099511627777, -1, 3, 1)': (-1, 'vali_warp_fit: kpts: strides (1099511627777, -1, 3, 1) outside 0..2^40'),
    'warp_fit tmpl=0': (-1, 'vali_warp_fit: template has a null pointer'),
    'warp_fit kpts=(0, 1, 1000, 15, 3, 1), tmpl=0': (-1, 'vali_warp_fit: kpts has a null pointer'),
    'warp_fit kpts=(8192, 3, 1000, 15, 3, 1), tmpl=0': (-1, 'vali_warp_fit: template has a null pointer'),
    'warp_fit kpts=(8193, 1, 1000, 15, 3, 1), tmpl=0': (-1, 'vali_warp_fit: template has a null pointer'),
    'warp_fit kpts=(0, 1, 1000, 15, 3, 1), mp=1': (-1, 'vali_warp_fit: min_points outside 2..p'),
    'warp_fit kpts=(8192, 1, 1000, 15, 3, -1), thr=nan': (-1, 'vali_warp_fit: kpts: strides (1000, 15, 3, -1) outside 0..2^40'),
    'warp_fit kpts=(8192, 1, 1099511627777, 15, 3, 1), tmpl=12290': (-1, 'vali_warp_fit: kpts: strides (1099511627777, 15, 3, 1) outside 0..2^40'),
    'jpeg_encode_tensor data=0': (-1, 'vali_jpeg_encode_tensor: null tensor data'),
    'jpeg_encode_tensor dtype=-1': (-1, 'vali_jpeg_encode_tensor: dtype must be VALI_DTYPE_F32, _F16, _BF16 or _U8'),
    'jpeg_encode_tensor dtype=4': (-1, 'vali_jpeg_encode_tensor: dtype must be VALI_DTYPE_F32, _F16, _BF16 or _U8'),
    'jpeg_encode_tensor packed=2': (-1, 'vali_jpeg_encode_tensor: packed must be 0 or 1'),
    'jpeg_encode_tensor n=0': (-1, 'vali_jpeg_encode_tensor: batch size out of range (1..65535)'),
    'jpeg_encode_tensor n=65536': (-1, 'vali_jpeg_encode_tensor: batch size out of range (1..65535)'),
    'jpeg_encode_tensor w=0': (-1, 'vali_jpeg_encode_tensor: size outside 1..65535'),
    'jpeg_encode_tensor h=0': (-1, 'vali_jpeg_encode_tensor: size outside 1..65535'),
    'jpeg_encode_tensor sy=65536, w=65536': (-1, 'vali_jpeg_encode_tensor: size outside 1..65535'),
    'jpeg_encode_tensor h=65536': (-1, 'vali_jpeg_encode_tensor: size outside 1..65535'),
    'jpeg_encode_tensor sn=0': (-1, 'vali_jpeg_encode_tensor: strides must be positive'),
    'jpeg_encode_tensor sn=-1': (-1, 'vali_jpeg_encode_tensor: strides must be positive'),
    'jpeg_encode_tensor sc=0': (-1, 'vali_jpeg_encode_tensor: strides must be positive'),
    'jpeg_encode_tensor sc=-1': (-1, 'vali_jpeg_encode_tensor: strides must be positive'),
    'jpeg_encode_tensor sy=0': (-1, 'vali_jpeg_encode_tensor: strides must be positive'),
    'jpeg_encode_tensor sy=-1': (-1, 'vali_jpeg_encode_tensor: strides must be positive'),
    'jpeg_encode_tensor sy=15': (-1, 'vali_jpeg_encode_tensor: stride_y is shorter than a row'),
    'jpeg_encode_tensor packed=1, sy=47': (-1, 'vali_jpeg_encode_tensor: stride_y is shorter than a row'),
    'jpeg_encode_tensor data=32769': (-1, 'vali_jpeg_encode_tensor: data is not aligned to its element'),
    'jpeg_encode_tensor data=32769, dtype=0': (-1, 'vali_jpeg_encode_tensor: data is not aligned to its element'),
    'jpeg_encode_tensor data=32770, dtype=0': (-1, 'vali_jpeg_encode_tensor: data is not aligned to its element'),
    'jpeg_encode_tensor scale=(nan, 1.0, 1.0)': (-1, 'vali_jpeg_encode_tensor: scale and offset must be finite'),
    'jpeg_encode_tensor scale=(1.0, inf, 1.0)': (-1, 'vali_jpeg_encode_tensor: scale and offset must be finite'),
    'jpeg_encode_tensor scale=(1.0, 1.0, -inf)': (-1, 'vali_jpeg_encode_tensor: scale and offset must be finite'),
    'jpeg_encode_tensor offset=(nan, 0.0, 0.0)': (-1, 'vali_jpeg_encode_tensor: scale and offset must be finite'),
    'jpeg_encode_tensor offset=(0.0, -inf, 0.0)': (-1, 'vali_jpeg_encode_tensor: scale and offset must be finite'),
    'jpeg_encode_tensor offset=(0.0, 0.0, inf)': (-1, 'vali_jpeg_encode_tensor: scale and offset must be finite'),
    'jpeg_encode_tensor data=0, dtype=4': (-1, 'vali_jpeg_encode_tensor: null tensor data'),
    'jpeg_encode_tensor dtype=4, packed=2': (-1, 'vali_jpeg_encode_tensor: dtype must be VALI_DTYPE_F32, _F16, _BF16 or _U8'),
    'jpeg_encode_tensor n=0, packed=2': (-1, 'vali_jpeg_encode_tensor: packed must be 0 or 1'),
    'jpeg_encode_tensor n=0, w=0': (-1, 'vali_jpeg_encode_tensor: batch size out of range (1..65535)'),
    'jpeg_encode_tensor sn=0, w=0': (-1, 'vali_jpeg_encode_tensor: size outside 1..65535'),
    'jpeg_encode_tensor sc=0, sy=15': (-1, 'vali_jpeg_encode_tensor: strides must be positive'),
    'jpeg_encode_tensor data=32769, sy=15': (-1, 'vali_jpeg_encode_tensor: stride_y is shorter than a row'),
    'jpeg_encode_tensor data=32769, scale=(nan, 1.0, 1.0)': (-1, 'vali_jpeg_encode_tensor: data is not aligned to its element'),
    'jpeg_encode_tensor offset=(nan, 0.0, 0.0), scale=(1.0, inf, 1.0)': (-1, 'vali_jpeg_encode_tensor: scale and offset must be finite'),
    'jpeg_encode_tensor data=0, ws=0': (-1, 'vali_jpeg_encode_tensor: null argument'),
    'jpeg_encode_tensor data=0, fmt=4': (-1, 'vali_jpeg_encode_tensor: null tensor data'),
    'jpeg_encode_tensor data=32770, dtype=0, fmt=4': (-1, 'vali_jpeg_encode_tensor: data is not aligned to its element'),
    'jpeg_encode_tensor fmt=4, offset=(0.0, 0.0, inf)': (-1, 'vali_jpeg_encode_tensor: scale and offset must be finite'),
    'tensor_to_surfaces data=0': (-1, 'vali_tensor_to_surfaces: null tensor data'),
    'tensor_to_surfaces dtype=-1': (-1, 'vali_tensor_to_surfaces: dtype must be VALI_DTYPE_F32, _F16, _BF16 or _U8'),
    'tensor_to_surfaces dtype=4': (-1, 'vali_tensor_to_surfaces: dtype must be VALI_DTYPE_F32, _F16, _BF16 or _U8'),
    'tensor_to_surfaces packed=2': (-1, 'vali_tensor_to_surfaces: packed must be 0 or 1'),
    'tensor_to_surfaces n=0': (-1, 'vali_tensor_to_surfaces: batch size out of range (1..65535)'),
    'tensor_to_surfaces n=65536': (-1, 'vali_tensor_to_surfaces: batch size out of range (1..65535)'),
    'tensor_to_surfaces w=0': (-1, 'vali_tensor_to_surfaces: size outside 1..65535'),
    'tensor_to_surfaces h=0': (-1, 'vali_tensor_to_surfaces: size outside 1..65535'),
    'tensor_to_surfaces sy=65536, w=65536': (-1, 'vali_tensor_to_surfaces: size outside 1..65535'),
    'tensor_to_surfaces h=65536': (-1, 'vali_tensor_to_surfaces: size outside 1..65535'),
    'tensor_to_surfaces sn=0': (-1, 'vali_tensor_to_surfaces: strides must be positive'),
    'tensor_to_surfaces sn=-1': (-1, 'vali_tensor_to_surfaces: strides must be positive'),
    'tensor_to_surfaces sc=0': (-1, 'vali_tensor_to_surfaces: strides must be positive'),
    'tensor_to_surfaces sc=-1': (-1, 'vali_tensor_to_surfaces: strides must be positive'),
    'tensor_to_surfaces sy=0': (-1, 'vali_tensor_to_surfaces: strides must be positive'),
    'tensor_to_surfaces sy=-1': (-1, 'vali_tensor_to_surfaces: strides must be positive'),
    'tensor_to_surfaces sy=15': (-1, 'vali_tensor_to_surfaces: stride_y is shorter than a row'),
    'tensor_to_surfaces packed=1, sy=47': (-1, 'vali_tensor_to_surfaces: stride_y is shorter than a row'),
    'tensor_to_surfaces data=32769': (-1, 'vali_tensor_to_surfaces: data is not aligned to its element'),
    'tensor_to_surfaces data=32769, dtype=0': (-1, 'vali_tensor_to_surfaces: data is not aligned to its element'),
    'tensor_to_surfaces data=32770, dtype=0': (-1, 'vali_tensor_to_surfaces: data is not aligned to its element'),
    'tensor_to_surfaces scale=(nan, 1.0, 1.0)': (-1, 'vali_tensor_to_surfaces: scale and offset must be finite'),
    'tensor_to_surfaces scale=(1.0, inf, 1.0)': (-1, 'vali_tensor_to_surfaces: scale and offset must be finite'),
    'tensor_to_surfaces scale=(1.0, 1.0, -inf)': (-1, 'vali_tensor_to_surfaces: scale and offset must be finite'),
    'tensor_to_surfaces offset=(nan, 0.0, 0.0)': (-1, 'vali_tensor_to_surfaces: scale and offset must be finite'),
    'tensor_to_surfaces offset=(0.0, -inf, 0.0)': (-1, 'vali_tensor_to_surfaces: scale and offset must be finite'),
    'tensor_to_surfaces offset=(0.0, 0.0, inf)': (-1, 'vali_tensor_to_surfaces: scale and offset must be finite'),
    'tensor_to_surfaces data=0, dtype=4': (-1, 'vali_tensor_to_surfaces: null tensor data'),
    'tensor_to_surfaces dtype=4, packed=2': (-1, 'vali_tensor_to_surfaces: dtype must be VALI_DTYPE_F32, _F16, _BF16 or _U8'),
    'tensor_to_surfaces n=0, packed=2': (-1, 'vali_tensor_to_surfaces: packed must be 0 or 1'),
    'tensor_to_surfaces n=0, w=0': (-1, 'vali_tensor_to_surfaces: batch size out of range (1..65535)'),
    'tensor_to_surfaces sn=0, w=0': (-1, 'vali_tensor_to_surfaces: size outside 1..65535'),
    'tensor_to_surfaces sc=0, sy=15': (-1, 'vali_tensor_to_surfaces: strides must be positive'),
    'tensor_to_surfaces data=32769, sy=15': (-1, 'vali_tensor_to_surfaces: stride_y is shorter than a row'),
    'tensor_to_surfaces data=32769, scale=(nan, 1.0, 1.0)': (-1, 'vali_tensor_to_surfaces: data is not aligned to its element'),
    'tensor_to_surfaces offset=(nan, 0.0, 0.0), scale=(1.0, inf, 1.0)': (-1, 'vali_tensor_to_surfaces: scale and offset must be finite'),
    'tensor_to_surfaces data=0, dst_format=1': (-2, 'vali_tensor_to_surfaces: destination format 1 (NV12, YUV420, YUV444, RGB, RGB_PLANAR)'),
    'tensor_to_surfaces data=0, params=False': (-1, 'vali_tensor_to_surfaces: a YUV destination needs params (rgb2yuv)'),
    'tensor_to_surfaces bgr=2, data=0': (-1, 'vali_tensor_to_surfaces: null tensor data'),
    'tensor_to_surfaces bgr=2, scale=(1.0, 1.0, -inf)': (-1, 'vali_tensor_to_surfaces: scale and offset must be finite'),
    'tensor_to_surfaces sy=15, w=15': (-1, 'vali_tensor_to_surfaces: 4:2:0 destinations (NV12, YUV420) need even width and height'),
    'tensor_to_surfaces h=15, offset=(nan, 0.0, 0.0), w=15': (-1, 'vali_tensor_to_surfaces: scale and offset must be finite'),
    'detect_select boxes=(0, 1, 4000, 4, 1)': (-1, 'vali_detect_select: boxes has a null pointer'),
    'detect_select boxes=(8192, -1, 4000, 4, 1)': (-1, 'vali_detect_select: boxes: dtype -1 is not float32, float16 or bfloat16'),
    'detect_select boxes=(8192, 3, 4000, 4, 1)': (-1, 'vali_detect_select: boxes: dtype 3 is not float32, float16 or bfloat16'),
    'detect_select boxes=(8193, 1, 4000, 4, 1)': (-1, 'vali_detect_select: boxes is not aligned to its element size'),
    'detect_select boxes=(8193, 0, 4000, 4, 1)': (-1, 'vali_detect_select: boxes is not aligned to its element size'),
    'detect_select boxes=(8194, 0, 4000, 4, 1)': (-1, 'vali_detect_select: boxes is not aligned to its element size'),
    'detect_select boxes=(8192, 1, -1, 4, 1)': (-1, 'vali_detect_select: boxes: strides (-1, 4, 1) outside 0..2^40'),
    'detect_select boxes=(8192, 1, 1099511627777, 4, 1)': (-1, 'vali_detect_select: boxes: strides (1099511627777, 4, 1) outside 0..2^40'),
    'detect_select boxes=(8192, 1, 4000, -1, 1)': (-1, 'vali_detect_select: boxes: strides (4000, -1, 1) outside 0..2^40'),
    'detect_select boxes=(8192, 1, 4000, 1099511627777, 1)': (-1, 'vali_detect_select: boxes: strides (4000, 1099511627777, 1) outside 0..2^40'),
    'detect_select boxes=(8192, 1, 4000, 4, -1)': (-1, 'vali_detect_select: boxes: strides (4000, 4, -1) outside 0..2^40'),
    'detect_select boxes=(8192, 1, 4000, 4, 1099511627777)': (-1, 'vali_detect_select: boxes: strides (4000, 4, 1099511627777) outside 0..2^40'),
    'detect_select boxes=(0, 3, 4000, 4, 1)': (-1, 'vali_detect_select: boxes has a null pointer'),
    'detect_select boxes=(8193, 3, 4000, 4, 1)': (-1, 'vali_detect_select: boxes: dtype 3 is not float32, float16 or bfloat16'),
    'detect_select boxes=(8194, 0, -1, 4, 1)': (-1, 'vali_detect_select: boxes is not aligned to its element size'),
    'detect_select boxes=(8192, 1, 1099511627777, -1, 1)': (-1, 'vali_detect_select: boxes: strides (1099511627777, -1, 1) outside 0..2^40'),
    'detect_select scores=(0, 1, 8000, 8, 1)': (-1, 'vali_detect_select: scores has a null pointer'),
    'detect_select scores=(12288, -1, 8000, 8, 1)': (-1, 'vali_detect_select: scores: dtype -1 is not float32, float16 or bfloat16'),
    'detect_select scores=(12288, 3, 8000, 8, 1)': (-1, 'vali_detect_select: scores: dtype 3 is not float32, float16 or bfloat16'),
    'detect_select scores=(12289, 1, 8000, 8, 1)': (-1, 'vali_detect_select: scores is not aligned to its element size'),
    'detect_select scores=(12289, 0, 8000, 8, 1)': (-1, 'vali_detect_select: scores is not aligned to its element size'),
    'detect_select scores=(12290, 0, 8000, 8, 1)': (-1, 'vali_detect_select: scores is not aligned to its element size'),
    'detect_select scores=(12288, 1, -1, 8, 1)': (-1, 'vali_detect_select: scores: strides (-1, 8, 1) outside 0..2^40'),
    'detect_select scores=(12288, 1, 1099511627777, 8, 1)': (-1, 'vali_detect_select: scores: strides (1099511627777, 8, 1) outside 0..2^40'),
    'detect_select scores=(12288, 1, 8000, -1, 1)': (-1, 'vali_detect_select: scores: strides (8000, -1, 1) outside 0..2^40'),
    'detect_select scores=(12288, 1, 8000, 1099511627777, 1)': (-1, 'vali_detect_select: scores: strides (8000, 1099511627777, 1) outside 0..2^40'),
    'detect_select scores=(12288, 1, 8000, 8, -1)': (-1, 'vali_detect_select: scores: strides (8000, 8, -1) outside 0..2^40'),
    'detect_select scores=(12288, 1, 8000, 8, 1099511627777)': (-1, 'vali_detect_select: scores: strides (8000, 8, 1099511627777) outside 0..2^40'),
    'detect_select scores=(0, 3, 8000, 8, 1)': (-1, 'vali_detect_select: scores has a null pointer'),
    'detect_select scores=(12289, 3, 8000, 8, 1)': (-1, 'vali_detect_select: scores: dtype 3 is not float32, float16 or bfloat16'),
    'detect_select scores=(12290, 0, -1, 8, 1)': (-1, 'vali_detect_select: scores is not aligned to its element size'),
    'detect_select scores=(12288, 1, 1099511627777, -1, 1)': (-1, 'vali_detect_select: scores: strides (1099511627777, -1, 1) outside 0..2^40'),
    'detect_select boxes=(0, 1, 4000, 4, 1), c=0': (-1, 'vali_detect_select: c outside 1..4096'),
    'detect_select boxes=(8192, 3, 4000, 4, 1), scores=(0, 1, 8000, 8, 1)': (-1, 'vali_detect_select: boxes: dtype 3 is not float32, float16 or bfloat16'),
    'detect_select boxes=(8192, 1, 4000, 4, -1), scores=(12288, -1, 8000, 8, 1)': (-1, 'vali_detect_select: boxes: strides (4000, 4, -1) outside 0..2^40'),
    'detect_select T=0, scores=(12288, 1, 8000, 1099511627777, 1)': (-1, 'vali_detect_select: scores: strides (8000, 1099511627777, 1) outside 0..2^40'),
    'mask_paint protos=(0, 1, 100, 10, 1)': (-1, 'vali_mask_paint: protos has a null pointer'),
    'mask_paint protos=(8192, -1, 100, 10, 1)': (-1, 'vali_mask_paint: protos: dtype -1 is not float32, float16 or bfloat16'),
    'mask_paint protos=(8192, 3, 100, 10, 1)': (-1, 'vali_mask_paint: protos: dtype 3 is not float32, float16 or bfloat16'),
    'mask_paint protos=(8193, 1, 100, 10, 1)': (-1, 'vali_mask_paint: protos is not aligned to its element size'),
    'mask_paint protos=(8193, 0, 100, 10, 1)': (-1, 'vali_mask_paint: protos is not aligned to its element size'),
    'mask_paint protos=(8194, 0, 100, 10, 1)': (-1, 'vali_mask_paint: protos is not aligned to its element size'),
    'mask_paint protos=(8192, 1, -1, 10, 1)': (-1, 'vali_mask_paint: protos: strides (-1, 10, 1) outside 0..2^40'),
    'mask_paint protos=(8192, 1, 1099511627777, 10, 1)': (-1, 'vali_mask_paint: protos: strides (1099511627777, 10, 1) outside 0..2^40'),
    'mask_paint protos=(8192, 1, 100, -1, 1)': (-1, 'vali_mask_paint: protos: strides (100, -1, 1) outside 0..2^40'),
    'mask_paint protos=(8192, 1, 100, 1099511627777, 1)': (-1, 'vali_mask_paint: protos: strides (100, 1099511627777, 1) outside 0..2^40'),
    'mask_paint protos=(8192, 1, 100, 10, -1)': (-1, 'vali_mask_paint: protos: strides (100, 10, -1) outside 0..2^40'),
    'mask_paint protos=(8192, 1, 100, 10, 1099511627777)': (-1, 'vali_mask_paint: protos: strides (100, 10, 1099511627777) outside 0..2^40'),
    'mask_paint protos=(0, 3, 100, 10, 1)': (-1, 'vali_mask_paint: protos has a null pointer'),
    'mask_paint protos=(8193, 3, 100, 10, 1)': (-1, 'vali_mask_paint: protos: dtype 3 is not float32, float16 or bfloat16'),
    'mask_paint protos=(8194, 0, -1, 10, 1)': (-1, 'vali_mask_paint: protos is not aligned to its element size'),
    'mask_paint protos=(8192, 1, 1099511627777, -1, 1)': (-1, 'vali_mask_paint: protos: strides (1099511627777, -1, 1) outside 0..2^40'),
    'mask_paint coeffs=(0, 0, 100, 10, 1)': (-1, 'vali_mask_paint: coeffs has a null pointer'),
    'mask_paint coeffs=(12288, -1, 100, 10, 1)': (-1, 'vali_mask_paint: coeffs: dtype -1 is not float32, float16 or bfloat16'),
    'mask_paint coeffs=(12288, 3, 100, 10, 1)': (-1, 'vali_mask_paint: coeffs: dtype 3 is not float32, float16 or bfloat16'),
    'mask_paint coeffs=(12289, 1, 100, 10, 1)': (-1, 'vali_mask_paint: coeffs is not aligned to its element size'),
    'mask_paint coeffs=(12289, 0, 100, 10, 1)': (-1, 'vali_mask_paint: coeffs is not aligned to its element size'),
    'mask_paint coeffs=(12290, 0, 100, 10, 1)': (-1, 'vali_mask_paint: coeffs is not aligned to its element size'),
    'mask_paint coeffs=(12288, 0, -1, 10, 1)': (-1, 'vali_mask_paint: coeffs: strides (-1, 10, 1) outside 0..2^40'),
    'mask_paint coeffs=(12288, 0, 1099511627777, 10, 1)': (-1, 'vali_mask_paint: coeffs: strides (1099511627777, 10, 1) outside 0..2^40'),
    'mask_paint coeffs=(12288, 0, 100, -1, 1)': (-1, 'vali_mask_paint: coeffs: strides (100, -1, 1) outside 0..2^40'),
    'mask_paint coeffs=(12288, 0, 100, 1099511627777, 1)': (-1, 'vali_mask_paint: coeffs: strides (100, 1099511627777, 1) outside 0..2^40'),
    'mask_paint coeffs=(12288, 0, 100, 10, -1)': (-1, 'vali_mask_paint: coeffs: strides (100, 10, -1) outside 0..2^40'),
    'mask_paint coeffs=(12288, 0, 100, 10, 1099511627777)': (-1, 'vali_mask_paint: coeffs: strides (100, 10, 1099511627777) outside 0..2^40'),
    'mask_paint coeffs=(0, 3, 100, 10, 1)': (-1, 'vali_mask_paint: coeffs has a null pointer'),
    'mask_paint coeffs=(12289, 3, 100, 10, 1)': (-1, 'vali_mask_paint: coeffs: dtype 3 is not float32, float16 or bfloat16'),
    'mask_paint coeffs=(12290, 0, -1, 10, 1)': (-1, 'vali_mask_paint: coeffs is not aligned to its element size'),
    'mask_paint coeffs=(12288, 0, 1099511627777, -1, 1)': (-1, 'vali_mask_paint: coeffs: strides (1099511627777, -1, 1) outside 0..2^40'),
    'mask_paint net_w=0, protos=(0, 1, 100, 10, 1)': (-1, 'vali_mask_paint: net_w or net_h outside 1..65535'),
    'mask_paint coeffs=(0, 0, 100, 10, 1), protos=(8192, 1, -1, 10, 1)': (-1, 'vali_mask_paint: protos: strides (-1, 10, 1) outside 0..2^40'),
    'mask_paint coeffs=(12288, 0, 100, 10, 1099511627777), nc=0': (-1, 'vali_mask_paint: coeffs: strides (100, 10, 1099511627777) outside 0..2^40'),
    'semantic_paint logits=(0, 1, 100, 10, 16)': (-1, 'vali_semantic_paint: logits has a null pointer'),
    'semantic_paint logits=(8192, -1, 100, 10, 16)': (-1, 'vali_semantic_paint: logits: dtype -1 is not float32, float16 or bfloat16'),
    'semantic_paint logits=(8192, 3, 100, 10, 16)': (-1, 'vali_semantic_paint: logits: dtype 3 is not float32, float16 or bfloat16'),
    'semantic_paint logits=(8193, 1, 100, 10, 16)': (-1, 'vali_semantic_paint: logits is not aligned to its element size'),
    'semantic_paint logits=(8193, 0, 100, 10, 16)': (-1, 'vali_semantic_paint: logits is not aligned to its element size'),
    'semantic_paint logits=(8194, 0, 100, 10, 16)': (-1, 'vali_semantic_paint: logits is not aligned to its element size'),
    'semantic_paint logits=(8192, 1, -1, 10, 16)': (-1, 'vali_semantic_paint: logits: strides (-1, 10, 16) outside 0..2^40'),
    'semantic_paint logits=(8192, 1, 1099511627777, 10, 16)': (-1, 'vali_semantic_paint: logits: strides (1099511627777, 10, 16) outside 0..2^40'),
    'semantic_paint logits=(8192, 1, 100, -1, 16)': (-1, 'vali_semantic_paint: logits: strides (100, -1, 16) outside 0..2^40'),
    'semantic_paint logits=(8192, 1, 100, 1099511627777, 16)': (-1, 'vali_semantic_paint: logits: strides (100, 1099511627777, 16) outside 0..2^40'),
    'semantic_paint logits=(8192, 1, 100, 10, -1)': (-1, 'vali_semantic_paint: logits: strides (100, 10, -1) outside 0..2^40'),
    'semantic_paint logits=(8192, 1, 100, 10, 1099511627777)': (-1, 'vali_semantic_paint: logits: strides (100, 10, 1099511627777) outside 0..2^40'),
    'semantic_paint logits=(0, 3, 100, 10, 16)': (-1, 'vali_semantic_paint: logits has a null pointer'),
    'semantic_paint logits=(8193, 3, 100, 10, 16)': (-1, 'vali_semantic_paint: logits: dtype 3 is not float32, float16 or bfloat16'),
    'semantic_paint logits=(8194, 0, -1, 10, 16)': (-1, 'vali_semantic_paint: logits is not aligned to its element size'),
    'semantic_paint logits=(8192, 1, 1099511627777, -1, 16)': (-1, 'vali_semantic_paint: logits: strides (1099511627777, -1, 16) outside 0..2^40'),
    'semantic_paint logits=(0, 1, 100, 10, 16), net_w=0': (-1, 'vali_semantic_paint: net_w or net_h outside 1..65535'),
    'semantic_paint logits=(8192, 3, 100, 10, 16), net_w=0': (-1, 'vali_semantic_paint: net_w or net_h outside 1..65535'),
    'semantic_paint logits=(8193, 1, 100, 10, 16), nc=0': (-1, 'vali_semantic_paint: logits is not aligned to its element size'),
    'semantic_paint logits=(8192, 1, 100, 10, -1), nc=0': (-1, 'vali_semantic_paint: logits: strides (100, 10, -1) outside 0..2^40'),
    'pose_paint kpts=(0, 1, 1000, 15, 3, 1)': (-1, 'vali_pose_paint: kpts has a null pointer'),
    'pose_paint kpts=(8192, -1, 1000, 15, 3, 1)': (-1, 'vali_pose_paint: kpts: dtype -1 is not float32, float16 or bfloat16'),
    'pose_paint kpts=(8192, 3, 1000, 15, 3, 1)': (-1, 'vali_pose_paint: kpts: dtype 3 is not float32, float16 or bfloat16'),
    'pose_paint kpts=(8193, 1, 1000, 15, 3, 1)': (-1, 'vali_pose_paint: kpts is not aligned to its element size'),
    'pose_paint kpts=(8193, 0, 1000, 15, 3, 1)': (-1, 'vali_pose_paint: kpts is not aligned to its element size'),
    'pose_paint kpts=(8194, 0, 1000, 15, 3, 1)': (-1, 'vali_pose_paint: kpts is not aligned to its element size'),
    'pose_paint kpts=(8192, 1, -1, 15, 3, 1)': (-1, 'vali_pose_paint: kpts: strides (-1, 15, 3, 1) outside 0..2^40'),
    'pose_paint kpts=(8192, 1, 1099511627777, 15, 3, 1)': (-1, 'vali_pose_paint: kpts: strides (1099511627777, 15, 3, 1) outside 0..2^40'),
    'pose_paint kpts=(8192, 1, 1000, -1, 3, 1)': (-1, 'vali_pose_paint: kpts: strides (1000, -1, 3, 1) outside 0..2^40'),
    'pose_paint kpts=(8192, 1, 1000, 1099511627777, 3, 1)': (-1, 'vali_pose_paint: kpts: strides (1000, 1099511627777, 3, 1) outside 0..2^40'),
    'pose_paint kpts=(8192, 1, 1000, 15, -1, 1)': (-1, 'vali_pose_paint: kpts: strides (1000, 15, -1, 1) outside 0..2^40'),
    'pose_paint kpts=(8192, 1, 1000, 15, 1099511627777, 1)': (-1, 'vali_pose_paint: kpts: strides (1000, 15, 1099511627777, 1) outside 0..2^40'),
    'pose_paint kpts=(8192, 1, 1000, 15, 3, -1)': (-1, 'vali_pose_paint: kpts: strides (1000, 15, 3, -1) outside 0..2^40'),
    'pose_paint kpts=(8192, 1, 1000, 15, 3, 1099511627777)': (-1, 'vali_pose_paint: kpts: strides (1000, 15, 3, 1099511627777) outside 0..2^40'),
    'pose_paint kpts=(0, 3, 1000, 15, 3, 1)': (-1, 'vali_pose_paint: kpts has a null pointer'),
    'pose_paint kpts=(8193, 3, 1000, 15, 3, 1)': (-1, 'vali_pose_paint: kpts: dtype 3 is not float32, float16 or bfloat16'),
    'pose_paint kpts=(8194, 0, -1, 15, 3, 1)': (-1, 'vali_pose_paint: kpts is not aligned to its element size'),
    'pose_paint kpts=(8192, 1, 1099511627777, -1, 3, 1)': (-1, 'vali_pose_paint: kpts: strides (1099511627777, -1, 3, 1) outside 0..2^40'),
    'pose_paint kpts=(0, 1, 1000, 15, 3, 1), limbs=0': (-1, 'vali_pose_paint: limbs has a null pointer'),
    'pose_paint kpts=(8192, 1, 1000, 15, 3, 1099511627777), lc=0': (-1, 'vali_pose_paint: kpts: strides (1000, 15, 3, 1099511627777) outside 0..2^40'),
    'kpt_decode heat=(0, 0, 0, 0)': (-1, 'vali_kpt_decode: neither heat nor both of simcc_x and simcc_y'),
    'kpt_decode simcc=(8192, 4000, 800, 12288, 4000, 800)': (-1, 'vali_kpt_decode: heat and SimCC vectors at once'),
    'kpt_decode dtype=-1': (-1, 'vali_kpt_decode: dtype -1 is not float32, float16 or bfloat16'),
    'kpt_decode dtype=3': (-1, 'vali_kpt_decode: dtype 3 is not float32, float16 or bfloat16'),
    'kpt_decode heat=(8193, 4000, 800, 20)': (-1, 'vali_kpt_decode: heat is not aligned to its element size'),
    'kpt_decode dtype=0, heat=(8193, 4000, 800, 20)': (-1, 'vali_kpt_decode: heat is not aligned to its element size'),
    'kpt_decode dtype=0, heat=(8194, 4000, 800, 20)': (-1, 'vali_kpt_decode: heat is not aligned to its element size'),
    'kpt_decode heat=(8192, -1, 800, 20)': (-1, 'vali_kpt_decode: a heat stride outside 0..2^40'),
    'kpt_decode heat=(8192, 1099511627777, 800, 20)': (-1, 'vali_kpt_decode: a heat stride outside 0..2^40'),
    'kpt_decode heat=(8192, 4000, -1, 20)': (-1, 'vali_kpt_decode: a heat stride outside 0..2^40'),
    'kpt_decode heat=(8192, 4000, 1099511627777, 20)': (-1, 'vali_kpt_decode: a heat stride outside 0..2^40'),
    'kpt_decode heat=(8192, 4000, 800, -1)': (-1, 'vali_kpt_decode: a heat stride outside 0..2^40'),
    'kpt_decode heat=(8192, 4000, 800, 1099511627777)': (-1, 'vali_kpt_decode: a heat stride outside 0..2^40'),
    'kpt_decode heat=(0, 0, 0, 0), simcc=(0, 4000, 800, 12288, 4000, 800)': (-1, 'vali_kpt_decode: neither heat nor both of simcc_x and simcc_y'),
    'kpt_decode heat=(0, 0, 0, 0), simcc=(8192, 4000, 800, 0, 4000, 800)': (-1, 'vali_kpt_decode: neither heat nor both of simcc_x and simcc_y'),
    'kpt_decode heat=(0, 0, 0, 0), simcc=(8193, 4000, 800, 12288, 4000, 800)': (-1, 'vali_kpt_decode: simcc_x or simcc_y is not aligned to its element size'),
    'kpt_decode heat=(0, 0, 0, 0), simcc=(8192, 4000, 800, 12289, 4000, 800)': (-1, 'vali_kpt_decode: simcc_x or simcc_y is not aligned to its element size'),
    'kpt_decode dtype=0, heat=(0, 0, 0, 0), simcc=(8194, 4000, 800, 12288, 4000, 800)': (-1, 'vali_kpt_decode: simcc_x or simcc_y is not aligned to its element size'),
    'kpt_decode dtype=0, heat=(0, 0, 0, 0), simcc=(8192, 4000, 800, 12290, 4000, 800)': (-1, 'vali_kpt_decode: simcc_x or simcc_y is not aligned to its element size'),
    'kpt_decode heat=(0, 0, 0, 0), simcc=(8192, -1, 800, 12288, 4000, 800)': (-1, 'vali_kpt_decode: a SimCC stride outside 0..2^40'),
    'kpt_decode heat=(0, 0, 0, 0), simcc=(8192, 1099511627777, 800, 12288, 4000, 800)': (-1, 'vali_kpt_decode: a SimCC stride outside 0..2^40'),
    'kpt_decode heat=(0, 0, 0, 0), simcc=(8192, 4000, -1, 12288, 4000, 800)': (-1, 'vali_kpt_decode: a SimCC stride outside 0..2^40'),
    'kpt_decode heat=(0, 0, 0, 0), simcc=(8192, 4000, 1099511627777, 12288, 4000, 800)': (-1, 'vali_kpt_decode: a SimCC stride outside 0..2^40'),
    'kpt_decode heat=(0, 0, 0, 0), simcc=(8192, 4000, 800, 12288, -1, 800)': (-1, 'vali_kpt_decode: a SimCC stride outside 0..2^40'),
    'kpt_decode heat=(0, 0, 0, 0), simcc=(8192, 4000, 800, 12288, 1099511627777, 800)': (-1, 'vali_kpt_decode: a SimCC stride outside 0..2^40'),
    'kpt_decode heat=(0, 0, 0, 0), simcc=(8192, 4000, 800, 12288, 4000, -1)': (-1, 'vali_kpt_decode: a SimCC stride outside 0..2^40'),
    'kpt_decode heat=(0, 0, 0, 0), simcc=(8192, 4000, 800, 12288, 4000, 1099511627777)': (-1, 'vali_kpt_decode: a SimCC stride outside 0..2^40'),
    'kpt_decode dtype=3, simcc=(8192, 4000, 800, 12288, 4000, 800)': (-1, 'vali_kpt_decode: heat and SimCC vectors at once'),
    'kpt_decode dtype=3, m=0': (-1, 'vali_kpt_decode: dtype 3 is not float32, float16 or bfloat16'),
    'kpt_decode heat=(8193, 4000, 800, 20), m=0': (-1, 'vali_kpt_decode: m outside 1..65535'),
    'kpt_decode heat=(8193, -1, 800, 20)': (-1, 'vali_kpt_decode: heat is not aligned to its element size'),
    'kpt_decode d_frames=4098, heat=(8192, 4000, 800, 1099511627777)': (-1, 'vali_kpt_decode: a heat stride outside 0..2^40'),
    'kpt_decode heat=(0, 0, 0, 0), simcc=(8192, 4000, 800, 12289, 4000, -1)': (-1, 'vali_kpt_decode: simcc_x or simcc_y is not aligned to its element size'),
    'kpt_decode d_frames=4098, heat=(0, 0, 0, 0), simcc=(8192, 4000, 800, 12288, 1099511627777, 800)': (-1, 'vali_kpt_decode: a SimCC stride outside 0..2^40'),
}
