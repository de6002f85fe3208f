"""Model of vali_tensor_to_surfaces / PySurfacePostprocessor (include/vali_hip.h, "batch tensor -> video frames").

The model is made of the two pinned halves the definition names and of nothing else:
    p    = vali_amd.codecs._quantise_tensor     the quantiser of vali_jpeg_encode_tensor (pinned to the torch chain on
                                                all 65,536 half-precision bit patterns by tests/test_jpeg_tensor_host.py)
    YUV  = oracle.convert RGB -> YUV420 / YUV444 with cvt_params(rgb2yuv_rows=...)   (oracle/vali_oracle_cvt.c)
    NV12 = the YUV420 planes with U and V interleaved (numpy)
numpy_yuv() is a second, independent statement of the fmaf chain and the 2 x 2 mean; tests/test_postproc_host.py holds
the two against each other.
"""
import numpy as np

DSTS = ("NV12", "YUV420", "YUV444", "RGB", "RGB_PLANAR")


def matrices():
    """name -> rows (kR, kG, kB, offset) of Y, U, V: the four matrices PySurfacePostprocessor selects between"""
    from vali_amd import tasks

    return {"601_JPEG": tasks.RGB2YUV_NPP_YUV, "601_MPEG": tasks.RGB2YUV_NPP_YCBCR,
            "709_JPEG": tasks.RGB2YUV_BT709_JPEG, "709_MPEG": tasks.RGB2YUV_BT709_MPEG}


def cc_ctx_of(vali, name):
    space, rng = name.split("_")
    return vali.ColorspaceConversionContext(getattr(vali.ColorSpace, "BT_" + space), getattr(vali.ColorRange, rng))


def quantise(bits, dtype, scale, offset, channels="RGB"):
    """(..., 3) bit patterns, channels LAST in the tensor's order -> (..., 3) uint8 R, G, B.  scale and offset belong to
    the TENSOR's channels; `channels` then names them"""
    from vali_amd.codecs import _quantise_tensor

    p = _quantise_tensor(np.ascontiguousarray(bits), dtype, scale, offset)
    return p[..., ::-1] if channels == "BGR" else p


def from_rgb(oracle, p, dst, rows):
    """(H, W, 3) uint8 R, G, B -> the flat tightly packed host image (Surface.HostSize layout) of format `dst`"""
    h, w = p.shape[:2]
    p = np.ascontiguousarray(p)
    if dst == "RGB":
        return p.reshape(-1).copy()
    if dst == "RGB_PLANAR":
        return np.ascontiguousarray(p.transpose(2, 0, 1)).reshape(-1)
    params = oracle.cvt_params(rgb2yuv_rows=rows)
    if dst == "YUV444":
        return oracle.convert(p.reshape(-1), "RGB", "YUV444", w, h, params)
    yuv = oracle.convert(p.reshape(-1), "RGB", "YUV420", w, h, params)
    if dst == "YUV420":
        return yuv
    assert dst == "NV12"
    c = (w // 2) * (h // 2)
    out = np.empty(w * h + 2 * c, np.uint8)
    out[:w * h] = yuv[:w * h]
    out[w * h::2] = yuv[w * h:w * h + c]
    out[w * h + 1::2] = yuv[w * h + c:]
    return out


def model(oracle, bits, dtype, scale, offset, channels, dst, rows):
    """(N, H, W, 3) bit patterns -> list of N flat host images"""
    p = quantise(bits, dtype, scale, offset, channels)
    return [from_rgb(oracle, p[i], dst, rows) for i in range(p.shape[0])]


# ---- the second statement ---------------------------------------------------------------------------------------------
def _fmaf(a, b, c):
    """fmaf(a, b, c) on float32 arrays where a * b + c is exact in float64: a float32 constant (24 bits) times an 8-bit
    integer is exact (32 bits), and adding a float32 addend of comparable magnitude stays within 53 bits -- one
    rounding, to float32, as the fused operation has"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _sat_u8(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def numpy_yuv(p, rows, dst):
    """(H, W, 3) uint8 R, G, B -> flat YUV444 / YUV420 / NV12 host image, from the words of the definition"""
    h, w = p.shape[:2]
    m = np.asarray(rows, np.float32)
    r, g, b = (p[..., c].astype(np.float32) for c in range(3))
    o = []
    for k in range(3):
        full = lambda v: np.full((h, w), v, np.float32)            # noqa: E731
        o.append(_fmaf(full(m[k, 2]), b, _fmaf(full(m[k, 1]), g, _fmaf(full(m[k, 0]), r, full(m[k, 3])))))
    y = _sat_u8(o[0])
    if dst == "YUV444":
        return np.concatenate([y.reshape(-1), _sat_u8(o[1]).reshape(-1), _sat_u8(o[2]).reshape(-1)])
    planes = []
    for c in o[1:]:
        s = (c[0::2, 0::2] + c[0::2, 1::2]) + (c[1::2, 0::2] + c[1::2, 1::2])      # float32 adds, in this association
        assert s.dtype == np.float32
        planes.append(_sat_u8(s * np.float32(0.25)))
    if dst == "YUV420":
        return np.concatenate([y.reshape(-1), planes[0].reshape(-1), planes[1].reshape(-1)])
    uv = np.stack(planes, -1)
    return np.concatenate([y.reshape(-1), uv.reshape(-1)])


# ---- inputs -----------------------------------------------------------------------------------------------------------
def lattice(w, h):
    """(H, W, 3) uint8: a colour lattice that walks all three channels through 0..255 with different periods, corners of
    the cube included"""
    yy, xx = np.mgrid[0:h, 0:w]
    k = yy * w + xx
    p = np.stack([(k * 37) % 256, (k * 101 + 255) % 256, (k * 17 + yy * 85) % 256], -1).astype(np.uint8)
    corners = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)]
    flat = p.reshape(-1, 3)
    for i, c in enumerate(corners[:flat.shape[0]]):
        flat[i] = c
    return p


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def planes_of(dst, flat, w, h):
    """the flat host image as a list of 2-D planes (rows x bytes), in the order the surface stores them"""
    flat = np.asarray(flat)
    if dst == "RGB":
        return [flat.reshape(h, 3 * w)]
    if dst in ("RGB_PLANAR", "YUV444"):
        return [flat[c * w * h:(c + 1) * w * h].reshape(h, w) for c in range(3)]
    if dst == "NV12":
        return [flat[:w * h].reshape(h, w), flat[w * h:].reshape(h // 2, w)]
    c = (w // 2) * (h // 2)
    return [flat[:w * h].reshape(h, w), flat[w * h:w * h + c].reshape(h // 2, w // 2), flat[w * h + c:].reshape(h // 2, w // 2)]
