"""numpy model of the quantiser of vali_jpeg_encode_tensor (include/vali_hip.h, "the same files straight from ONE batch
tensor"), and the inputs its tests share.

For element e (as float32) of channel c:
    v = fl32(fl32(e * scale[c]) + offset[c]);   p = 0 if v is NaN, else min(max(rint(v), 0), 255)
numpy multiplies and adds float32 arrays in two separately rounded steps, so the model is the definition as written;
tests/test_jpeg_tensor_host.py pins it to the torch chain it replaces.
"""
import numpy as np

DTYPES = ("float32", "float16", "bfloat16", "uint8")
BITS = {"float32": np.uint32, "float16": np.uint16, "bfloat16": np.uint16, "uint8": np.uint8}

# (scale, offset) per channel: the default of the float dtypes, [-1, 1] data, the default of uint8, and a triple with a
# negative scale; its second channel has a scale of 24 significant bits and an offset that cancels most of the product,
# which is where a fused multiply-add rounds differently (fma_differs)
SCALE_OFFSETS = (
    ((255.0, 255.0, 255.0), (0.0, 0.0, 0.0)),
    ((127.5, 127.5, 127.5), (127.5, 127.5, 127.5)),
    ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),
    ((-255.0, 1021.7142944335938, 0.75), (255.0, -893.5, 3.25)),
)


def as_float32(bits, dtype):
    """the elements whose bit patterns `bits` holds, as float32: exact for every dtype"""
    bits = np.asarray(bits)
    if dtype == "float32":
        return bits.astype(np.uint32).view(np.float32)
    if dtype == "float16":
        return bits.astype(np.uint16).view(np.float16).astype(np.float32)
    if dtype == "bfloat16":
        return (bits.astype(np.uint32) << 16).view(np.float32)
    return bits.astype(np.float32)


def quantise(e, scale, offset):
    """p of the definition; `e` float32 with the channel as its LAST axis (or scalar scale / offset)"""
    e = np.asarray(e, np.float32)
    with np.errstate(all="ignore"):
        v = e * np.asarray(scale, np.float32)
        assert v.dtype == np.float32
        v = v + np.asarray(offset, np.float32)
        assert v.dtype == np.float32
        v = np.where(np.isnan(v), np.float32(0), v)
        return np.minimum(np.maximum(np.rint(v), 0), 255).astype(np.uint8)


def quantise_fma(e, scale, offset):
    """what a kernel that contracts the two operations into one fused multiply-add would give: the product is exact in
    float64 (24 + 24 bits), the sum is rounded to float64 and then to float32 -- only ever used to FIND inputs where the
    byte differs from quantise()"""
    with np.errstate(all="ignore"):
        e = np.asarray(e, np.float32).astype(np.float64)
        v = (e * np.asarray(scale, np.float32).astype(np.float64) +
             np.asarray(offset, np.float32).astype(np.float64)).astype(np.float32)
        v = np.where(np.isnan(v), np.float32(0), v)
        return np.minimum(np.maximum(np.rint(v), 0), 255).astype(np.uint8)


def fma_differs(e, scale, offset):
    """mask of the elements a fused multiply-add would quantise to another byte"""
    return quantise(e, scale, offset) != quantise_fma(e, scale, offset)


def all_patterns(dtype=None):
    """every bit pattern of a 16-bit dtype"""
    return np.arange(65536, dtype=np.uint32).astype(np.uint16)


def _around(x):
    x = np.asarray(x, np.float32)
    return np.concatenate([np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))])


def float32_edges(steps=2):
    """float32 inputs: +-0, +-inf, NaN, subnormals, and for every (scale, offset) pair above the inputs that land on and
    just around (`steps` neighbours either side) every tie k + 0.5, k = -1..256"""
    ties = np.arange(-1, 257, dtype=np.float64) + 0.5
    parts = [np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, 3.4028235e38,
                       -3.4028235e38, 1.0, -1.0, 0.5, 255.0, 256.0], np.float32)]
    for scale, offset in SCALE_OFFSETS:
        for s, o in sorted(set(zip(scale, offset))):
            x = ((ties - o) / s).astype(np.float32)
            # a few steps either side: the tie is met by the neighbours of the rounded quotient too
            for _ in range(steps):
                x = np.unique(_around(x))
            parts.append(x)
    return np.concatenate(parts)


def edge_bits(dtype):
    """the bit patterns of a compact edge set of `dtype` for the GPU test of the quantiser: the float32 edge set (one
    neighbour either side of a tie) rounded to the dtype, plus the dtype's own subnormals and specials"""
    import torch

    f = torch.from_numpy(float32_edges(1))
    if dtype == "float32":
        return f.numpy().view(np.uint32)
    t = f.to(torch.float16 if dtype == "float16" else torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    own = np.array([0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x007F, 0x807F, 0x0080, 0x7C00, 0xFC00, 0x7E00, 0x7F80,
                    0xFF80, 0x7FC0, 0x8000, 0x0000], np.uint16)
    return np.unique(np.concatenate([t, own]))


def noise_bits(dtype, shape, scale, offset, seed):
    """seeded noise of `shape` (channels LAST) as bit patterns, spread so that about a tenth of the elements fall outside
    0..255 after scale / offset"""
    rng = np.random.default_rng(seed)
    if dtype == "uint8":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    import torch

    want = rng.uniform(-14.0, 269.0, shape)                      # 255 / 0.9 wide, centred on 127.5
    e = (want - np.asarray(offset, np.float64)) / np.asarray(scale, np.float64)
    t = torch.from_numpy(e.astype(np.float32))
    if dtype == "float32":
        return t.numpy().view(np.uint32)
    return t.to(torch.float16 if dtype == "float16" else torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def torch_tensor(bits, dtype):
    """a torch CPU tensor of `dtype` with these bit patterns, same shape"""
    import torch

    bits = np.ascontiguousarray(bits)
    if dtype == "float32":
        return torch.from_numpy(bits.view(np.float32).copy())
    if dtype == "uint8":
        return torch.from_numpy(bits.copy())
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.float16 if dtype == "float16" else torch.bfloat16)


def torch_chain(x, scale, offset):
    """the chain RunTensor replaces, on a torch tensor with the channel as its last axis"""
    import torch

    s, o = torch.tensor(scale, dtype=torch.float32), torch.tensor(offset, dtype=torch.float32)
    return torch.nan_to_num(x.float() * s + o, nan=0.0).round().clamp(0, 255).to(torch.uint8)
