"""Every place that reads a caller's device tensor, driven without a device: stand-ins that expose
__cuda_array_interface__ as a dict and a `.device`, and CPU numpy / torch tensors through __dlpack__.  One table; the
expected message of every refusal is written out.  None marks what is accepted."""
import types
from functools import partial

import numpy as np
import pytest


# ---- what goes in ---------------------------------------------------------------------------------------------------------
class Cai:
    """a device array seen through __cuda_array_interface__ (never dereferenced).  device: (type, index), "bare" for a
    `.device` with neither attribute (CuPy's has `.id`), None for no `.device` at all"""

    def __init__(self, shape, typestr, strides=None, device=("cuda", 0)):
        self.shape = tuple(shape)
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (4096, False), "version": 3,
                                         "strides": strides}
        if device == "bare":
            self.device = types.SimpleNamespace(id=0)
        elif device is not None:
            self.device = types.SimpleNamespace(type=device[0], index=device[1])


class OnlyDlpack:
    """a CPU array that speaks __dlpack__ and does not say where it is"""

    def __init__(self, a):
        self._a, self.shape = a, a.shape

    def __dlpack__(self, **_kw):
        return self._a.__dlpack__()


def host(shape, dtype):
    return np.zeros(shape, dtype)


def bf16(shape):
    import torch

    return torch.zeros(shape, dtype=torch.bfloat16)


# ---- the intakes, each as its public caller reaches it --------------------------------------------------------------------
def _marks(vali, t):
    """PySurfaceAnnotator.RunBatch on a batch of no frames: the marks are judged, nothing is launched"""
    ann = object.__new__(vali.PySurfaceAnnotator)
    ann._gpu_id, ann._stream = 0, 0
    ab = object.__new__(vali.AnnotateBatch)
    ab.gpu_id, ab.n, ab.format, ab.sizes, ab.d_marks, ab._marks_keep = 0, 0, vali.RGB, [], 0, None
    assert ann.RunBatchAsync(ab, t) == (True, vali.TaskExecInfo.SUCCESS)


def _colours(vali, t):
    """PyInstanceMasker.Run up to its `rects`, which are refused: the colours were accepted"""
    mk = object.__new__(vali.PyInstanceMasker)
    mk._gpu_id, mk._stream = 0, 0
    mb = object.__new__(vali.MaskBatch)
    mb.gpu_id, mb.n, mb.format, mb._colours_keep, mb._colours = 0, 2, vali.RGB, {}, {}
    try:
        mk.RunAsync(mb, 5, t)
    except ValueError as e:
        if not str(e).startswith("rects: a device tensor "):
            raise
    else:
        raise AssertionError("Run went past rects that are no rects")


def drivers(vali):
    from vali_amd import _runargs, detect, mask, pose, tasks, tensors

    def i32(who, shape):
        return lambda t: tensors.device_i32(who, t, shape, 0)

    def head(who, layout_of):
        return lambda t: tensors.device_float(who, t, layout_of, 0, *tensors.HEAD_CAI)

    return {
        "rects": lambda t: _runargs.device_rects(t, 2, 0),
        "marks": partial(_marks, vali),
        "dets": i32("dets", (4, 8)),
        "points": i32("points", (4, 17, 4)),
        "colours": partial(_colours, vali),
        "boxes": head("boxes", partial(detect.head_layout, "boxes", last=4)),
        "scores": head("scores", partial(detect.head_layout, "scores")),
        "protos": head("protos", mask.protos_layout),
        "coeffs": head("coeffs", mask.coeffs_layout),
        "kpts": head("kpts", pose.kpts_layout),
        "out": lambda t: tasks._tensor_dst(t, 0),
        "tensor": lambda t: tasks._tensor_src(t, 0),
    }


# ---- the table ------------------------------------------------------------------------------------------------------------
I4, F4 = "<i4", "<f4"
CAI_OR_DLPACK = "a device tensor with __cuda_array_interface__ or __dlpack__"
DLPACK_OR_CAI = "a device tensor with __dlpack__ or __cuda_array_interface__"
HEADS_CAI = "the dtype must be float32 or float16 through __cuda_array_interface__ (bfloat16: __dlpack__), got <f8"
F64 = "(DLPack code 2, 64 bits)"

CASES = [
    # rects: the (n, 8) records of a batch of n = 2
    ("rects", Cai((2, 8), I4), None),
    ("rects", Cai((2, 8), "|i4", (32, 4)), None),
    ("rects", Cai((2, 8), I4, device=None), None),                          # no .device: the pointer is asked
    ("rects", Cai((2, 8), F4), "rects: need an int32 tensor of shape (2, 8), got <f4 (2, 8)"),
    ("rects", Cai((3, 8), I4), "rects: need an int32 tensor of shape (2, 8), got <i4 (3, 8)"),
    ("rects", Cai((2, 8), I4, (64, 4)), "rects: the tensor must be contiguous"),
    ("rects", Cai((2, 8), I4, (32, 6)), "rects: the tensor must be contiguous"),
    ("rects", Cai((2, 8), I4, device=("cuda", 1)), "rects: the tensor is on device 1, the batch on 0"),
    ("rects", host((2, 8), np.int32), "rects: the tensor must live on the GPU"),
    ("rects", host((2, 8), np.float32), "rects: need an int32 tensor of shape (2, 8)"),
    ("rects", host((2, 4), np.int32), "rects: need an int32 tensor of shape (2, 8)"),
    ("rects", host((4, 8), np.int32)[::2], "rects: the tensor must be contiguous"),
    ("rects", object(), "rects: " + CAI_OR_DLPACK),
    # marks: (M, 8), M from 0
    ("marks", Cai((3, 8), I4), None),
    ("marks", Cai((0, 8), I4), None),
    ("marks", Cai((1, 8), I4, (4, 4)), None),                               # the stride of a dimension of size 1
    ("marks", Cai((3, 8), F4), "marks: need an int32 tensor of shape (M, 8), got <f4 (3, 8)"),
    ("marks", Cai((3, 7), I4), "marks: need an int32 tensor of shape (M, 8), got <i4 (3, 7)"),
    ("marks", Cai((24,), I4), "marks: need an int32 tensor of shape (M, 8), got <i4 (24,)"),
    ("marks", Cai((3, 8), I4, (64, 4)), "marks: the tensor must be contiguous"),
    ("marks", Cai((3, 8), I4, device=("cuda", 1)), "marks: the tensor is on device 1, the batch on 0"),
    ("marks", Cai((4097, 8), I4), "marks: 4097 rows; at most 4096 per call"),
    ("marks", host((3, 8), np.int32), "marks: the tensor must live on the GPU"),
    ("marks", host((3, 8), np.int64), "marks: need an int32 tensor of shape (M, 8), got shape (3, 8)"),
    ("marks", host((3, 8, 1), np.int32), "marks: need an int32 tensor of shape (M, 8), got shape (3, 8, 1)"),
    ("marks", object(), "marks: " + CAI_OR_DLPACK + ", or a sequence of 8-tuples"),
    # dets, and with them counts, rois and the selector's marks: an exact shape
    ("dets", Cai((4, 8), I4), None),
    ("dets", Cai((4, 8), I4, (32, 4)), None),
    ("dets", Cai((4, 8), F4), "dets: need an int32 tensor of shape (4x8), got <f4 (4, 8)"),
    ("dets", Cai((3, 8), I4), "dets: need an int32 tensor of shape (4x8), got <i4 (3, 8)"),
    ("dets", Cai((32,), I4), "dets: need an int32 tensor of shape (4x8), got <i4 (32,)"),
    ("dets", Cai((4, 8), I4, (64, 4)), "dets: the tensor must be contiguous"),
    ("dets", Cai((4, 8), I4, (32, 3)), "dets: the tensor must be contiguous"),
    ("dets", Cai((4, 8), I4, device=("cuda", 1)), "dets: the tensor is on device 1, the task on 0"),
    ("dets", host((4, 8), np.int32), "dets: the tensor must live on the GPU"),
    ("dets", host((4, 8), np.uint32), "dets: need an int32 tensor of shape (4x8), got shape (4, 8)"),
    ("dets", host((8, 8), np.int32)[::2], "dets: the tensor must be contiguous"),
    ("dets", [[0] * 8] * 4, "dets: " + CAI_OR_DLPACK),
    # points: three dimensions
    ("points", Cai((4, 17, 4), I4), None),
    ("points", Cai((4, 17, 4), I4, (272, 16, 4)), None),
    ("points", Cai((4, 17, 4), "<i8"), "points: need an int32 tensor of shape (4x17x4), got <i8 (4, 17, 4)"),
    ("points", Cai((4, 17, 3), I4), "points: need an int32 tensor of shape (4x17x4), got <i4 (4, 17, 3)"),
    ("points", Cai((4, 17, 4), I4, (272, 32, 4)), "points: the tensor must be contiguous"),
    ("points", Cai((4, 17, 4), I4, device=("cuda", 1)), "points: the tensor is on device 1, the task on 0"),
    ("points", host((4, 17, 4), np.int32), "points: the tensor must live on the GPU"),
    ("points", None, "points: " + CAI_OR_DLPACK),
    # colours: (n,), n from 1.  One look at the tensor, so one message for its shape and its dtype: before, a wrong shape
    # was "..., got (2, 3)" without the dtype and a wrong dtype "... of shape (3), got <f4 (3,)"
    ("colours", Cai((3,), I4), None),
    ("colours", Cai((3,), I4, (4,)), None),
    ("colours", Cai((3,), F4), "colours: need an int32 tensor of shape (n,), n >= 1, got <f4 (3,)"),
    ("colours", Cai((2, 3), I4), "colours: need an int32 tensor of shape (n,), n >= 1, got <i4 (2, 3)"),
    ("colours", Cai((0,), I4), "colours: need an int32 tensor of shape (n,), n >= 1, got <i4 (0,)"),
    ("colours", Cai((3,), I4, (8,)), "colours: the tensor must be contiguous"),
    ("colours", Cai((3,), I4, device=("cuda", 1)), "colours: the tensor is on device 1, the task on 0"),
    ("colours", OnlyDlpack(host((3,), np.int32)), "colours: the tensor must live on the GPU"),
    ("colours", 5, "colours: an int32 device tensor or a sequence of packed colours (pack_colour)"),
    # the heads: boxes and scores ...
    ("boxes", Cai((2, 100, 4), F4), None),
    ("boxes", Cai((2, 100, 4), "<f2", (800, 2, 200)), None),
    ("boxes", Cai((2, 100, 4), "<f8"), "boxes: " + HEADS_CAI),
    ("boxes", Cai((2, 100, 4), I4), "boxes: the dtype must be float32 or float16 through __cuda_array_interface__ "
                                     "(bfloat16: __dlpack__), got <i4"),
    ("boxes", Cai((100, 4), F4), "boxes: need a 3-D tensor (N, K, 4), got 2-D (100, 4)"),
    ("boxes", Cai((2, 100, 5), F4), "boxes: the last dimension must be 4, got (2, 100, 5)"),
    ("boxes", Cai((2, 100, 4), F4, (1600, 16, 3)), "boxes: strides that are no multiple of the element size"),
    ("boxes", Cai((2, 100, 4), F4, device=("cuda", 1)), "boxes: the tensor is on device 1, the task on 0"),
    ("boxes", host((2, 100, 4), np.float32), "boxes: the tensor must live on the GPU"),
    ("boxes", host((2, 100, 4), np.float64), "boxes: the dtype must be float32, float16 or bfloat16 " + F64),
    ("boxes", object(), "boxes: " + DLPACK_OR_CAI),
    ("scores", Cai((2, 100, 3), F4), None),
    ("scores", Cai((2, 100, 3), "<f8"), "scores: " + HEADS_CAI),
    ("scores", Cai((2, 100, 3, 1), F4), "scores: need a 3-D tensor (N, K, C), got 4-D (2, 100, 3, 1)"),
    ("scores", Cai((2, 100, 3), "<f2", (600, 6, 1)), "scores: strides that are no multiple of the element size"),
    ("scores", Cai((2, 100, 3), F4, device=("cuda", 1)), "scores: the tensor is on device 1, the task on 0"),
    ("scores", bf16((2, 100, 3)), "scores: the tensor must live on the GPU"),
    ("scores", [[[0.5]]], "scores: " + DLPACK_OR_CAI),
    # ... protos, coeffs and kpts
    ("protos", Cai((2, 32, 40, 40), F4), None),
    ("protos", Cai((2, 32, 40, 40), "<f8"), "protos: " + HEADS_CAI),
    ("protos", Cai((32, 40, 40), F4), "protos: need a 4-D tensor (N, M, Hp, Wp), got 3-D (32, 40, 40)"),
    ("protos", Cai((2, 32, 40, 40), F4, (204800, 6400, 160, 2)), "protos: strides that are no multiple of the element size"),
    ("protos", Cai((2, 32, 40, 40), F4, device=("cuda", 1)), "protos: the tensor is on device 1, the task on 0"),
    ("protos", host((2, 32, 40, 40), np.float16), "protos: the tensor must live on the GPU"),
    ("protos", host((2, 32, 40, 40), np.float64), "protos: the dtype must be float32, float16 or bfloat16 " + F64),
    ("protos", object(), "protos: " + DLPACK_OR_CAI),
    ("coeffs", Cai((2, 100, 32), "<f2"), None),
    ("coeffs", Cai((2, 100, 32), "|u1"), "coeffs: the dtype must be float32 or float16 through __cuda_array_interface__ "
                                          "(bfloat16: __dlpack__), got |u1"),
    ("coeffs", Cai((100, 32), F4), "coeffs: need a 3-D tensor (N, K, M), got 2-D (100, 32)"),
    ("coeffs", Cai((2, 100, 32), F4, (12800, 128, 5)), "coeffs: strides that are no multiple of the element size"),
    ("coeffs", Cai((2, 100, 32), F4, device=("cuda", 1)), "coeffs: the tensor is on device 1, the task on 0"),
    ("coeffs", bf16((2, 100, 32)), "coeffs: the tensor must live on the GPU"),
    ("coeffs", object(), "coeffs: " + DLPACK_OR_CAI),
    ("kpts", Cai((2, 100, 17, 3), F4), None),
    ("kpts", Cai((2, 100, 17, 3), "<f8"), "kpts: " + HEADS_CAI),
    ("kpts", Cai((2, 100, 51), F4), "kpts: need a 4-D tensor (N, K, P, 3 or 2), got 3-D (2, 100, 51)"),
    ("kpts", Cai((2, 100, 17, 3), F4, (20400, 204, 12, 2)), "kpts: strides that are no multiple of the element size"),
    ("kpts", Cai((2, 100, 17, 3), F4, device=("cuda", 1)), "kpts: the tensor is on device 1, the task on 0"),
    ("kpts", host((2, 100, 17, 3), np.float32), "kpts: the tensor must live on the GPU"),
    ("kpts", object(), "kpts: " + DLPACK_OR_CAI),
    # out (PrepareTensorBatch) and tensor (the JPEG encoder's RunTensor, the postprocessor)
    ("out", Cai((2, 3, 8, 10), F4), None),
    ("out", Cai((2, 3, 8, 10), "<f2", (480, 2, 60, 6)), None),              # channels last
    ("out", Cai((2, 3, 8, 10), "<f8"), "out: the dtype must be float32 or float16 through __cuda_array_interface__, got <f8"),
    ("out", Cai((2, 3, 8, 10), "|u1"), "out: the dtype must be float32 or float16 through __cuda_array_interface__, got |u1"),
    ("out", Cai((3, 8, 10), F4), "out: need a 4-D tensor (N, 3, H, W), got 3-D (3, 8, 10)"),
    ("out", Cai((2, 3, 8, 10), F4, (960, 320, 40, 2)), "out: strides that are no multiple of the element size"),
    ("out", Cai((2, 3, 8, 10), F4, device=("cuda", 1)), "out: the tensor is on device 1, the task on 0"),
    ("out", host((2, 3, 8, 10), np.float32), "out: the tensor must live on the GPU"),
    ("out", host((2, 3, 8, 10), np.float64), "out: the dtype must be float32, float16 or bfloat16 " + F64),
    ("out", host((2, 3, 8, 10), np.uint8), "out: the dtype must be float32, float16 or bfloat16 (DLPack code 1, 8 bits)"),
    ("out", object(), "out: " + DLPACK_OR_CAI),
    ("tensor", Cai((2, 3, 8, 10), F4), None),
    ("tensor", Cai((2, 3, 8, 10), "|u1"), None),
    ("tensor", Cai((2, 3, 8, 10), "<f8"), "tensor: the dtype must be float32 or float16 or uint8 through "
                                           "__cuda_array_interface__, got <f8"),
    ("tensor", Cai((2, 4, 8, 10), F4), "tensor: need 3 channels (N, 3, H, W), got C = 4"),
    ("tensor", Cai((2, 3, 8, 10), "<f2", (480, 160, 20, 1)), "tensor: strides that are no multiple of the element size"),
    ("tensor", Cai((2, 3, 8, 10), F4, device=("cuda", 1)), "tensor: the tensor is on device 1, the task on 0"),
    ("tensor", host((2, 3, 8, 10), np.uint8), "tensor: the tensor must live on the GPU"),
    ("tensor", bf16((2, 3, 8, 10)), "tensor: the tensor must live on the GPU"),
    ("tensor", host((2, 3, 8, 10), np.float64), "tensor: the dtype must be float32, float16, bfloat16 or uint8 " + F64),
    ("tensor", object(), "tensor: " + DLPACK_OR_CAI),
]

# one good tensor per intake, for the device rule: (shape, typestr)
GOOD = {"rects": ((2, 8), I4), "marks": ((3, 8), I4), "dets": ((4, 8), I4), "points": ((4, 17, 4), I4), "colours": ((3,), I4),
        "boxes": ((2, 100, 4), F4), "scores": ((2, 100, 3), F4), "protos": ((2, 32, 40, 40), F4),
        "coeffs": ((2, 100, 32), F4), "kpts": ((2, 100, 17, 3), F4), "out": ((2, 3, 8, 10), F4), "tensor": ((2, 3, 8, 10), F4)}


def _no_pointer_is_asked(p):
    raise AssertionError(f"shim.ptr_device({p}) was called")


@pytest.fixture
def asked(vali, monkeypatch):
    """the pointers shim.ptr_device is asked about; every one of them is on device 0"""
    from vali_amd._native import shim

    seen = []
    monkeypatch.setattr(shim, "ptr_device", lambda p: seen.append(p) or 0)
    return seen


@pytest.mark.parametrize("intake, t, message", CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(CASES)])
def test_intake_says_what_is_wrong(vali, asked, intake, t, message):
    drive = drivers(vali)[intake]
    if message is None:
        drive(t)
        return
    with pytest.raises(ValueError) as e:
        drive(t)
    assert str(e.value) == message


@pytest.mark.parametrize("intake", sorted(GOOD))
def test_a_device_without_type_or_index_is_asked_by_pointer(vali, asked, intake):
    """CuPy's Device has `.id`: every intake takes such a tensor and finds its device through the pointer"""
    drivers(vali)[intake](Cai(*GOOD[intake], device="bare"))
    assert asked == [4096]
    drivers(vali)[intake](Cai(*GOOD[intake], device=("cuda", None)))
    assert asked == [4096, 4096]
    drivers(vali)[intake](Cai(*GOOD[intake], device=("cuda", 0)))          # an index is believed
    assert asked == [4096, 4096]


@pytest.mark.parametrize("intake", sorted(GOOD))
def test_a_device_of_another_type_is_not_the_gpu(vali, asked, intake):
    with pytest.raises(ValueError) as e:
        drivers(vali)[intake](Cai(*GOOD[intake], device=("cpu", 0)))
    assert str(e.value) == f"{intake}: the tensor must live on the GPU"
    assert asked == []


def test_the_pointer_of_a_tensor_on_another_device_is_believed(vali, monkeypatch):
    from vali_amd._native import shim

    monkeypatch.setattr(shim, "ptr_device", lambda p: 3)
    with pytest.raises(ValueError) as e:
        drivers(vali)["dets"](Cai((4, 8), I4, device="bare"))
    assert str(e.value) == "dets: the tensor is on device 3, the task on 0"


def test_marks_of_no_rows_and_no_memory_are_on_the_tasks_device(vali, monkeypatch):
    from vali_amd._native import shim

    monkeypatch.setattr(shim, "ptr_device", _no_pointer_is_asked)
    empty = Cai((0, 8), I4, device=None)
    empty.__cuda_array_interface__["data"] = (0, False)
    _marks(vali, empty)


@pytest.mark.parametrize("intake", sorted(GOOD))
def test_a_tensor_is_exported_once(vali, asked, intake):
    """one __dlpack__ per intake: an export is a capsule to import and release"""
    class Counting(OnlyDlpack):
        calls = 0

        def __dlpack__(self, **_kw):
            Counting.calls += 1
            return self._a.__dlpack__()

    shape, typestr = GOOD[intake]
    with pytest.raises(ValueError, match=f"^{intake}: the tensor must live on the GPU$"):
        drivers(vali)[intake](Counting(host(shape, np.int32 if typestr == I4 else np.float32)))
    assert Counting.calls == 1
