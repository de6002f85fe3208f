"""The teardown of every prepared batch, driven without a device: objects made with object.__new__, fake device pointers,
and recorders in place of the shim's mem_free and stream_sync.  The owned and borrowed arrays of each class are written
out here, not read from the classes."""
import pytest

# class -> (module, owned device arrays, borrowed device arrays)
BATCHES = {
    "SurfaceBatch": ("tasks", "d_src d_dst", ""),
    "RoiBatch": ("tasks", "d_src d_dst d_roi", ""),
    "TensorBatch": ("tasks", "d_src d_roi", ""),
    "FrameBatch": ("tasks", "d_dst", ""),
    "AnnotateBatch": ("tasks", "d_frames d_ws d_marks", ""),
    "SelectBatch": ("detect", "d_ws d_rects", "d_dets d_counts d_rois d_marks"),
    "MaskBatch": ("mask", "d_frames d_ws d_rects d_colours", "d_dets"),
    "SemanticBatch": ("semantic", "d_frames d_labels d_rects d_colours", ""),
    "PoseBatch": ("pose", "d_frames d_ws d_rects d_limbs d_limb_colours d_joint_colours", "d_dets d_points"),
    "PointsBatch": ("pose", "d_frames d_ws d_limbs d_limb_colours d_joint_colours", "d_points"),
    "KeypointBatch": ("keypoints", "d_frames", "d_matrices d_rois d_points d_kpts"),
    "WarpBatch": ("warp", "d_frames d_ws d_rects d_template", "d_dets d_matrices"),
}
CASES = [(name, False) for name in BATCHES] + [("WarpBatch", True)]     # True: d_matrices aliases d_ws
GPU, STREAM = 3, 0x5EED


class Recorder:
    """stands in for shim.stream_sync and shim.mem_free: every call in order"""

    def __init__(self, monkeypatch, fail_free=False):
        import vali_amd._native

        self.calls = []

        def free(gpu_id, ptr):
            self.calls.append(("mem_free", gpu_id, ptr))
            if fail_free:
                raise RuntimeError("mem_free failed")

        monkeypatch.setattr(vali_amd._native.shim, "stream_sync", lambda g, s: self.calls.append(("stream_sync", g, s)))
        monkeypatch.setattr(vali_amd._native.shim, "mem_free", free)


def make(name, alias):
    """(batch, {owned name: pointer}, {borrowed name: pointer}) with gpu_id, _stream and distinct fake pointers set"""
    import importlib

    module, owned, borrowed = BATCHES[name]
    b = object.__new__(getattr(importlib.import_module("vali_amd." + module), name))
    b.gpu_id, b._stream = GPU, STREAM
    owned = {attr: 0x1000 * (i + 1) for i, attr in enumerate(owned.split())}
    borrowed = {attr: 0x100000 * (i + 1) for i, attr in enumerate(borrowed.split())}
    if alias:
        borrowed["d_matrices"] = owned["d_ws"]
    for attr, p in {**owned, **borrowed}.items():
        setattr(b, attr, p)
    return b, owned, borrowed


@pytest.mark.parametrize("name, alias", CASES, ids=[n + ("-rows-in-ws" if a else "") for n, a in CASES])
def test_del_frees_what_the_batch_owns_after_its_stream(monkeypatch, name, alias):
    rec = Recorder(monkeypatch)
    b, owned, borrowed = make(name, alias)
    b.__del__()
    # (a) one synchronisation of the batch's stream, before anything is freed
    assert rec.calls[0] == ("stream_sync", GPU, STREAM)
    assert [c[0] for c in rec.calls].count("stream_sync") == 1
    # (b) exactly the owned arrays, each once, on the batch's device
    frees = rec.calls[1:]
    assert all(c[0] == "mem_free" and c[1] == GPU for c in frees)
    assert sorted(c[2] for c in frees) == sorted(owned.values())
    # (c) owned attributes are cleared, borrowed ones untouched
    assert all(getattr(b, attr) == 0 for attr in owned)
    assert all(getattr(b, attr) == p for attr, p in borrowed.items())
    # (d) a second teardown has nothing left to do
    del rec.calls[:]
    b.__del__()
    assert rec.calls == []


@pytest.mark.parametrize("name, alias", CASES, ids=[n + ("-rows-in-ws" if a else "") for n, a in CASES])
def test_del_survives_a_failing_free(monkeypatch, name, alias):
    rec = Recorder(monkeypatch, fail_free=True)
    b, owned, borrowed = make(name, alias)
    b.__del__()                                                  # (e) returns ...
    assert sorted(c[2] for c in rec.calls if c[0] == "mem_free") == sorted(owned.values())
    assert all(getattr(b, attr) == 0 for attr in owned)          # ... and still clears
    assert all(getattr(b, attr) == p for attr, p in borrowed.items())


@pytest.mark.parametrize("name", list(BATCHES))
def test_del_of_a_bare_object_is_silent(monkeypatch, name):
    import importlib

    rec = Recorder(monkeypatch)
    object.__new__(getattr(importlib.import_module("vali_amd." + BATCHES[name][0]), name)).__del__()     # (f)
    assert rec.calls == []
