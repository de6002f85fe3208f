"""bench.py --dump-outputs on the host: what dump_outputs() writes for a batch of frames (CPU tensors stand in for the
destination surfaces; both export DLPack).  The run on the GPU is in tests/test_gpu_bench.py."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("_bench", ROOT / "bench.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _frames(n, shape, dtype=np.uint8):
    import torch

    rng = np.random.default_rng(5)
    return [torch.from_numpy(rng.integers(0, 256, shape).astype(dtype)) for _ in range(n)]


def test_small_batch_is_dumped_whole(bench, tmp_path):
    frames = _frames(3, (36, 64, 3))
    got = bench.dump_outputs(frames, tmp_path, 0, 1)
    assert got == {"dst": [3, 36, 64, 3]} and sorted(p.name for p in tmp_path.iterdir()) == ["dst.npy"]
    a = np.load(tmp_path / "dst.npy")
    assert a.dtype == np.float32 and np.array_equal(a, np.stack([f.numpy() for f in frames]).astype(np.float32))


def test_large_batch_is_sampled_within_the_budget(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 20)
    frames = _frames(4, (3, 180, 320), np.float32)                     # 4 x 691 200 B > 1 MiB: sampled
    got = bench.dump_outputs(frames, tmp_path / "a", 1, 2)              # rank 1 of 2: half the budget
    a, idx = np.load(tmp_path / "a" / "dst_rank1.npy"), np.load(tmp_path / "a" / "dst_rank1_index.npy")
    assert got == {"dst_rank1": [4, idx.size], "dst_rank1_index": [idx.size]}
    assert a.dtype == np.float32 and idx.dtype == np.float64 and a.shape == (4, idx.size)
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= (1 << 20) // 2 + 256
    assert idx[0] == 0 and idx[-1] == 3 * 180 * 320 - 1 and np.all(np.diff(idx) > 0) and idx.size > 1000
    want = np.stack([f.numpy().reshape(-1)[idx.astype(np.int64)] for f in frames])
    assert np.array_equal(a, want)
    # the same positions in every run
    bench.dump_outputs(frames, tmp_path / "b", 1, 2)
    assert np.array_equal(np.load(tmp_path / "b" / "dst_rank1_index.npy"), idx)


def test_full_is_an_option_that_is_off_by_default(bench, monkeypatch):
    """A plain `bench.py --gpus 1 --steps N --warmup W` only times its steps; --full asks for the rest."""
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2", "--full"])
    assert bench.parse().full is True
