"""vali_tensor_to_surfaces exercised from plain C (tests/c_abi/postproc_client.c), with chroma rounding made visible: the
matrix Y = (0, 1, 0, 0), U = (0, 0, 1, 0.5), V = (1, 0, 0, 0.25) puts every 2 x 2 mean of U on k / 4 + 0.5 and of V on
k / 4 + 0.25, on or beside a tie.  A kernel that averaged rounded values, summed in another association or rounded
half away from zero writes other bytes.  Compared with the CPU oracle bit for bit."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import postproc_model as pm

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
ROWS = ((0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.5), (1.0, 0.0, 0.0, 0.25))


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    lib = ROOT / "vali_amd" / "libvali_hip.so"
    exe = tmp_path_factory.mktemp("postproc_client") / "postproc_client"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "c_abi" / "postproc_client.c"), "-o", str(exe), f"-L{lib.parent}", "-lvali_hip",
                    f"-Wl,-rpath,{lib.parent}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], check=True)
    return exe


# 16 * 65 + 2: more than one wave and a ragged tail (the misaligned store forms); 32: whole strips (non-temporal stores)
@pytest.mark.parametrize("size", [(16 * 65 + 2, 6), (32, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_chroma_rounding_through_the_c_abi(tmp_path, gpu, oracle, client, size):
    w, h = size
    n = 3
    rng = np.random.default_rng(w)
    p = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    # make sure of the extremes: blocks whose sums are 0, 1020 and on every residue mod 4
    p[0, :2, :8] = np.array([[0, 0, 0, 0, 255, 255, 255, 255], [0, 0, 1, 0, 255, 255, 254, 255]], np.uint8)[..., None]
    (tmp_path / "t.u8").write_bytes(np.ascontiguousarray(p.transpose(0, 3, 1, 2)).tobytes())
    r = subprocess.run([str(client), str(tmp_path / "t.u8"), str(n), str(w), str(h), str(tmp_path / "o.yuv420"),
                        str(tmp_path / "o.nv12")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    assert r.stdout.startswith("ok ")
    ibytes = w * h * 3 // 2
    got420 = np.fromfile(tmp_path / "o.yuv420", np.uint8).reshape(n, ibytes)
    gotnv = np.fromfile(tmp_path / "o.nv12", np.uint8).reshape(n, ibytes)
    ties = 0
    for i in range(n):
        want = pm.from_rgb(oracle, p[i], "YUV420", ROWS)
        assert np.array_equal(want, pm.numpy_yuv(p[i], ROWS, "YUV420"))
        assert np.array_equal(got420[i], want), (i, np.flatnonzero(got420[i] != want)[:5])
        assert np.array_equal(gotnv[i], pm.from_rgb(oracle, p[i], "NV12", ROWS)), i
        b = p[i, :, :, 2].astype(np.int64)
        s = b[0::2, 0::2] + b[0::2, 1::2] + b[1::2, 0::2] + b[1::2, 1::2]
        ties += int(((s % 4) == 0).sum())
        # Y is G, untouched
        assert np.array_equal(got420[i][:w * h].reshape(h, w), p[i, :, :, 1])
    assert ties >= 10                      # exact ties were met
