"""vali_mask_workspace_size and vali_mask_paint exercised from plain C (tests/c_abi/mask_client.c): the first frame of the
shared fixtures as packed RGB, its four masks painted in one call, against the frame tests/mask_model.py painted; the
client also checks that the refusals come."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mask_cases as mc
import mask_model as mm

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    lib = ROOT / "vali_amd" / "libvali_hip.so"
    exe = tmp_path_factory.mktemp("mask_client") / "mask_client"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "c_abi" / "mask_client.c"), "-o", str(exe), f"-L{lib.parent}", "-lvali_hip",
                    f"-Wl,-rpath,{lib.parent}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], check=True)
    return exe


def test_paint_through_the_c_abi(tmp_path, gpu, client):
    m, (wp, hp), alpha = 5, (24, 20), 128
    w, h = mc.SIZES[0]
    protos, coeffs = mc.protos(m, wp, hp)[:1], mc.coeffs(m)[:1]
    dets = np.asarray(mc.PLACEMENTS[:mc.D], np.int32)
    frame = mc.noise_frames("RGB", seed=30)[0]
    want = [frame.copy()]
    drawn = mm.apply(want, "RGB", mc.SIZES[:1], dets, mc.D, protos, coeffs, mc.RECTS[:1], mc.COLOURS, alpha, mc.NET)
    assert len(drawn) == mc.D and not np.array_equal(want[0], frame)
    files = {"frame": frame, "protos": protos, "coeffs": coeffs, "dets": dets, "rect": np.asarray(mc.RECTS[0], np.int32),
             "colours": np.asarray(mc.COLOURS, np.int32), "want": want[0]}
    for name, a in files.items():
        (tmp_path / f"{name}.bin").write_bytes(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([str(client), *(str(v) for v in (w, h, m, hp, wp, mc.K, mc.D, *mc.NET, alpha)),
                        *(str(tmp_path / f"{name}.bin") for name in files), str(tmp_path / "got.bin")],
                       capture_output=True, text=True, timeout=120)
    if r.returncode == 5:
        got = np.fromfile(tmp_path / "got.bin", np.uint8)
        bad = np.flatnonzero(got != want[0])
        raise AssertionError(f"{bad.size} bytes differ, first at {bad[:8]}")
    assert r.returncode == 0, r.stderr + r.stdout
    assert r.stdout.startswith("ok ")
