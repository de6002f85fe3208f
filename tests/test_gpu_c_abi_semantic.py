"""vali_semantic_paint exercised from plain C (tests/c_abi/semantic_client.c): the first frame of the shared fixtures as
packed RGB, labelled and painted in one call, against the frame and the labels of tests/semantic_model.py; the client also
checks that the refusals come."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import semantic_cases as sc
import semantic_model as sm

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    lib = ROOT / "vali_amd" / "libvali_hip.so"
    exe = tmp_path_factory.mktemp("semantic_client") / "semantic_client"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "c_abi" / "semantic_client.c"), "-o", str(exe), f"-L{lib.parent}", "-lvali_hip",
                    f"-Wl,-rpath,{lib.parent}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], check=True)
    return exe


def test_paint_through_the_c_abi(tmp_path, gpu, client):
    c, (ws, hs), alpha = 19, (24, 20), 128
    w, h = sc.SIZES[0]
    logits = sc.logits(c, ws, hs)[:1]
    colours = sc.palette(7)
    frame = sc.noise_frames("RGB", seed=30)[0]
    want = [frame.copy()]
    maps = sm.apply(want, "RGB", sc.SIZES[:1], logits, sc.RECTS[:1], colours, alpha, sc.NET)
    assert len(np.unique(maps[0])) >= 5 and not np.array_equal(want[0], frame)
    files = {"frame": frame, "logits": logits, "rect": np.asarray(sc.RECTS[0], np.int32),
             "colours": np.asarray(colours, np.int32), "want": np.concatenate([want[0], maps[0].reshape(-1)])}
    for name, a in files.items():
        (tmp_path / f"{name}.bin").write_bytes(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([str(client), *(str(v) for v in (w, h, c, hs, ws, *sc.NET, len(colours), alpha)),
                        *(str(tmp_path / f"{name}.bin") for name in files), str(tmp_path / "got.bin")],
                       capture_output=True, text=True, timeout=120)
    if r.returncode == 5:
        got = np.fromfile(tmp_path / "got.bin", np.uint8)
        bad = np.flatnonzero(got != files["want"])
        raise AssertionError(f"{bad.size} bytes differ, first at {bad[:8]} (the frame has {frame.size} bytes)")
    assert r.returncode == 0, r.stderr + r.stdout
    assert r.stdout.startswith("ok ")
