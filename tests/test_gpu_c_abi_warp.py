"""vali_warp_fit and vali_warp_tensor exercised from plain C (tests/c_abi/warp_client.c): one NV12 frame, three detections
with five landmarks each, fitted and sampled into a float32 tensor with device arrays the client uploads itself, against the
matrices and the crops tests/warp_model.py gives; the client also checks that the refusals come."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import annotate_model as am
import pose_cases as pc
import warp_model as wm

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    lib = ROOT / "vali_amd" / "libvali_hip.so"
    exe = tmp_path_factory.mktemp("warp_client") / "warp_client"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "c_abi" / "warp_client.c"), "-o", str(exe), f"-L{lib.parent}", "-lvali_hip",
                    f"-Wl,-rpath,{lib.parent}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], check=True)
    return exe


def test_fit_and_sample_through_the_c_abi(tmp_path, gpu, client):
    from vali_amd import tasks

    (w, h), rect, K, P, D, canvas = (64, 48), (0, 0, 64, 48, 0, 4, 32, 24), 40, 5, 3, (33, 9)
    thr, min_points = 0.5, 2
    norm = (2.0, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    csc = tasks.CSC_NPP_709CSC
    template = np.asarray([(u * 33 / 112, v * 9 / 112) for u, v in wm.ARCFACE_112], np.float32)
    kpts = pc.kpts(P, "float32", 3, 3, 1, K, [(w, h)], [rect])
    dets = np.asarray([(0, 5, 7, 40, 30, 0, 0x3F000000, 3), (0, 20, 10, 30, 30, 0, 0x3F000000, 39),
                       (1, 5, 7, 40, 30, 0, 0x3F000000, 4)], np.int32)          # the last one is skipped
    frame = am.noise_frame("NV12", w, h, 77)
    rows = wm.fit([(w, h)], dets, D, kpts, [rect], template, thr, min_points)
    assert rows[:, 0].tolist() == [0, 0, -1]
    want, inside = wm.warp([frame], "NV12", [(w, h)], rows, canvas, norm, (30, 60, 90), csc)
    assert inside[:2].mean() > 0.3 and not inside[2].any()
    params = np.zeros(16, np.float32)
    params[:6], params[8], params[9:12], params[12:15] = csc, norm[0], norm[1], norm[2]
    files = {"frame": frame, "kpts": kpts, "dets": dets, "rect": np.asarray(rect, np.int32), "template": template,
             "params": params, "want_rows": rows, "want": want}
    for name, a in files.items():
        (tmp_path / f"{name}.bin").write_bytes(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([str(client), *(str(v) for v in (w, h, K, P, D, canvas[0], canvas[1], thr, min_points)),
                        *(str(tmp_path / f"{name}.bin") for name in files), str(tmp_path / "got_rows.bin"),
                        str(tmp_path / "got.bin")], capture_output=True, text=True, timeout=120)
    if r.returncode == 6:
        got = np.fromfile(tmp_path / "got_rows.bin", np.int32).reshape(rows.shape)
        raise AssertionError(f"matrices differ at {np.argwhere(got != rows)[:8].tolist()}: {got.tolist()} != {rows.tolist()}")
    if r.returncode == 5:
        got = np.fromfile(tmp_path / "got.bin", np.float32).reshape(want.shape)
        bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
        raise AssertionError(f"{len(bad)} elements differ, first at {bad[:6].tolist()}")
    assert r.returncode == 0, r.stderr + r.stdout
    assert r.stdout.startswith("ok ")
