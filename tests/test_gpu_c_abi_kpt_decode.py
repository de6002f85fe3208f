"""vali_kpt_decode and vali_pose_paint_points exercised from plain C (tests/c_abi/kpt_decode_client.c): planted float32
heatmaps decoded through similarities onto one packed RGB frame and drawn there in two calls, against the points, kpts and
frame tests/kpt_decode_model.py gives; the client also checks that every documented refusal comes."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import annotate_model as am
import kpt_decode_model as kd
import pose_cases as pc

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    lib = ROOT / "vali_amd" / "libvali_hip.so"
    exe = tmp_path_factory.mktemp("kpt_decode_client") / "kpt_decode_client"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "c_abi" / "kpt_decode_client.c"), "-o", str(exe), f"-L{lib.parent}", "-lvali_hip",
                    f"-Wl,-rpath,{lib.parent}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], check=True)
    return exe


def test_decode_and_draw_through_the_c_abi(tmp_path, gpu, client):
    w, h, m, p, hh, wh, cw, ch = 96, 80, 4, 5, 17, 13, 26, 34
    thr, thickness, diameter, alpha = 0.3, 3, 7, 160
    rng = np.random.default_rng(11)
    heat = (rng.standard_normal((m, p, hh, wh)) * 0.3 + 0.3).astype(np.float32)
    s, th = rng.uniform(0.8, 2.0, m), rng.uniform(-0.5, 0.5, m)
    mats = np.stack([s * np.cos(th), -s * np.sin(th), rng.uniform(5, 40, m), s * np.sin(th), s * np.cos(th),
                     rng.uniform(5, 25, m)], 1)
    rows = kd.matrix_rows([0] * m, mats)
    lcol, jcol = pc.LIMB_COLOURS[:3], pc.JOINT_COLOURS[:2]
    points, kpts = kd.decode([(w, h)], rows, 0, (cw, ch), heat=heat, thr=thr)
    assert (points[..., 3] == 3).sum() >= m * p // 2 and not np.isnan(kpts).any()
    frame = am.noise_frame("RGB", w, h, 60)
    want = [frame.copy()]
    assert kd.paint_points(want, "RGB", [(w, h)], points, m, pc.LIMBS, lcol, jcol, thickness, diameter, alpha) > 10
    files = {"frame": frame, "heat": heat, "matrices": rows, "limbs": np.asarray(pc.LIMBS, np.int32),
             "limb_colours": np.asarray(lcol, np.int32), "joint_colours": np.asarray(jcol, np.int32), "want": want[0],
             "want_points": points, "want_kpts": kpts}
    for name, a in files.items():
        (tmp_path / f"{name}.bin").write_bytes(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([str(client), *(str(v) for v in (w, h, m, p, hh, wh, cw, ch, thr, len(pc.LIMBS), thickness, diameter,
                                                        alpha)),
                        *(str(tmp_path / f"{name}.bin") for name in files), str(tmp_path / "got.bin"),
                        str(tmp_path / "points.bin"), str(tmp_path / "kpts.bin")], capture_output=True, text=True, timeout=120)
    if r.returncode == 6:
        got = np.fromfile(tmp_path / "points.bin", np.int32).reshape(points.shape)
        raise AssertionError(f"points differ at {np.argwhere(got != points)[:8]}")
    if r.returncode == 7:
        got = np.fromfile(tmp_path / "kpts.bin", np.float32).reshape(kpts.shape)
        raise AssertionError(f"kpts differ at {np.argwhere(got != kpts)[:8]}")
    if r.returncode == 5:
        got = np.fromfile(tmp_path / "got.bin", np.uint8)
        bad = np.flatnonzero(got != want[0])
        raise AssertionError(f"{bad.size} bytes differ, first at {bad[:8]}")
    assert r.returncode == 0, r.stderr + r.stdout
    assert r.stdout.startswith("ok ")
