"""vali_pose_workspace_size and vali_pose_paint exercised from plain C (tests/c_abi/pose_client.c): the first frame of the
shared fixtures as packed RGB, its four skeletons drawn in one call, against the frame and the points tests/pose_model.py
gives; the client also checks that the refusals come."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pose_cases as pc
import pose_model as po

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    lib = ROOT / "vali_amd" / "libvali_hip.so"
    exe = tmp_path_factory.mktemp("pose_client") / "pose_client"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "c_abi" / "pose_client.c"), "-o", str(exe), f"-L{lib.parent}", "-lvali_hip",
                    f"-Wl,-rpath,{lib.parent}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], check=True)
    return exe


def test_draw_through_the_c_abi(tmp_path, gpu, client):
    thr, thickness, diameter, alpha = pc.THR, 3, 7, 160
    w, h = pc.SIZES[0]
    kpts = pc.kpts()[:1]
    dets = np.asarray(pc.PLACEMENTS[:pc.D], np.int32)
    lcol, jcol = pc.LIMB_COLOURS[:3], pc.JOINT_COLOURS[:2]
    frame = pc.noise_frames("RGB", seed=30)[0]
    want = [frame.copy()]
    points, drawn = po.apply(want, "RGB", pc.SIZES[:1], dets, pc.D, kpts, pc.RECTS[:1], pc.LIMBS, lcol, jcol, thr, thickness,
                             diameter, alpha)
    assert {d[0] for d in drawn} == set(range(pc.D)) and not np.array_equal(want[0], frame)
    files = {"frame": frame, "kpts": kpts, "dets": dets, "rect": np.asarray(pc.RECTS[0], np.int32),
             "limbs": np.asarray(pc.LIMBS, np.int32), "limb_colours": np.asarray(lcol, np.int32),
             "joint_colours": np.asarray(jcol, np.int32), "want": want[0], "want_points": points}
    for name, a in files.items():
        (tmp_path / f"{name}.bin").write_bytes(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([str(client), *(str(v) for v in (w, h, pc.K, pc.P, pc.D, len(pc.LIMBS), thr, thickness, diameter, alpha)),
                        *(str(tmp_path / f"{name}.bin") for name in files), str(tmp_path / "got.bin"),
                        str(tmp_path / "points.bin")], capture_output=True, text=True, timeout=120)
    if r.returncode == 5:
        got = np.fromfile(tmp_path / "got.bin", np.uint8)
        bad = np.flatnonzero(got != want[0])
        raise AssertionError(f"{bad.size} bytes differ, first at {bad[:8]}")
    if r.returncode == 6:
        got = np.fromfile(tmp_path / "points.bin", np.int32).reshape(points.shape)
        raise AssertionError(f"points differ at {np.argwhere(got != points)[:8]}")
    assert r.returncode == 0, r.stderr + r.stdout
    assert r.stdout.startswith("ok ")
