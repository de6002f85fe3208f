"""vali_detect_select exercised from plain C (tests/c_abi/detect_client.c): one call with all four outputs on a float32
head of three frames, one of them emptied by its record, against rows tests/detect_model.py wrote to a file."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import detect_model as dm
from test_detect_host import random_head

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    lib = ROOT / "vali_amd" / "libvali_hip.so"
    exe = tmp_path_factory.mktemp("detect_client") / "detect_client"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "c_abi" / "detect_client.c"), "-o", str(exe), f"-L{lib.parent}", "-lvali_hip",
                    f"-Wl,-rpath,{lib.parent}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], check=True)
    return exe


def test_select_through_the_c_abi(tmp_path, gpu, client):
    n, k, c, t, d = 3, 257, 5, 64, 12
    rect = (4, 6, 320, 200, 10, 20, 160, 100)
    boxes, scores, _ = random_head(3, n, k, c, "xyxy", rect)
    rects = np.asarray([rect, (4, 6, 320, 200, 10, 20, 160, 0), (100, 50, 77, 33, 10, 20, 160, 100)], np.int32)
    colours = [dm.pack_colour(40, 255, 80), dm.pack_colour(255, 0, 0, 128), dm.pack_colour(1, 2, 3, 0)]
    dets, counts = dm.select(boxes, scores, rects, 0.25, 0.45, False, "xyxy", t, d)
    assert counts[0] > 0 and counts[1] == 0 and counts[2] > 0
    want = b"".join(a.astype(np.int32).tobytes() for a in (dets, counts, dm.rois_of(dets, (0, 0, 224, 224)),
                                                           dm.marks_of(dets, colours, 2)))
    (tmp_path / "boxes.bin").write_bytes(boxes.tobytes())
    (tmp_path / "scores.bin").write_bytes(scores.tobytes())
    (tmp_path / "rects.bin").write_bytes(rects.tobytes())
    (tmp_path / "want.bin").write_bytes(want)
    r = subprocess.run([str(client), *(str(v) for v in (n, k, c, t, d)), str(tmp_path / "boxes.bin"),
                        str(tmp_path / "scores.bin"), str(tmp_path / "rects.bin"), str(tmp_path / "want.bin"),
                        str(tmp_path / "got.bin")], capture_output=True, text=True, timeout=120)
    if r.returncode == 5:
        got = np.fromfile(tmp_path / "got.bin", np.int32)
        bad = np.flatnonzero(got != np.frombuffer(want, np.int32))
        raise AssertionError(f"{bad.size} values differ, first at {bad[:8]}")
    assert r.returncode == 0, r.stderr + r.stdout
    assert r.stdout.startswith("ok ")
