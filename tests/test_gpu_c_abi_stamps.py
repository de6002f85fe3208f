"""vali_annotate_batch_atlas exercised from plain C (tests/c_abi/stamp_client.c): two frames of different sizes, one NV12 and
one RGB case, stamps among the other kinds, against bytes tests/annotate_stamp_model.py wrote to a file."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import annotate_model as am
import annotate_stamp_model as sm
import postproc_model as pm

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
T = am.TILE
AW, AH = 97, 45


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    lib = ROOT / "vali_amd" / "libvali_hip.so"
    exe = tmp_path_factory.mktemp("stamp_client") / "stamp_client"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "c_abi" / "stamp_client.c"), "-o", str(exe), f"-L{lib.parent}", "-lvali_hip",
                    f"-Wl,-rpath,{lib.parent}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], check=True)
    return exe


@pytest.mark.parametrize("fmt", ["NV12", "RGB"])
def test_stamps_through_the_c_abi(tmp_path, gpu, client, fmt):
    sizes = [(2 * T + 2, T + 6), (T - 2, T + 2)]
    c, uv = am.pack_colour, sm.pack_uv
    atlas = np.random.default_rng(3).integers(0, 256, (AH, AW), dtype=np.uint8)
    rows = [(0, T - 9, T - 11, 30, 25, sm.STAMP, uv(5, 3), c(250, 10, 40, 140)), (1, 5, 7, 33, 21, am.PIXELATE, 8, 0),
            (0, 3, 3, 2 * T - 10, T - 2, am.BOX, 3, c(0, 255, 0)), (0, T + 1, 11, 50, 45, sm.STAMP, uv(60, 1), c(255, 255, 255)),
            (1, -8, T - 6, 2**31 - 1, 40, sm.STAMP, 0, c(20, 30, 255, 90)), (2, 0, 0, 9, 9, sm.STAMP, 0, c(1, 2, 3)),
            (1, 0, 0, 9, 9, sm.STAMP, uv(AW, 0), c(1, 2, 3)), (0, 2 * T - 3, 1, 9, 200, am.FILL, 0, c(77, 66, 55, 254)),
            (0, 2 * T - 5, 3, 9, 9, sm.STAMP, uv(AW - 4, AH - 3), c(9, 8, 7))]
    hosts = [am.noise_frame(fmt, w, h, 90 + i) for i, (w, h) in enumerate(sizes)]
    (tmp_path / "frames.bin").write_bytes(b"".join(x.tobytes() for x in hosts))
    (tmp_path / "marks.bin").write_bytes(np.asarray(rows, np.int64).astype(np.int32).tobytes())
    (tmp_path / "atlas.bin").write_bytes(atlas.tobytes())
    assert sm.apply(hosts, fmt, sizes, rows, pm.matrices()["601_JPEG"], atlas) == [0, 1, 2, 3, 4, 7, 8]
    (tmp_path / "want.bin").write_bytes(b"".join(x.tobytes() for x in hosts))
    r = subprocess.run([str(client), fmt.lower(), *(str(v) for s in sizes for v in s), str(tmp_path / "frames.bin"),
                        str(tmp_path / "marks.bin"), str(len(rows)), str(tmp_path / "want.bin"), str(tmp_path / "got.bin"),
                        str(tmp_path / "atlas.bin"), str(AW), str(AH)], capture_output=True, text=True, timeout=120)
    if r.returncode == 5:
        got, want = np.fromfile(tmp_path / "got.bin", np.uint8), np.concatenate(hosts)
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{bad.size} bytes differ, first at {bad[:8]}")
    assert r.returncode == 0, r.stderr + r.stdout
    assert r.stdout.startswith("ok ")
