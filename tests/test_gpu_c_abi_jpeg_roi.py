"""The region encoder exercised from plain C (tests/c_abi/jpeg_roi_client.c): vali_jpeg_plan_rois and
vali_jpeg_encode_rois on rectangles of one noise picture; the files equal the model's (tests/jpeg_roi_model.py)."""
import shutil
import subprocess
from pathlib import Path

import pytest

import jpeg_model as jm
import jpeg_roi_model as rm

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_c_client_encodes_rectangles(tmp_path, gpu):
    lib = ROOT / "vali_amd" / "libvali_hip.so"
    exe = tmp_path / "jpeg_roi_client"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "c_abi" / "jpeg_roi_client.c"), "-o", str(exe), f"-L{lib.parent}",
                    "-lvali_hip", f"-Wl,-rpath,{lib.parent}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"],
                   check=True)
    w, h = 168, 152
    host = jm.make_host(jm.RGB, w, h, "noise", seed=5)
    host.tofile(tmp_path / "in.rgb")
    rects = [(w - 1, h - 1, 1, 1), (21, 11, 136, 136), (5, 3, 17, 9), (0, 0, w, h), (7, 13, 16, 16)]
    for samp, (hs, vs), optimize in (("420", (2, 2), 0), ("444", (1, 1), 1)):
        prefix = tmp_path / f"out_{samp}_"
        r = subprocess.run([str(exe), str(tmp_path / "in.rgb"), str(w), str(h), "90", str(hs), str(vs), str(optimize),
                            str(prefix)] + [",".join(str(v) for v in r) for r in rects],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr + r.stdout
        assert r.stdout.split() == ["ok", str(len(rects))]
        for i, rect in enumerate(rects):
            got = Path(f"{prefix}{i}.jpg").read_bytes()
            assert got == rm.encode(jm.RGB, host, w, h, rect, 90, samp, bool(optimize)), (samp, optimize, i, rect)
