"""The JPEG decoder exercised from plain C (tests/c_abi/jpeg_decode_client.c): vali_jpeg_parse,
vali_jpeg_decode_workspace_size and vali_jpeg_decode_batch on tests/golden/frame_0.jpg; the pixels equal Pillow's."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_c_client_decodes_frame0(tmp_path, gpu):
    from PIL import Image

    lib = ROOT / "vali_amd" / "libvali_hip.so"
    exe = tmp_path / "jpeg_decode_client"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "c_abi" / "jpeg_decode_client.c"), "-o", str(exe), f"-L{lib.parent}",
                    "-lvali_hip", f"-Wl,-rpath,{lib.parent}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"],
                   check=True)
    src = ROOT / "tests" / "golden" / "frame_0.jpg"
    r = subprocess.run([str(exe), str(src), str(tmp_path / "out.rgb")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    assert r.stdout.split() == ["ok", "848", "464"]
    got = np.fromfile(tmp_path / "out.rgb", np.uint8).reshape(464, 848, 3)
    assert np.array_equal(got, np.asarray(Image.open(src).convert("RGB")))
