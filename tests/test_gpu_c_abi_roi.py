"""The region entry points exercised from plain C (tests/c_abi/roi_client.c): two NV12 frames of different sizes,
vali_nv12_preproc_roi_batch with padding into RGB_32F_PLANAR and vali_nv12_preproc_roi without padding into BGR;
the outputs are compared with the CPU oracle bit for bit."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from conftest import make_nv12

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CSC_709CSC = (16.0, 1.164, 1.793, -0.213, -0.533, 2.112)


def crop_nv12(host, sh, x, y, w, h):
    return np.ascontiguousarray(np.concatenate([host[y:y + h, x:x + w], host[sh + y // 2:sh + (y + h) // 2, x:x + w]]))


def oracle_u8(oracle, host, sw, sh, crop, dw, dh, fmt):
    x, y, w, h = crop
    nv = crop_nv12(host, sh, x, y, w, h)
    if (w, h) != (dw, dh):
        nv = oracle.resize_surface(nv.reshape(-1), "NV12", w, h, dw, dh).reshape(dh * 3 // 2, dw)
    return oracle.nv12_to_rgb(nv, dw, dh, oracle.csc_from_tuple(CSC_709CSC), fmt).reshape(dh, dw, 3)


def normalise(q):
    """(H, W, 3) u8 -> (3, H, W) float32: ((q / 255) / 1 - mean) / std"""
    x = (q.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1) / np.float32(1.0)
    return ((x - np.asarray(MEAN, np.float32)[:, None, None]) / np.asarray(STD, np.float32)[:, None, None]).astype(
        np.float32)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_c_client_regions(tmp_path, gpu, oracle):
    lib = ROOT / "vali_amd" / "libvali_hip.so"
    exe = tmp_path / "roi_client"
    subprocess.run(["gcc", "-std=c99", "-O1", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "c_abi" / "roi_client.c"),
                    "-o", str(exe), f"-L{lib.parent}", "-lvali_hip", f"-Wl,-rpath,{lib.parent}",
                    "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], check=True)
    wa, ha, wb, hb, cw, ch = 640, 360, 320, 240, 224, 224
    a, b = make_nv12(wa, ha, 21), make_nv12(wb, hb, 22)
    (tmp_path / "a.nv12").write_bytes(a.tobytes())
    (tmp_path / "b.nv12").write_bytes(b.tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "a.nv12"), str(wa), str(ha), str(tmp_path / "b.nv12"), str(wb), str(hb),
                        str(cw), str(ch), str(tmp_path / "batch.f32"), str(tmp_path / "single.bgr")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    assert r.stdout.startswith("ok ")

    got = np.fromfile(tmp_path / "batch.f32", np.float32).reshape(3, 3, ch, cw)
    pad = normalise(np.full((1, 1, 3), 114, np.uint8))[:, 0, 0]
    items = [(a, wa, ha, (0, 0, wa, ha), (0, ch // 4, cw, ch // 2)),
             (b, wb, hb, (2, 2, wb - 4, hb // 2), (2, 0, cw - 4, ch)),
             (a, wa, ha, (wa // 2, ha // 2, wa // 4, ha // 4), (6, 10, 96, 64))]
    for i, (host, sw, sh, crop, (x, y, w, h)) in enumerate(items):
        want = np.empty((3, ch, cw), np.float32)
        want[:] = pad[:, None, None]
        want[:, y:y + h, x:x + w] = normalise(oracle_u8(oracle, host, sw, sh, crop, w, h, "RGB"))
        assert np.array_equal(got[i].view(np.uint32), want.view(np.uint32)), i

    single = np.fromfile(tmp_path / "single.bgr", np.uint8).reshape(ch, cw, 3)
    want = np.full((ch, cw, 3), 0x5A, np.uint8)
    x, y, w, h = 2, 4, cw // 2, ch // 2
    want[y:y + h, x:x + w] = oracle_u8(oracle, b, wb, hb, (wb // 4, hb // 4, wb // 2, hb // 2), w, h, "BGR")
    assert np.array_equal(single, want)
