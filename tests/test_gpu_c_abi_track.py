"""vali_track_update exercised from plain C (tests/c_abi/track_client.c): a sequence of six calls on one state, three
streams of four frames each, with all three outputs, against what tests/track_model.py wrote to a file for every call."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import track_cases as tc
import track_model as tm

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    lib = ROOT / "vali_amd" / "libvali_hip.so"
    exe = tmp_path_factory.mktemp("track_client") / "track_client"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "c_abi" / "track_client.c"), "-o", str(exe), f"-L{lib.parent}", "-lvali_hip",
                    f"-Wl,-rpath,{lib.parent}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], check=True)
    return exe


def test_a_sequence_through_the_c_abi(tmp_path, gpu, client):
    s, f, d, t, calls = 3, 4, 5, 65, 6
    colours = [tm.pack_colour(40, 255, 80), tm.pack_colour(255, 0, 0, 128), tm.pack_colour(1, 2, 3, 0)]
    rows = tc.scene(11, s, f, d, calls)
    tracks, clock = np.zeros((s * t, 16), np.int32), np.zeros((s, 4), np.int32)
    want, shown = [], 0
    for r in rows:
        tracks, clock, tracked, assoc = tm.update(r, tracks, clock, s, d, t, 0.3, 0.5, 2, 3, 0.5)
        want += [tracks, clock, tracked, assoc, tm.marks_of(tracked, colours, 2)]
        shown += int((tracked[:, 0] >= 0).sum())
    assert shown > 20 and (tracks[:, tm.MISSES] > 0).any()
    want = b"".join(a.astype(np.int32).tobytes() for a in want)
    (tmp_path / "dets.bin").write_bytes(b"".join(r.tobytes() for r in rows))
    (tmp_path / "want.bin").write_bytes(want)
    r = subprocess.run([str(client), *(str(v) for v in (s, f, d, t, calls)), str(tmp_path / "dets.bin"),
                        str(tmp_path / "want.bin"), str(tmp_path / "got.bin")], capture_output=True, text=True, timeout=120)
    if r.returncode == 5:
        got = np.fromfile(tmp_path / "got.bin", np.int32)
        bad = np.flatnonzero(got != np.frombuffer(want, np.int32))
        raise AssertionError(f"{bad.size} values differ, first at {bad[:8]}")
    assert r.returncode == 0, r.stderr + r.stdout
    assert r.stdout.startswith("ok ")
