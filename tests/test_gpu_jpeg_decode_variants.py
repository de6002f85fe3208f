"""Baseline JPEG decode on the GPU of files as other encoders write them (tests/jpeg_variant_files.py): every
downloaded surface equals tests/jpeg_decode_model.py byte for byte, which tests/test_jpeg_decode_variants_host.py pins
to Pillow on the same files.  RGB and Y for every file, and the raw format of its sampling where it has one."""
import numpy as np
import pytest

import jpeg_decode_model as dm
import jpeg_variant_files as vf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec(vali, gpu):
    return vali.PyNvJpegDecoder(gpu)


def download(vali, gpu, surface):
    host = np.zeros(surface.HostSize, np.uint8)
    ok, info = vali.PySurfaceDownloader(gpu).Run(surface, host)
    assert ok, info
    return host


def check(vali, gpu, dec, cases):
    """one call per output format over the files that have it; every surface against the model"""
    assert cases
    for fmt in ("RGB", "Y", "YUV444", "YUV422", "NV12"):
        sel = [c for c in cases if fmt in ("RGB", "Y") or c.raw == fmt]
        if not sel:
            continue
        surfaces, info = dec.Run([c.data for c in sel], vali.PixelFormat[fmt])
        assert info == vali.TaskExecInfo.SUCCESS, (fmt, info, dec.last_status)
        for c, s in zip(sel, surfaces):
            want = dm.surface_bytes(c.data, fmt)
            assert want is not None, c.name
            assert np.array_equal(download(vali, gpu, s), want), (c.name, fmt)


# ---- a ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", vf.A_SAMPLINGS)
def test_optimised_tables_from_pillow(vali, gpu, dec, sampling):
    pytest.importorskip("PIL.Image")
    cases = vf.group_a(sampling)
    assert len(cases) >= 25 and (sampling == "gray" or any(c.raw for c in cases))
    check(vali, gpu, dec, cases)


# ---- b ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", vf.B_SAMPLINGS)
@pytest.mark.parametrize("variant", vf.B_VARIANTS)
def test_hand_built_tables(vali, gpu, dec, variant, sampling):
    check(vali, gpu, dec, vf.group_b(variant, sampling))


# ---- c ----------------------------------------------------------------------------------------------------------------------
def test_marker_layouts(vali, gpu, dec):
    pytest.importorskip("PIL.Image")
    check(vali, gpu, dec, vf.group_c())


def test_equal_headers_different_entropy_data_in_one_call(vali, gpu):
    pytest.importorskip("PIL.Image")
    a, b = vf.equal_header_pair()
    fresh = vali.PyNvJpegDecoder(gpu)
    check(vali, gpu, fresh, [vf.Case("pair a", a, "NV12", True), vf.Case("pair b", b, "NV12", True),
                             vf.Case("pair a again", a, "NV12", True)])
    assert len(fresh._headers) == 1


# ---- d ----------------------------------------------------------------------------------------------------------------------
def test_unstuffer_boundaries(vali, gpu, dec):
    cases = vf.group_d()
    got = set()
    for c in cases:
        got |= vf.unstuff_props(c.data)
    assert got >= set(vf.UNSTUFF_PROPS), set(vf.UNSTUFF_PROPS) - got      # the files still pin every boundary
    check(vali, gpu, dec, cases)
    for c in cases:                                                         # and each alone: image 0 of its call
        check(vali, gpu, dec, [c._replace(raw=None)])


# ---- e ----------------------------------------------------------------------------------------------------------------------
def test_restart_interval_edges(vali, gpu, dec):
    cases = vf.group_e()
    want = {"420 48x32 R7": (7, 1), "420 48x32 R3": (3, 2), "420 48x32 R4": (4, 2), "420 48x32 R65535": (65535, 1),
            "420 48x32 DRI 5 then DRI 0": (0, 1), "gray 80x8 R1": (1, 10)}
    from vali_amd._native import shim

    for c in cases:
        info = shim.jpeg_parse(c.data)
        assert (info.restart_interval, info.segments) == want[c.name], c.name
    assert b"\xff\xd7" in cases[-1].data and cases[-1].data.count(b"\xff\xd0") >= 2          # RSTn wraps
    check(vali, gpu, dec, cases)


# ---- f ----------------------------------------------------------------------------------------------------------------------
def test_batch_of_300_and_one_truncated_file(vali, gpu, dec):
    pytest.importorskip("PIL.Image")
    cases = vf.group_f()
    assert len(cases) == vf.BATCH == 300 and {c.name.split()[2] for c in cases} == set(vf.jf.SAMPLINGS)
    files = [c.data for c in cases]
    want = {fmt: [dm.surface_bytes(f, fmt) for f in files] for fmt in ("RGB", "Y")}
    for fmt in ("RGB", "Y"):
        surfaces, info = dec.Run(files, vali.PixelFormat[fmt])
        assert info == vali.TaskExecInfo.SUCCESS, (fmt, dec.last_status)
        for k, s in enumerate(surfaces):
            assert np.array_equal(download(vali, gpu, s), want[fmt][k]), (cases[k].name, fmt)
    # the same call with file 271 truncated in its scan: all or nothing, and only that file is named
    bad = list(files)
    bad[vf.BATCH_BAD] = vf.truncated_in_scan(files[vf.BATCH_BAD])
    assert dm.decode(bad[vf.BATCH_BAD]) is None
    assert dec.Run(bad, vali.RGB) == ([], vali.TaskExecInfo.FAIL)
    assert [k for k, st in enumerate(dec.last_status) if st] == [vf.BATCH_BAD]
    surfaces = []
    for k, f in enumerate(files):
        info = dec.Info(f)
        s = vali.Surface.Make(vali.RGB, info.width, info.height, gpu)
        if k in (vf.BATCH_BAD - 1, vf.BATCH_BAD, vf.BATCH_BAD + 1):
            assert vali.PyFrameUploader(gpu).Run(np.full(s.HostSize, 0xC3, np.uint8), s)[0]
        surfaces.append(s)
    assert dec.RunInto(bad, surfaces) == (False, vali.TaskExecInfo.FAIL)
    assert [k for k, st in enumerate(dec.last_status) if st] == [vf.BATCH_BAD]
    assert np.all(download(vali, gpu, surfaces[vf.BATCH_BAD]) == 0xC3)
    for k in (vf.BATCH_BAD - 1, vf.BATCH_BAD + 1, 0, vf.BATCH - 1):           # its neighbours are decoded
        assert np.array_equal(download(vali, gpu, surfaces[k]), want["RGB"][k]), k


# ---- g ----------------------------------------------------------------------------------------------------------------------
def test_dynamic_range(vali, gpu, dec):
    pytest.importorskip("PIL.Image")
    cases = vf.group_g()
    assert [c.name for c in cases if not c.pillow] == ["16-bit tables x40", "16-bit tables all 65535", "extreme gray 16x8"]
    q = dm.parse(cases[-2].data)["q"]
    assert all(int(t.min()) == 65535 for t in q)
    check(vali, gpu, dec, cases)


def test_extreme_coefficients_from_the_writer(vali, gpu, dec):
    """DC differences of size 11 and AC values of sizes 10 to 15 at the int16 extremes: a writer file, no Pillow"""
    data = vf.extreme_stream()
    coefs = dm.entropy_decode(dm.parse(data))[0]
    assert coefs.max() == 32767 and coefs.min() == -32767
    check(vali, gpu, dec, [vf.Case("extreme gray 16x8", data, None, False)])
