"""Baseline JPEG decode on the GPU of streams built against its parallel entropy decode (tests/jpeg_hostile_files.py):
streams that never synchronise, blocks longer than a subsequence, thousands of restart segments, segments that end on
subsequence and workgroup boundaries, code words in the last bit of a subsequence.  Every downloaded surface equals
tests/jpeg_decode_model.py byte for byte; tests/test_jpeg_hostile_host.py pins the model to Pillow on these files and
asserts that each file has the property it is named for."""
import numpy as np
import pytest

import jpeg_decode_model as dm
import jpeg_hostile_files as hf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec(vali, gpu):
    return vali.PyNvJpegDecoder(gpu)


def download(vali, gpu, surface):
    host = np.zeros(surface.HostSize, np.uint8)
    ok, info = vali.PySurfaceDownloader(gpu).Run(surface, host)
    assert ok, info
    return host


def run(vali, gpu, dec, files, fmt):
    surfaces, info = dec.Run(files, vali.PixelFormat[fmt])
    assert info == vali.TaskExecInfo.SUCCESS, (fmt, info, dec.last_status)
    return [download(vali, gpu, s) for s in surfaces]


def check(vali, gpu, dec, cases):
    """every file alone, in Y, RGB and the raw format of its sampling, against the model"""
    assert cases
    for c in cases:
        for fmt in ("Y", "RGB", c.raw):
            if fmt is None:
                continue
            want = dm.surface_bytes(c.data, fmt)
            assert want is not None, c.name
            assert np.array_equal(run(vali, gpu, dec, [c.data], fmt)[0], want), (c.name, fmt)


def test_never_synchronising_streams(vali, gpu, dec):
    """every seam walk of k_jd_seams runs to the end of its workgroup and corrects tail; k_jd_sync loops 255 times"""
    check(vali, gpu, dec, hf.group_a())


def test_blocks_longer_than_a_subsequence(vali, gpu, dec):
    check(vali, gpu, dec, hf.group_b())


@pytest.mark.parametrize("part", ["segments", "lengths", "1.6 workgroups", "last bit"])
def test_restart_structure(vali, gpu, dec, part):
    cases = [c for c in hf.group_c() if part in c.name]
    assert len(cases) == {"segments": 3, "lengths": 2, "1.6 workgroups": 1, "last bit": len(hf.LAST_BIT_SEEDS)}[part]
    check(vali, gpu, dec, cases)


def test_batch_in_two_orders_equals_single_calls_and_the_model(vali, gpu, dec):
    pytest.importorskip("PIL.Image")
    cases = hf.group_d()
    for fmt in ("RGB", "Y"):
        want = [dm.surface_bytes(c.data, fmt) for c in cases]
        single = [run(vali, gpu, dec, [c.data], fmt)[0] for c in cases]
        for order in (list(range(len(cases))), list(range(len(cases)))[::-1]):
            got = run(vali, gpu, dec, [cases[i].data for i in order], fmt)
            for g, i in zip(got, order):
                assert np.array_equal(g, single[i]), (fmt, cases[i].name, order[0])
                assert np.array_equal(g, want[i]), (fmt, cases[i].name, order[0])


def test_corrupt_twin_fails_alone_and_leaves_its_destination(vali, gpu, dec):
    """the decoder's defined error path: a run past 63 in the last workgroup of a stream that never synchronises"""
    import torch

    good, bad = hf.corrupt_pair()
    assert dm.decode(bad) is None
    before, after = hf.group_b()[0].data, hf.group_c()[3].data
    want = [dm.surface_bytes(f, "RGB") for f in (before, good, after)]
    assert dec.Run([before, bad, after], vali.RGB) == ([], vali.TaskExecInfo.FAIL)
    assert [k for k, st in enumerate(dec.last_status) if st] == [1]

    info = dec.Info(bad)
    w, h = info.width, info.height
    big = torch.full((h + 8, 3 * w + 64), 0xC3, dtype=torch.uint8, device=f"cuda:{gpu}")
    torch.cuda.synchronize()

    def surfaces():
        view = vali.Surface.from_dlpack(torch.utils.dlpack.to_dlpack(big[4:4 + h, 16:16 + 3 * w]))
        out = [vali.Surface.Make(vali.RGB, dec.Info(f).width, dec.Info(f).height, gpu) for f in (before, after)]
        return [out[0], view, out[1]]

    dst = surfaces()
    assert dec.RunInto([before, bad, after], dst) == (False, vali.TaskExecInfo.FAIL)
    assert [k for k, st in enumerate(dec.last_status) if st] == [1]
    torch.cuda.synchronize()
    assert np.all(big.cpu().numpy() == 0xC3)
    for k in (0, 2):                                                            # its neighbours are decoded
        assert np.array_equal(download(vali, gpu, dst[k]), want[k]), k
    # the same batch with the good twin in its place
    dst = surfaces()
    ok, res = dec.RunInto([before, good, after], dst)
    assert ok, (res, dec.last_status)
    torch.cuda.synchronize()
    got = big.cpu().numpy()
    assert np.array_equal(got[4:4 + h, 16:16 + 3 * w].reshape(-1), want[1])
    mask = np.ones_like(got, bool)
    mask[4:4 + h, 16:16 + 3 * w] = False
    assert np.all(got[mask] == 0xC3)


def test_one_decoder_decodes_a_hostile_file_twice(vali, gpu):
    """the second call finds the workspace as the first one left it, a noise file of the same size having used it in
    between: entries, counts, heads and tails are all written anew"""
    fresh = vali.PyNvJpegDecoder(gpu)
    data = hf.group_a()[0].data
    first = run(vali, gpu, fresh, [data], "RGB")[0]
    noise = run(vali, gpu, fresh, [hf.noise_twin()], "RGB")[0]
    second = run(vali, gpu, fresh, [data], "RGB")[0]
    assert np.array_equal(first, second)
    assert np.array_equal(first, dm.surface_bytes(data, "RGB"))
    assert np.array_equal(noise, dm.surface_bytes(hf.noise_twin(), "RGB"))
