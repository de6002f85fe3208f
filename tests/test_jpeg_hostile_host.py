"""CPU side of the hostile decoder files (tests/jpeg_hostile_files.py): every file parses, has the structural property
it was built for (measured by the plain Python simulation of the synchronisation, never by the GPU), decodes in the
numpy model, and -- families A, C and D -- equals Pillow's libjpeg-turbo byte for byte, so that the GPU test compares
with a trusted reference.  The conditions that keep a wrong decode from hiding are asserted here: no two blocks of a
file decode to the same samples, and few samples sit at 0 or 255.

Run as a script, it prints the measured figures of every file."""
import io

import numpy as np
import pytest

import jpeg_decode_model as dm
import jpeg_hostile_files as hf

GROUPS = {"a": hf.group_a, "b": hf.group_b, "c": hf.group_c, "d": hf.group_d}


def shim():
    from vali_amd._native import shim as s

    return s


def pillow_rgb(data):
    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def pillow_y(data):
    from PIL import Image

    im = Image.open(io.BytesIO(data))
    im.draft("L", im.size)
    return np.asarray(im.convert("L"))


def case(group, part):
    return next(c for c in GROUPS[group]() if part in c.name)


# ---- every file parses and decodes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(GROUPS))
def test_every_file_parses_as_the_model_reads_it(group):
    if group == "d":
        pytest.importorskip("PIL.Image")
    s = shim()
    for c in GROUPS[group]():
        want, got = dm.parse(c.data), s.jpeg_parse(c.data)
        mcux, mcuy, bpm = dm.geometry(want)
        assert (got.width, got.height, got.components, got.mcux, got.mcuy) == (want["w"], want["h"], want["nc"], mcux,
                                                                             mcuy), c.name
        assert (got.h_samp, got.v_samp) == (want["H"], want["V"]) and bpm == hf.sim(c.data).bpm, c.name
        assert got.restart_interval == want["ri"] and got.segments == hf.sim(c.data).nseg, c.name
        assert c.data[got.data_offset:got.data_offset + got.data_len] == want["data"], c.name


@pytest.mark.parametrize("group", list(GROUPS))
def test_model_decodes_every_file_and_equals_pillow(group):
    """B's coefficients lie beyond the range in which libjpeg-turbo's C and SIMD paths agree:
    there the model alone is the reference"""
    pytest.importorskip("PIL.Image")
    for c in GROUPS[group]():
        rgb, y = dm.decode(c.data, "RGB"), dm.decode(c.data, "Y")
        assert rgb is not None and y is not None, c.name
        assert c.pillow == ("long blocks" not in c.name)
        if c.pillow:
            assert np.array_equal(rgb, pillow_rgb(c.data)), c.name
            assert np.array_equal(y, pillow_y(c.data)), c.name


def test_only_the_corrupt_file_is_corrupt():
    good, bad = hf.corrupt_pair()
    assert dm.decode(good) is not None and dm.decode(bad) is None
    assert shim().jpeg_parse(bad).data_len == shim().jpeg_parse(good).data_len
    diff = [i for i, (x, y) in enumerate(zip(good, bad)) if x != y]
    assert len(diff) == 1 and bin(good[diff[0]] ^ bad[diff[0]]).count("1") == 1
    # the flipped bit lies in the last workgroup of subsequences
    s = hf.sim(good)
    a = len(good) - 2 - s.seg_start[-1] // 8
    assert (diff[0] - a) * 8 // hf.SUB_BITS // hf.GROUP == s.ngroups - 1 >= 3


# ---- the conditions on the inputs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["a", "b", "c"])
def test_no_two_blocks_are_equal_and_few_samples_are_saturated(group):
    """a block written to the wrong place shows: every block of a file is unlike every other, so the model's output
    with two blocks swapped is not the model's output.  B (coefficients of size 10 and 11) is exempt from the limit
    on saturated samples"""
    for c in GROUPS[group]():
        blocks = hf.model_blocks(c.data)
        assert len(np.unique(blocks, axis=0)) == len(blocks), c.name
        swapped = blocks.copy()
        swapped[[0, len(blocks) // 2]] = swapped[[len(blocks) // 2, 0]]
        assert not np.array_equal(swapped, blocks), c.name
        if group != "b":
            assert hf.saturated_share(c.data) <= 0.25, c.name


# ---- A ------------------------------------------------------------------------------------------------------------------------
def test_never_synchronising_files():
    gray, c420 = hf.group_a()
    for c, min_groups in ((gray, 4), (c420, 3)):
        s = hf.sim(c.data)
        assert s.nseg == 1 and s.ngroups >= min_groups and s.nsub > 512, c.name
        assert hf.never_synchronises(c.data) == (True, True, True), c.name
        seams = s.seams()
        assert len(seams) == s.ngroups - 1
        assert any(x["delta"] != 0 for x in seams if x["walked"] == hf.GROUP), seams     # tail is really corrected
        assert hf.figures(c.data)["never"] > 0.9
        assert sum(g != x for g, x in zip(s.guess_cnt, s.exact_cnt)) > s.nsub // 20     # guessed and exact block counts
    assert hf.sim(c420.data).bpm == 6 and any(st[1] for st in hf.sim(c420.data).entry)      # c is part of the state


def test_noise_of_the_same_size_fails_the_properties_of_a():
    """the support module is sensitive: the Annex K q100 noise file of A's size has seams too, but its guessed
    decodes meet the sequential one within tens of subsequences (or reach the end of the data first), so no seam is
    walked to its end and k_jd_sync's loop stops early"""
    data = hf.noise_twin()
    s = hf.sim(data)
    assert s.ngroups >= 3 and len(s.seams()) == s.ngroups - 1
    assert hf.never_synchronises(data)[:2] == (False, False)
    assert all(x["walked"] < 64 and not x["to_end"] for x in s.seams())
    ups = [(j,) + s.catch_up(j) for j in range(s.nsub) if s.sub_t[j] > 0]
    assert all(met or j + n == s.nsub for j, n, met in ups) and max(n for _, n, _ in ups) <= 64


# ---- B ------------------------------------------------------------------------------------------------------------------------
def test_blocks_longer_than_a_subsequence():
    """Two consecutive subsequences without a block end cannot exist: a block is at most 64 code words of at most
    31 bits, 1984 bits, and two subsequences are 2048.  What a block of 1665 bits does reach is asserted: many
    subsequences without a block end, one of them the first of a workgroup, and the run of 1 is the longest"""
    c, = hf.group_b()
    s = hf.sim(c.data)
    info = dm.parse(c.data)
    coefs = dm.entropy_decode(info)[0].reshape(-1, 64)
    assert len(coefs) == 289 and np.abs(coefs[1:, 1:]).min() >= 512 and np.abs(np.diff(coefs[:, 0])).min() >= 1024
    assert all(len(code) == 16 for code, sym in info["dc"][0].items() if sym == 11)
    assert all(len(code) == 16 for code, sym in info["ac"][0].items() if sym == 0x0A)
    assert s.seg_start[-1] > 288 * 1665 and 450 <= s.nsub <= 480 and len(s.seams()) == 1
    empty, first = hf.long_block_props(c.data)
    assert len(empty) > 100 and first == [hf.GROUP], (len(empty), first)
    assert s.longest_gap() == 1
    assert hf.search_b_first() == hf.B_FIRST


# ---- C ------------------------------------------------------------------------------------------------------------------------
def test_more_segments_than_one_trip_of_the_unstuffer():
    for part, segments, bpm in (("1089", 1089, 1), ("2116", 2116, 1), ("1056", 1056, 6)):
        s = hf.sim(case("c", part).data)
        assert (s.nseg, s.bpm) == (segments, bpm) and s.nsub == s.nseg and not s.seams()


def test_segment_lengths_on_subsequence_boundaries():
    small = hf.sim(case("c", "m 1 2").data)
    large = hf.sim(case("c", "m 256").data)
    assert small.segment_bits() == [1024, 1016, 1032, 2048, 2040, 2056]
    assert large.segment_bits() == [1024 * 256, 1024 * 256 + 8, 1024 * 256 - 8]
    assert large.seg_sub == [0, 256, 513, 769]
    # the m = 256 segment fills workgroup 0: the next segment starts on lane 0 of workgroup 1, which is no seam
    assert large.sub_t[hf.GROUP] == 0 and [x["group"] for x in large.seams()] == [2, 3]
    for s in (small, large):                       # no padding bits: the last code word ends with its segment
        for seg in range(s.nseg):
            assert s.exit[s.seg_sub[seg + 1] - 1][0] == s.seg_start[seg + 1]


def test_segments_of_one_and_a_half_workgroups():
    s = hf.sim(case("c", "1.6").data)
    seams = s.seams()
    assert s.nseg == 2 and [x["group"] for x in seams] == [1, 2, 3]
    assert {x["tail_is_s"] for x in seams} == {True, False}
    # workgroups 1, 2 and 3 in segment 1: head of 3 chains over the corrected tail of 2
    assert [x["segment"] for x in seams] == [0, 1, 1] and seams[2]["chained"] and seams[1]["tail_is_s"]
    assert seams[1]["walked"] == hf.GROUP and seams[1]["delta"] != 0
    assert all(x["to_end"] and x["differs"] for x in seams)
    assert s.sub_seg[hf.GROUP] == 0 and s.sub_seg[2 * hf.GROUP - 1] == 1       # a segment ends inside workgroup 1


def test_code_words_in_the_last_bit_at_every_alignment():
    got = set()
    for c in hf.group_c():
        if "last bit" in c.name:
            got |= hf.sim(c.data).last_bit_alignments()
    assert got == {0, 1, 2, 3}
    assert hf.search_last_bit_seeds() == (list(hf.LAST_BIT_SEEDS), set())


# ---- D ------------------------------------------------------------------------------------------------------------------------
def test_batch_mixes_workgroups_and_single_subsequences():
    pytest.importorskip("PIL.Image")
    subs = [hf.sim(c.data).nsub for c in hf.group_d()]
    assert subs[0] == subs[-1] == 1 and max(subs) > 3 * hf.GROUP, subs
    assert sum(1 for n in subs if n == 1) >= 3 and sum(1 for n in subs if n > hf.GROUP) >= 5, subs
    assert all(a <= 16 or b <= 16 for a, b in zip(subs, subs[1:])), subs           # every large file has small neighbours


# ---- the figures ----------------------------------------------------------------------------------------------------------------
def report():
    lines = []
    for group in "abc":
        for c in GROUPS[group]():
            f = hf.figures(c.data)
            lines.append(f"{group.upper()}  {c.name:42s}{f['subsequences']:5d}{f['workgroups']:3d}{f['seams']:3d}"
                         f"{100 * f['never']:6.1f} %{f['gap']:3d}{f['segments']:6d}{100 * f['saturated']:6.1f} %")
            seams = hf.sim(c.data).seams()
            if seams:
                lines.append("     seams walk " + ", ".join(f"{x['walked']} ({x['delta']:+d})" for x in seams) +
                             " subsequences (correction of tail); k_jd_sync passes " +
                             ", ".join(str(hf.sim(c.data).sync_group(w)[0]) for w in range(hf.sim(c.data).ngroups)))
    s = hf.sim(hf.noise_twin())
    ups = sorted(s.catch_up(j)[0] for j in range(s.nsub) if s.sub_t[j] > 0)
    lines.append(f"noise twin: {s.nsub} subsequences, catch-up median {ups[len(ups) // 2]}, largest {ups[-1]}")
    return lines


def test_figures_in_the_docstring_are_the_measured_ones():
    for line in report():
        assert line.rstrip() in hf.__doc__, line


if __name__ == "__main__":
    print("\n".join(report()))
