"""No kernel may use scratch (private) memory or spill registers.

Scratch is silent: results stay bit-exact and only the speed goes.  A `for (r = 0; r < (has_row1 ? 2 : 1); ++r)` over a
register array stayed rolled after an unrelated change, the array moved to scratch, and every converter with a packed
RGB / BGR destination ran at 2.5-4.3 TB/s instead of 5.9-6.2 for most of round 2 (tools/cliffs.py found it).  The build
keeps the compiler's per-kernel resource remarks next to the objects (vali_amd/build.py); this test reads them.
"""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
OBJ = ROOT / "vali_amd" / "csrc" / "_obj"

ALLOWED = set()   # (round 2 had one A/B instantiation that spilled; it also turned out to mis-render and was removed)

# SGPR spills (scalars parked in VGPR lanes: v_writelane / v_readlane on the critical path): none, anywhere.  Rounds 1-3
# allowed six instantiations of k_ud_down2 (13-75 spilled SGPRs: the any-height / ragged-width / half-turn forms of the
# exact-ratio UD kernel); round 4 replaced that kernel with k_ud_lean, which serves the aligned geometries without a spill,
# and sent the ragged and half-turned ones to the general kernel.
SGPR_SPILLS_ALLOWED = {}


def kernels():
    out = {}
    for f in sorted(OBJ.glob("*.resources.txt")):
        name = None
        for line in f.read_text().splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                out[name] = {"file": f.name}
                continue
            m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (-?\d+)", line)
            if m and name:
                out[name][m.group(1).strip()] = int(m.group(2))
    return out


def test_resource_reports_exist_for_every_translation_unit():
    srcs = sorted((ROOT / "vali_amd" / "csrc").glob("*.hip"))
    assert srcs
    for s in srcs:
        assert (OBJ / (s.stem + ".resources.txt")).exists(), f"build did not leave a resource report for {s.name}"
    assert len(kernels()) > 100


def test_no_kernel_uses_scratch_or_spills():
    bad = []
    for name, r in kernels().items():
        if name in ALLOWED:
            continue
        if r.get("ScratchSize", 0) or r.get("VGPRs Spill", 0) or r.get("SGPRs Spill", 0) > SGPR_SPILLS_ALLOWED.get(name, 0):
            bad.append((name, r))
    assert not bad, "kernels with scratch / spills:\n" + "\n".join(f"{n}: {r}" for n, r in bad)


def test_the_hot_kernels_spill_nothing_and_keep_their_occupancy():
    """the kernels the bench lines are quoted on: no spilled SGPR, and the waves per SIMD their design counts on"""
    k = kernels()
    want = {"k_nv12_rgb8": 8, "k_ud_half": 8, "k_ud_half_t": 4, "k_resize_cols_x2IhLi12ELi6ELi3E": 5,
            # the general columns-first form on specialised waves (3 slots at 1.98:1, 4 at 4:3 / 5:4; the last figure is the
            # consumer's sets): six waves per SIMD at 3 slots, five with wide tiles or 4 slots
            "k_resize_cols_wsIhLi12ELi6ELi3ELi4E": 6, "k_resize_cols_wsIhLi12ELi6ELi3ELi5E": 5, "k_resize_cols_wsIhLi12ELi6ELi4ELi5E": 5,
            "k_resize_cols_wsIhLi3ELi6ELi4ELi5E": 5, "k_resize_cols_wsIhLi3ELi6ELi3ELi4E": 6,
            "k_resize_up2IhLi6ELb0E": 6, "k_resize_up2IhLi6ELb1E": 6, "k_resize_up2ItLi6ELb0E": 6,   # (the workgroups-per-CU figures of launch_resize_up2)
            # planes that grow: the 3:2 form the upscale bench line is quoted on, and the general rows-first kernel
            "k_resize_rows_x23IhLi12ELi6ELi48E": 4, "k_resize_rowsIhLi12ELi6ELi32E": 4,
            # ... its packed-RGB variant: 54 registers of filtered rows and still the fourth wave (3 waves: 3.5 us instead of 2.9)
            "k_resize_rows_x23_rgbILi6ELi48E": 4, "k_resize_rows_rgbILi64E": 4}
    seen = set()
    for name, r in k.items():
        for needle, occ in want.items():
            if needle in name and ("_x2I" in name) == ("_x2I" in needle) and ("half_t" in name) == ("half_t" in needle) and ("_wsI" in name) == ("_wsI" in needle):
                seen.add(needle)
                assert r.get("SGPRs Spill", 0) == 0 and r.get("ScratchSize", 0) == 0, (name, r)
                if "Occupancy" in r:
                    assert r["Occupancy"] >= occ, (name, r["Occupancy"], occ)
    assert seen == set(want), seen


def test_no_timing_only_branches_in_the_product_kernels():
    """Ablation switches (`VALI_COLS_ABLATE`, `VALI_WS_ABL`: parts of a kernel compiled out for timing, results invalid) live
    in tools/exp/resize_cols_ablations.patch, not in the sources the library is built from."""
    for f in sorted((ROOT / "vali_amd" / "csrc").glob("*.h*")):
        text = f.read_text()
        assert not re.search(r"ABLATE|_ABL\b", text), f.name
    assert (ROOT / "tools" / "exp" / "resize_cols_ablations.patch").exists()
