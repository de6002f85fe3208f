#!/usr/bin/env python3
"""Diff the device code of two trees of this repository, kernel by kernel.

    python tools/diff_device_code.py OLD_TREE NEW_TREE [file.hip ...]

Every named translation unit of vali_amd/csrc (all of them when none is named) is compiled to gfx950 assembly in both
trees, with the flags of that tree's vali_amd/build.py plus --offload-device-only -S.  Per file the set of kernel symbols
must be the same, and per kernel the instruction text and the .amdhsa_ block.  Where both trees hold a built
vali_amd/csrc/_obj, the *.resources.txt reports of the two builds are compared as well.  Exit status 0: no difference.

The compiler's local labels (.LBB<function>_<block>, and BB<function>_<block> in its comments on loops) count the
functions of a file in the order it emits them; that number is dropped from the text that is compared, nothing else is."""
import importlib.util
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path


def hip_flags(tree):
    spec = importlib.util.spec_from_file_location("_build_" + str(abs(hash(str(tree)))), tree / "vali_amd" / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b.HIPCC, [f for f in b.HIP_FLAGS if not f.startswith("-W")]


def assembly(tree, name, out):
    hipcc, flags = hip_flags(tree)
    dst = out / (name + ".s")
    subprocess.run([hipcc, *flags, "--offload-device-only", "-S", str(tree / "vali_amd" / "csrc" / name), "-o", str(dst)],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return dst.read_text()


def kernels(text):
    """{symbol: (instruction lines, .amdhsa_ lines)} of one assembly file"""
    text = re.sub(r"\.L(func_end|func_begin|tmp)\d+", r".L\1", re.sub(r"(BB|JTI)\d+_(\d+)", r"\1_\2", text))
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    out = {}
    for n in names:
        body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end" % re.escape(n), text, re.M | re.S).group(1)
        desc = re.search(r"^\s*\.amdhsa_kernel\s+%s\n(.*?)^\s*\.end_amdhsa_kernel" % re.escape(n), text, re.M | re.S).group(1)
        body = body.split("\t.section\t.rodata", 1)[0]
        out[n] = ([l.rstrip() for l in body.splitlines()], [l.strip() for l in desc.splitlines()])
    return out


def diff_file(old, new, name):
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        ko, kn = kernels(assembly(old, name, Path(a))), kernels(assembly(new, name, Path(b)))
    bad = []
    if set(ko) != set(kn):
        bad.append(f"{name}: kernel symbols differ: only old {sorted(set(ko) - set(kn))}, only new {sorted(set(kn) - set(ko))}")
    for k in sorted(set(ko) & set(kn)):
        if ko[k][0] != kn[k][0]:
            bad.append(f"{name}: {k}: instructions differ ({len(ko[k][0])} and {len(kn[k][0])} lines)")
        if ko[k][1] != kn[k][1]:
            bad.append(f"{name}: {k}: .amdhsa_ block differs")
    return name, len(ko), sum(len(v[0]) for v in ko.values()), bad


def report(path):
    """{kernel: its figures} of one resources report, without the source positions that lead every line"""
    out, name = {}, None
    for line in path.read_text().splitlines():
        line = re.sub(r"^.*?:\d+:\d+: remark: ", "", line).strip()
        if line.startswith("Function Name:"):
            name = line.split()[2]
            out[name] = []
        elif name:
            out[name].append(line)
    return out


def diff_reports(old, new, names):
    bad, seen = [], 0
    for name in names:
        ro, rn = (t / "vali_amd" / "csrc" / "_obj" / (Path(name).stem + ".resources.txt") for t in (old, new))
        if not (ro.exists() and rn.exists()):
            continue
        seen += 1
        if report(ro) != report(rn):
            bad.append(f"{name}: the resource reports differ")
    return seen, bad


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    old, new = Path(argv[1]).resolve(), Path(argv[2]).resolve()
    names = argv[3:] or sorted(p.name for p in (new / "vali_amd" / "csrc").glob("*.hip"))
    with ThreadPoolExecutor(max_workers=8) as pool:
        results = list(pool.map(lambda n: diff_file(old, new, n), names))
    bad = []
    for name, n, lines, b in results:
        print(f"{name}: {n} kernels, {lines} lines of instructions: {'DIFFERENT' if b else 'identical'}")
        bad += b
    seen, b = diff_reports(old, new, names)
    print(f"resource reports compared: {seen} of {len(names)}: {'DIFFERENT' if b else 'identical'}")
    bad += b
    print("\n".join(bad) if bad else "no difference")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
