"""CPU: the build's register report (lib/kernel_resources.json) of the long-row k-NN scans (csrc/mgp_knn_long.hip): both
kernels in each of their three chunk counts, none with a stack, none spilling a vector register.  The figures are also
in the header comment of the kernel file; this test keeps that table honest."""

import json
import os
import re

from muygpys_amd import _lib

HERE = os.path.dirname(os.path.abspath(_lib.__file__))


def report():
    _lib.load()  # (builds the library where it is missing)
    with open(os.path.join(HERE, "lib", "kernel_resources.json")) as f:
        return {name: r for name, r in json.load(f).items() if "knn_scan_long" in name}


def chunk_count(name):
    return int(re.search(r"ILi(\d)EEE", name).group(1))


def test_every_instantiation_is_in_the_report_and_none_spills():
    kernels = report()
    narrow = sorted(chunk_count(n) for n in kernels if "knn_scan_long_kernel" in n)
    wide = sorted(chunk_count(n) for n in kernels if "knn_scan_long_wide_kernel" in n)
    assert narrow == [2, 3, 4] and wide == [2, 3, 4] and len(kernels) == 6, sorted(kernels)
    for name, r in kernels.items():
        print(f"{name}: {r['VGPRs']} VGPRs, {r['AGPRs']} AGPRs, {r['Occupancy [waves/SIMD]']} waves/SIMD")
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0 and r["Dynamic Stack"] == "False", (name, r)
        assert r["VGPRs"] + r["AGPRs"] <= 512 and r["Occupancy [waves/SIMD]"] >= 1, (name, r)


def test_the_header_comment_of_the_kernel_file_states_the_report():
    with open(os.path.join(HERE, "csrc", "mgp_knn_long.hip")) as f:
        text = f.read()
    for name, r in report().items():
        kernel = "knn_scan_long_wide_kernel" if "long_wide" in name else "knn_scan_long_kernel"
        row = re.search(rf"^//\s+{kernel}\s+{chunk_count(name)}\s+(\d+)\s+(\d+)\s+(\d+)\s+0\s+0\s*$", text, flags=re.M)
        assert row, (kernel, chunk_count(name))
        assert tuple(map(int, row.groups())) == (r["VGPRs"], r["AGPRs"], r["Occupancy [waves/SIMD]"]), (name, r)
