"""CPU: the build's register report (lib/kernel_resources.json) of the grid walk (csrc/mgp_knn_grid.hip): the kernel is
there, with no stack, no scratch and no spilled vector register.  The figures are also in the header comment of the
kernel file; this test keeps that line honest."""

import json
import os
import re

from muygpys_amd import _lib

HERE = os.path.dirname(os.path.abspath(_lib.__file__))


def report():
    _lib.load()  # (builds nothing: the library and its report come from the build)
    with open(os.path.join(HERE, "lib", "kernel_resources.json")) as f:
        return {name: r for name, r in json.load(f).items() if "knn_grid_scan_kernel" in name}


def test_the_kernel_is_in_the_report_and_does_not_spill():
    kernels = report()
    assert len(kernels) == 1, sorted(kernels)
    for name, r in kernels.items():
        print(f"{name}: {r['VGPRs']} VGPRs, {r['TotalSGPRs']} SGPRs, {r['Occupancy [waves/SIMD]']} waves/SIMD, "
              f"{r['LDS Size [bytes/block]']} bytes of LDS")
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0 and r["Dynamic Stack"] == "False", (name, r)
        assert r["SGPRs Spill"] == 0 and r["AGPRs"] == 0, (name, r)
        assert r["LDS Size [bytes/block]"] == 4 * (64 + 128) * 8  # four waves: 64 list + 128 pending slots of 8 bytes


def test_the_header_comment_of_the_kernel_file_states_the_report():
    with open(os.path.join(HERE, "csrc", "mgp_knn_grid.hip")) as f:
        text = f.read()
    (r,) = report().values()
    row = re.search(r"^//\s+knn_grid_scan_kernel\s+(\d+)\s+(\d+)\s+(\d+)\s+0\s+0\s*$", text, flags=re.M)
    assert row, "the resource line of the header comment"
    assert tuple(map(int, row.groups())) == (r["VGPRs"], r["TotalSGPRs"], r["Occupancy [waves/SIMD]"]), r
