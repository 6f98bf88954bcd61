"""CPU: the k-NN kernels keep the compiler's records they had before they were moved onto their shared headers
(csrc/mgp_knn_common.h, mgp_knn_tile.h, mgp_knn_cells_scan.h).

tests/golden/parent_bits/knn_kernel_resources.json holds the records of the commit before that change, from its build's
lib/kernel_resources.json, for every kernel of the six k-NN files that report them (mgp_knn_wide, mgp_knn_long,
mgp_knn_cells, mgp_knn_cells_wide, mgp_knn_cells_block, mgp_knn_grid)."""

import json
import os

from muygpys_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = {"knn_scan_wide_kernel": 8, "knn_finish_wide_kernel": 1, "knn_scan_long_kernel": 3, "knn_scan_long_wide_kernel": 3,
            "knn_cells_scan_kernel": 16, "knn_cells_wide_kernel": 16, "knn_cells_block_kernel": 8, "knn_grid_scan_kernel": 1}
EQUAL = ("VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Dynamic Stack", "AGPRs",
         "TotalSGPRs")


def _records():
    with open(os.path.join(ROOT, "tests", "golden", "parent_bits", "knn_kernel_resources.json")) as f:
        then = json.load(f)
    with open(os.path.join(os.path.dirname(_lib.LIB_PATH), "kernel_resources.json")) as f:
        now = json.load(f)
    return then, {n: r for n, r in now.items() if any(f"{fam}I" in n or f"{fam}E" in n for fam in FAMILIES)}


def test_the_recording_holds_every_family():
    then, _ = _records()
    for fam, count in FAMILIES.items():
        assert len([n for n in then if f"{fam}I" in n or f"{fam}E" in n]) == count, fam
    assert len(then) == sum(FAMILIES.values())


def test_the_kernel_names_are_the_same():
    then, now = _records()
    assert sorted(now) == sorted(then)


def test_kernels_keep_their_records():
    """Spills, scratch, LDS, dynamic stack, AGPRs and SGPRs equal; VGPRs no higher and occupancy no lower."""
    then, now = _records()
    for name, r in then.items():
        mine = now.get(name)
        assert mine is not None, name
        for field in EQUAL:
            assert mine[field] == r[field], (name, field, r[field], mine[field])
        assert mine["VGPRs"] <= r["VGPRs"], (name, r["VGPRs"], mine["VGPRs"])
        assert mine["Occupancy [waves/SIMD]"] >= r["Occupancy [waves/SIMD]"], (name, r, mine)
