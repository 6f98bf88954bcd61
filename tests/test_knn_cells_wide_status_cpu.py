"""CPU: the wide cell scan's C entry (mgp_knn_cells_scan_wide, 1 <= k <= 1024) -- its declaration, its refusals before
any HIP call in the order the header states, and the build's resource record of its sixteen instantiations."""

import ctypes
import json
import os

import pytest

from muygpys_amd import _abi, _lib


def test_header_declares_both_symbols_with_the_narrow_signature():
    names = _lib.exported_names_from_header()
    assert "mgp_knn_cells_scan_wide" in names and "mgp_knn_cells_wide_max_nn_count" in names
    sig = _abi.signatures()
    assert sig["mgp_knn_cells_scan_wide"] == sig["mgp_knn_cells_scan"]
    assert _lib.load().mgp_knn_cells_wide_max_nn_count() == 1024
    from muygpys_amd import neighbors

    assert neighbors.CELLS_WIDE_MAX_K == 1024 and "wide" in neighbors.CELL_SCANS


BUF = (ctypes.c_char * 4096)()
P = (ctypes.addressof(BUF) + 15) // 16 * 16  # (a host address: no accepted call is made with it)


@pytest.mark.parametrize("change,status", [
    ({"k": 0}, "EINVAL"), ({"nprobe": 11}, "EINVAL"), ({"m": -1}, "EINVAL"),
    ({"k": 1025}, "EUNSUPPORTED"), ({"d": 68}, "EUNSUPPORTED"), ({"d": 6}, "EUNSUPPORTED"),
    ({"n": 2**31}, "EUNSUPPORTED"), ({"table": P + 4}, "EUNSUPPORTED"), ({"queries": P + 4}, "EUNSUPPORTED"),
    ({"table": None, "queries": None, "best_i": None, "m": 0}, "OK"),  # an empty batch reads nothing
    ({"table": None, "k": 1025}, "EINVAL"),  # pointers are looked at before limits
    *[({name: None}, "EINVAL") for name in ("table", "cell_start", "queries", "probes", "best_d", "best_i", "short_flag")],
])
def test_refusals_without_a_gpu(change, status):
    a = dict(table=P, n=1000, d=8, cell_start=P, nlist=10, queries=P, m=5, probes=P, nprobe=3, self_pos=None, k=1024,
             best_d=P, best_i=P, short_flag=P)
    a.update(change)
    assert _lib.load().mgp_knn_cells_scan_wide(*a.values(), None) == getattr(_lib, status)


def test_no_instantiation_uses_scratch():
    with open(os.path.join(os.path.dirname(_lib.LIB_PATH), "kernel_resources.json")) as f:
        mine = {name: r for name, r in json.load(f).items() if "knn_cells_wide_kernel" in name}
    assert len(mine) == 16, sorted(mine)
    for name, r in mine.items():
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0 and r["Dynamic Stack"] == "False", (name, r)
        assert r["Occupancy [waves/SIMD]"] >= 3, (name, r)  # (what 48 KiB of LDS per workgroup allows at k = 1024)
