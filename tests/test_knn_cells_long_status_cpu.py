"""CPU: the long-row cell scan's C entry (mgp_knn_cells_scan_long, 68 <= d <= 256, 1 <= k <= 1024) -- its declaration,
its refusals before any HIP call in the order the header states, and the build's resource record of its two kernels."""

import ctypes
import json
import os

import pytest

from muygpys_amd import _abi, _lib


def test_header_declares_the_entry_with_the_narrow_signature():
    assert "mgp_knn_cells_scan_long" in _lib.exported_names_from_header()
    sig = _abi.signatures()
    assert sig["mgp_knn_cells_scan_long"] == sig["mgp_knn_cells_scan"]
    from muygpys_amd import neighbors

    assert "long" in neighbors.CELL_SCANS and _lib.load().mgp_knn_long_max_features() == neighbors.LONG_MAX_D == 256


BUF = (ctypes.c_char * 4096)()
P = (ctypes.addressof(BUF) + 15) // 16 * 16  # (a host address: no accepted call is made with it)


@pytest.mark.parametrize("change,status", [
    ({"k": 0}, "EINVAL"), ({"nprobe": 11}, "EINVAL"), ({"m": -1}, "EINVAL"),
    ({"d": 64}, "EUNSUPPORTED"), ({"d": 8}, "EUNSUPPORTED"), ({"d": 70}, "EUNSUPPORTED"), ({"d": 260}, "EUNSUPPORTED"),
    ({"k": 1025}, "EUNSUPPORTED"), ({"n": 2**31}, "EUNSUPPORTED"),
    ({"table": P + 4}, "EUNSUPPORTED"), ({"queries": P + 4}, "EUNSUPPORTED"),
    ({"table": None, "queries": None, "best_i": None, "m": 0}, "OK"),  # an empty batch reads nothing
    ({"table": None, "k": 1025}, "EINVAL"), ({"probes": None, "d": 64}, "EINVAL"),  # pointers are looked at before limits
    *[({name: None}, "EINVAL") for name in ("table", "cell_start", "queries", "probes", "best_d", "best_i", "short_flag")],
])
def test_refusals_without_a_gpu(change, status):
    a = dict(table=P, n=1000, d=100, cell_start=P, nlist=10, queries=P, m=5, probes=P, nprobe=3, self_pos=None, k=1024,
             best_d=P, best_i=P, short_flag=P)
    a.update(change)
    assert _lib.load().mgp_knn_cells_scan_long(*a.values(), None) == getattr(_lib, status)


def test_no_kernel_spills_or_uses_scratch():
    with open(os.path.join(os.path.dirname(_lib.LIB_PATH), "kernel_resources.json")) as f:
        mine = {name: r for name, r in json.load(f).items() if "cells_longrow" in name}
    assert len(mine) == 2, sorted(mine)  # the WaveList and the WideWaveList form
    for name, r in mine.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (name, r)
        assert r["Dynamic Stack"] == "False", (name, r)
