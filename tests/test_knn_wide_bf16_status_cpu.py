"""CPU: the status mgp_knn_scan_wide_bf16x3 (csrc/mgp_knn_wide_bf16.hip) returns BEFORE any HIP call, in the order of
include/muygpys_hip.h -- sizes (MGP_EINVAL), nothing to do (MGP_OK, pointers not looked at), NULL pointers (MGP_EINVAL),
then k > 1024, d outside {4, 8, .. 64}, alignment, n >= 2^31, k (+ 1 with self_idx) > start (MGP_EUNSUPPORTED) -- one rule
violated per row, host buffers standing in for device pointers; its declaration; and the build's register report."""

import ctypes as C
import json
import os
import re

import pytest

from muygpys_amd import _lib

OK, EINVAL, EUNSUPPORTED = _lib.OK, _lib.EINVAL, _lib.EUNSUPPORTED
PARAMS = "train ptrain sqn n d q pq qsqn self m k start best_d best_i overflow st".split()
NUMBERS = dict(n=5000, d=40, m=5, k=100, start=130)  # (any start: 130 is no multiple of 64)
OPTIONAL = ("self", "st")
_BUF = (C.c_char * 4096)()
PTR = (C.addressof(_BUF) + 15) // 16 * 16
REQUIRED = [n for n in PARAMS if n not in NUMBERS and n not in OPTIONAL]
NOTHING = {n: None for n in PARAMS if n not in NUMBERS}

ROWS = [(f"{s} < 0", {s: -1}, EINVAL) for s in ("n", "m", "start")]
ROWS += [("d < 1", dict(d=0), EINVAL), ("k < 1", dict(k=0), EINVAL)]
ROWS += [("no queries, all pointers NULL", dict(m=0, **NOTHING), OK),
         ("start = n, all pointers NULL", dict(start=5000, **NOTHING), OK),
         ("start > n, all pointers NULL", dict(start=5056, **NOTHING), OK),
         ("no queries, k < 1", dict(m=0, k=0), EINVAL),
         ("no queries, k = 1025, d = 68", dict(m=0, k=1025, d=68, **NOTHING), OK)]
ROWS += [(f"{p} NULL", {p: None}, EINVAL) for p in REQUIRED]
ROWS += [("k = 1025", dict(k=1025, start=2048), EUNSUPPORTED),
         ("k = 1025 with a NULL pointer", dict(k=1025, start=2048, best_d=None), EINVAL)]
ROWS += [(f"d = {d}", dict(d=d), EUNSUPPORTED) for d in (2, 6, 66, 68, 100)]
ROWS += [(f"{p} 4 bytes off alignment", {p: PTR + 4}, EUNSUPPORTED) for p in ("train", "ptrain", "q", "pq")]
ROWS += [("n = 2^31", dict(n=2**31), EUNSUPPORTED)]
ROWS += [("k = start + 1", dict(k=131), EUNSUPPORTED), ("k = start with self_idx", dict(k=130, self=PTR), EUNSUPPORTED),
         ("k = 1024 at start = 1024 with self_idx", dict(k=1024, start=1024, self=PTR), EUNSUPPORTED)]


@pytest.mark.parametrize("name, changes, want", ROWS, ids=[r[0] for r in ROWS])
def test_status_of_refused_and_empty_calls(name, changes, want):
    args = {n: NUMBERS.get(n, None if n in OPTIONAL else PTR) for n in PARAMS}
    args.update(changes)
    assert _lib.load().mgp_knn_scan_wide_bf16x3(*[args[n] for n in PARAMS]) == want


def test_the_declaration_and_the_window():
    lib = _lib.load()
    assert "mgp_knn_scan_wide_bf16x3" in _lib.exported_names_from_header()
    assert list(lib.mgp_knn_scan_wide_bf16x3.argtypes) == list(lib.mgp_knn_scan_bf16x3.argtypes)
    assert lib.mgp_knn_scan_wide_bf16x3.restype == lib.mgp_knn_scan_bf16x3.restype
    assert lib.mgp_knn_wide_bf16_window() in (8, 16)


def test_every_instantiation_is_in_the_report_and_the_header_comment_states_it():
    here = os.path.dirname(os.path.abspath(_lib.__file__))
    _lib.load()
    with open(os.path.join(here, "lib", "kernel_resources.json")) as f:
        kernels = {n: r for n, r in json.load(f).items() if "knn_prefilter_wide_kernel" in n}
    with open(os.path.join(here, "csrc", "mgp_knn_wide_bf16.hip")) as f:
        text = f.read()
    assert sorted(int(re.search(r"ILi(\d+)EEE", n).group(1)) for n in kernels) == [16, 32, 48, 64, 80], sorted(kernels)
    for name, r in kernels.items():
        kp = int(re.search(r"ILi(\d+)EEE", name).group(1))
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0 and r["Dynamic Stack"] == "False", (name, r)
        assert r["Occupancy [waves/SIMD]"] >= 2, (name, r)
        row = re.search(rf"^//\s+knn_prefilter_wide_kernel\s+{kp}\s+(\d+)\s+(\d+)\s+(\d+)\s+0\s+0\s+(\d+)\s*$", text, flags=re.M)
        assert row, kp
        assert tuple(map(int, row.groups()[:3])) == (r["VGPRs"], r["AGPRs"], r["Occupancy [waves/SIMD]"]), (name, r)
        # dynamic LDS (the launcher's formula: two tiles, the mask ring, slot words and tau): two workgroups per CU
        lds = int(row.group(4))
        assert lds == 2 * 64 * (4 * kp + 16) + 256 * (2 * lib_window() + 2) * 4 and 2 * lds <= 160 * 1024


def lib_window():
    return _lib.load().mgp_knn_wide_bf16_window()
