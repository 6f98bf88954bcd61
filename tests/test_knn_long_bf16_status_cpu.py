"""CPU: the status mgp_knn_scan_long_bf16x3 (csrc/mgp_knn_long_bf16.hip) returns BEFORE any HIP call, in the order of
include/muygpys_hip.h -- sizes (MGP_EINVAL), nothing to do (MGP_OK, pointers not looked at), NULL pointers (MGP_EINVAL),
then k > 64, d outside {68, 72, .. 256}, alignment, n >= 2^31 (MGP_EUNSUPPORTED) -- one rule violated per row, host buffers
standing in for device pointers; the derived margin; and the build's register report of its instantiations."""

import ctypes as C
import json
import os
import re

import pytest

from muygpys_amd import _lib

OK, EINVAL, EUNSUPPORTED = _lib.OK, _lib.EINVAL, _lib.EUNSUPPORTED
PARAMS = "train ptrain sqn n d q pq qsqn self m k start best_d best_i overflow st".split()
NUMBERS = dict(n=5000, d=100, m=5, k=30, start=128)
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
         ("no queries, k = 65, d = 64", dict(m=0, k=65, d=64, **NOTHING), OK)]
ROWS += [(f"{p} NULL", {p: None}, EINVAL) for p in REQUIRED]
ROWS += [("k = 65", dict(k=65), EUNSUPPORTED), ("k = 65 with a NULL pointer", dict(k=65, best_d=None), EINVAL)]
ROWS += [(f"d = {d}", dict(d=d), EUNSUPPORTED) for d in (4, 40, 64, 66, 70, 260)]
ROWS += [(f"{p} 4 bytes off alignment", {p: PTR + 4}, EUNSUPPORTED) for p in ("train", "ptrain", "q", "pq")]
ROWS += [("n = 2^31", dict(n=2**31), EUNSUPPORTED)]


@pytest.mark.parametrize("name, changes, want", ROWS, ids=[r[0] for r in ROWS])
def test_status_of_refused_and_empty_calls(name, changes, want):
    args = {n: NUMBERS.get(n, None if n in OPTIONAL else PTR) for n in PARAMS}
    args.update(changes)
    assert _lib.load().mgp_knn_scan_long_bf16x3(*[args[n] for n in PARAMS]) == want


def test_the_declaration_the_packed_width_and_the_margin():
    """At KP = 272 the derived error bound exceeds the short rows' 2^-14 even at a unit roundoff of 2^-24 per addition:
    3.1 x 2^-16 + 816 x 2^-24 = 6.3 x 2^-16 > 4 x 2^-16."""
    pytest.importorskip("torch")
    from muygpys_amd import neighbors as nb

    assert "mgp_knn_scan_long_bf16x3" in _lib.exported_names_from_header()
    assert list(_lib.load().mgp_knn_scan_long_bf16x3.argtypes) == list(_lib.load().mgp_knn_scan_bf16x3.argtypes)
    assert [nb.packed_width(d) for d in (68, 78, 80, 100, 128, 256)] == [80, 80, 96, 112, 144, 272]
    assert 3.1 * 2.0**-16 + 3 * 272 * 2.0**-24 > 2.0**-14
    for kp in range(80, 273, 16):
        assert nb.prefilter_margin(kp) >= 3.1 * 2.0**-16 + 3 * kp * 2.0**-23 > 2.0**-14
        assert nb.prefilter_raise(kp) >= 2.0**-18 + 2.0**-24 + 3 * kp * 2.0**-23
    assert nb.prefilter_margin(272) < 2.5 * 2.0**-14  # (what the no-overflow rule of the GPU tests allows for)


def test_every_instantiation_is_in_the_report_and_the_header_comment_states_it():
    here = os.path.dirname(os.path.abspath(_lib.__file__))
    _lib.load()
    with open(os.path.join(here, "lib", "kernel_resources.json")) as f:
        kernels = {n: r for n, r in json.load(f).items() if "knn_prefilter_long_kernel" in n}
    with open(os.path.join(here, "csrc", "mgp_knn_long_bf16.hip")) as f:
        text = f.read()
    shapes = sorted(tuple(map(int, re.search(r"ILi(\d+)ELi(\d)EEE", n).groups())) for n in kernels)
    assert shapes == [(nq, 2 if nq <= 6 else 1) for nq in range(5, 18)], shapes
    for name, r in kernels.items():
        nq, rbn = map(int, re.search(r"ILi(\d+)ELi(\d)EEE", name).groups())
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0 and r["Dynamic Stack"] == "False", (name, r)
        assert r["Occupancy [waves/SIMD]"] >= (2 if nq <= 9 else 1), (name, r)  # (NQ = 9: d = 128)
        row = re.search(rf"^//\s+knn_prefilter_long_kernel\s+{nq}\s+{rbn}\s+(\d+)\s+(\d+)\s+(\d+)\s+0\s+0\s*$", text, flags=re.M)
        assert row, (nq, rbn)
        assert tuple(map(int, row.groups())) == (r["VGPRs"], r["AGPRs"], r["Occupancy [waves/SIMD]"]), (name, r)
