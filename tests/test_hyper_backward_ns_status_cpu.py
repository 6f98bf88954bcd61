"""CPU: the hyper-parameter backward entries with a length scale per neighbourhood (mgp_hyper_backward_ns_*,
mgp_hyper_backward_ns_large_*; include/muygpys_hip.h) -- the status of every refused or empty call, decided BEFORE any
HIP call, in the style of tests/test_posterior_ns_status_cpu.py -- and the compiler's record of the new kernels.

One rule is violated per row, starting from arguments that would launch.  Host buffers stand in for device pointers:
nothing dereferences them before the status is decided.  No row here reaches a launch."""

import ctypes as C
import json
import os

import pytest

from muygpys_amd import _lib

OK, EINVAL, EUNSUPPORTED = 0, -1, -2
ES = {"f32": 4, "f64": 8}
INT_MAX, INT64_MAX = 2**31 - 1, 2**63 - 1

ENTRIES = {
    "hyper_backward_ns": "feat d bi ni b k tg R nm eps nd kid mid lsb lsc gm gv gyk gls gnz info st",
    "hyper_backward_ns_large": "feat d bi ni b k tg R nm eps nd kid mid lsb lsc gm gv gyk gls gnz info ws wsb st",
}
NUMBERS = dict(d=4, b=3, k=5, R=1, nm=0, eps=1e-3, kid=2, mid=0, lsc=1, wsb=1 << 40)
OPTIONAL = ("nd", "st", "bi", "info")
BUF = (C.c_double * 64)()
PTR = C.addressof(BUF)
assert PTR % 16 == 0


def status(entry, suf, **changes):
    names = ENTRIES[entry].split()
    args = {n: NUMBERS[n] if n in NUMBERS else (None if n in OPTIONAL else PTR) for n in names}
    assert not set(changes) - set(names), (entry, changes)
    args.update(changes)
    return getattr(_lib.load(), f"mgp_{entry}_{suf}")(*[args[n] for n in names])


def rows_of(entry):
    names = ENTRIES[entry].split()
    large = entry.endswith("large")
    rows = [("b < 0", dict(b=-1), EINVAL), ("k < 1", dict(k=0), EINVAL), ("d < 1", dict(d=0), EINVAL), ("R < 1", dict(R=0), EINVAL)]
    rows += [(f"{p} NULL", {p: None}, EINVAL) for p in "feat tg ni lsb".split()]
    rows += [(f"kernel id {i}", dict(kid=i), EINVAL) for i in (-1, 6, 99)]
    rows += [(f"metric id {i}", dict(mid=i), EINVAL) for i in (-1, 2)]
    rows += [(f"noise mode {i}", dict(nm=i), EINVAL) for i in (-1, 3)]
    rows += [(f"noise mode {i} without noise_dev", dict(nm=i, nd=None), EINVAL) for i in (1, 2)]
    rows += [(f"ls_count {i} at d = 4", dict(lsc=i), EINVAL) for i in (0, 2, 5)]
    rows.append(("no cotangent", dict(gm=None, gv=None, gyk=None), EINVAL))
    rows.append(("no output", dict(gls=None, gnz=None), EINVAL))
    rows.append(("grad_ykinvy with R = 3", dict(R=3), EINVAL))
    rows.append(("the general-nu id", dict(kid=5), EUNSUPPORTED))
    rows.append(("the general-nu id, length_scale_batch NULL", dict(kid=5, lsb=None), EINVAL))
    rows.append(("the general-nu id, no output", dict(kid=5, gls=None, gnz=None), EINVAL))
    if large:
        rows.append(("the general-nu id, workspace NULL", dict(kid=5, ws=None), EINVAL))
        rows.append(("k + 2 = 1025", dict(k=1023), EUNSUPPORTED))
        rows.append(("k = INT_MAX", dict(k=INT_MAX, wsb=INT64_MAX), EUNSUPPORTED))
        rows.append(("workspace NULL", dict(ws=None), EINVAL))
        rows.append(("workspace misaligned", dict(ws=PTR + 8), EINVAL))
    else:
        rows.append(("a system beyond LDS", dict(k=1000), EUNSUPPORTED))
        rows.append(("a system beyond LDS, length_scale_batch NULL", dict(k=1000, lsb=None), EINVAL))
        rows.append(("k = INT_MAX", dict(k=INT_MAX), EUNSUPPORTED))
    nothing = {n: None for n in names if n not in NUMBERS}
    rows.append(("empty batch, all pointers NULL", dict(b=0, **nothing, **({"wsb": 0} if large else {})), OK))
    rows.append(("empty batch, ids not looked at", dict(b=0, **nothing, kid=99, mid=7, nm=8, lsc=9), OK))
    rows.append(("empty batch, k < 1", dict(b=0, k=0), EINVAL))
    return rows


GRID = [(e, n, ch, want) for e in ENTRIES for n, ch, want in rows_of(e)]


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("entry, name, changes, want", GRID, ids=[f"{e}: {n}" for e, n, _, _ in GRID])
def test_status_of_refused_and_empty_calls(entry, name, changes, want, suf):
    assert status(entry, suf, **changes) == want


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_limits_are_the_scalar_entries(suf):
    es = ES[suf]
    limit = _lib.load().mgp_max_nn_count_backward(es)
    assert status("hyper_backward_ns", suf, k=limit + 1) == EUNSUPPORTED
    for k in (5, 200, 1022):
        slab = _lib.load().mgp_backward_large_workspace_bytes(es, k, 1)
        assert status("hyper_backward_ns_large", suf, k=k, wsb=slab - 1) == EINVAL, k


def test_resource_records_of_the_new_kernels():
    """Two LDS and two slab kernels without spills or scratch; thirteen wave-sized kernels (fp32: two slot counts, five
    row widths; fp64: three) whose scratch stays within that of backward_wave_kernel's hyper-parameter instantiation of
    the same shape (the fp32 64-slot ones spill a handful of registers, as those do)."""
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), "kernel_resources.json")
    with open(path) as f:
        res = json.load(f)
    mine = {n: r for n, r in res.items() if "ns_lds_backward_kernel" in n or "ns_slab_backward_kernel" in n}
    assert len(mine) == 4, sorted(mine)
    for name, r in mine.items():
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (name, r)
    wave = {n: r for n, r in res.items() if "ns_wave_backward_kernel" in n}
    assert len(wave) == 13, sorted(wave)
    for name, r in wave.items():  # ...ns_kernelI<T>Li<NP>ELi<DG>EEEv... against ...kernelI<T>Li<NP>ELi<DG>ELi0ELb1EEEv...
        shape = name.split("ns_wave_backward_kernelI")[1].split("EEEv")[0]
        scalar = res[f"_ZN3mgp20backward_wave_kernelI{shape}ELi0ELb1EEEvNS_12BackwardArgsEi"]
        assert r["ScratchSize [bytes/lane]"] <= scalar["ScratchSize [bytes/lane]"], (name, r, scalar)
