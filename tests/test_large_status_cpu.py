"""CPU: the entries for systems beyond LDS (mgp_posterior_large_*, mgp_solve_large_*, mgp_large_max_nn_count,
mgp_large_workspace_bytes; include/muygpys_hip.h) -- the status of every refused or empty call, decided BEFORE any HIP
call, the limits and workspace sizes, the unchanged mgp_max_nn_count, and the compiler's register record of the kernels.

One rule is violated per row, starting from arguments that would launch.  Host buffers stand in for device pointers:
nothing dereferences them before the status is decided.  No row here reaches a launch."""

import ctypes as C
import json
import os

import pytest

from muygpys_amd import _lib

OK, EINVAL, EUNSUPPORTED = 0, -1, -2
ES = {"f32": 4, "f64": 8}
MIB = 1 << 20
INT_MAX, INT64_MAX = 2**31 - 1, 2**63 - 1

ENTRIES = {
    "posterior_large": "fq fn d bi ni b k tg R tb nm eps nd kid mid ls lsc mean var yk info ws wsb st",
    "solve_large": "Kin Kc Y b k R kout mean var yk coeffs info ws wsb st",
}
NUMBERS = dict(d=4, b=3, k=5, R=1, tb=0, nm=0, eps=1e-3, kid=2, mid=0, lsc=1, kout=1.0, wsb=1 << 40)
OPTIONAL = ("nd", "st")
REQUIRED = {"posterior_large": "fq fn tg ni ls mean var", "solve_large": "Kin Y Kc"}
BUF = (C.c_double * 64)()
PTR = C.addressof(BUF)  # (16-byte aligned: ctypes arrays of doubles come from malloc)
assert PTR % 16 == 0


def status(entry, suf, **changes):
    names = ENTRIES[entry].split()
    args = {n: NUMBERS[n] if n in NUMBERS else (None if n in OPTIONAL else PTR) for n in names}
    unknown = set(changes) - set(names)
    assert not unknown, (entry, unknown)
    args.update(changes)
    return getattr(_lib.load(), f"mgp_{entry}_{suf}")(*[args[n] for n in names])


def slab(es, k, R):
    """What one system occupies: the recommended workspace of a batch of one."""
    return _lib.load().mgp_large_workspace_bytes(es, k, R, 1)


def rows_of(entry):
    names = ENTRIES[entry].split()
    fused = entry == "posterior_large"
    rows = [("b < 0", dict(b=-1), EINVAL), ("k < 1", dict(k=0), EINVAL)]
    rows += [("d < 1", dict(d=0), EINVAL), ("R < 1", dict(R=0), EINVAL)] if fused else [("R < 0", dict(R=-1), EINVAL)]
    rows += [(f"{p} NULL", {p: None}, EINVAL) for p in REQUIRED[entry].split()]
    if fused:
        rows += [(f"kernel id {i}", dict(kid=i), EINVAL) for i in (-1, 6, 99)]
        rows += [(f"metric id {i}", dict(mid=i), EINVAL) for i in (-1, 2)]
        rows += [(f"noise mode {i}", dict(nm=i), EINVAL) for i in (-1, 3)]
        rows += [(f"noise mode {i} without noise_dev", dict(nm=i, nd=None), EINVAL) for i in (1, 2)]
        rows += [(f"ls_count {i} at d = 4", dict(lsc=i), EINVAL) for i in (0, 2, 5)]
        rows.append(("the general-nu id", dict(kid=5), EUNSUPPORTED))
        rows.append(("the general-nu id, workspace NULL", dict(kid=5, ws=None), EINVAL))
        rows.append(("k + 1 + R = 1025", dict(k=1023), EUNSUPPORTED))
        rows.append(("k + 1 + R = 1025 by responses", dict(k=1008, R=16), EUNSUPPORTED))
        rows.append(("k + 1 + R = 1025, outputs NULL", dict(k=1023, mean=None), EINVAL))
    else:
        rows.append(("mean without responses", dict(R=0, Y=None), EINVAL))
        rows.append(("k + 1 + R = 1025", dict(k=1023), EUNSUPPORTED))
        rows.append(("k + 1 + R = 1025, Kin NULL", dict(k=1023, Kin=None), EINVAL))
    # sizes near INT_MAX: the row count is taken in 64 bits (in 32 it wraps below the limit and the call would launch),
    # and a slab whose byte count passes int64 is larger than any workspace
    rows.append(("k = INT_MAX", dict(k=INT_MAX, wsb=INT64_MAX), EUNSUPPORTED))
    rows.append(("k = R = INT_MAX", dict(k=INT_MAX, R=INT_MAX, wsb=INT64_MAX), EUNSUPPORTED))
    rows.append(("k = INT_MAX, a workspace of 1 TiB", dict(k=INT_MAX), EINVAL))
    rows.append(("workspace NULL", dict(ws=None), EINVAL))
    rows.append(("workspace misaligned", dict(ws=PTR + 8), EINVAL))
    rows.append(("k + 1 + R = 1025, workspace misaligned", dict(k=1023, ws=PTR + 4), EINVAL))
    nothing = {n: None for n in names if n not in NUMBERS}
    rows.append(("empty batch, all pointers NULL", dict(b=0, wsb=0, **nothing), OK))
    if fused:
        rows.append(("empty batch, ids not looked at", dict(b=0, wsb=0, **nothing, kid=99, mid=7, nm=8, lsc=9), OK))
    rows.append(("empty batch, k < 1", dict(b=0, k=0), EINVAL))
    return rows


GRID = [(e, n, ch, want) for e in ENTRIES for n, ch, want in rows_of(e)]


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("entry, name, changes, want", GRID, ids=[f"{e}: {n}" for e, n, _, _ in GRID])
def test_status_of_refused_and_empty_calls(entry, name, changes, want, suf):
    assert status(entry, suf, **changes) == want


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_workspace_one_byte_short_of_a_slab(entry, suf):
    es = ES[suf]
    for k, R in ((5, 1), (200, 1), (1022, 1), (1007, 16)):
        assert status(entry, suf, k=k, R=R, wsb=slab(es, k, R) - 1) == EINVAL, (k, R)
    # ... and in front of the refusal of a system beyond the kernel: any finite workspace is short of 0 slabs' worth
    assert status(entry, suf, k=1023, wsb=15) == EINVAL


def test_limits():
    lib = _lib.load()
    assert lib.mgp_large_max_nn_count(4, 1) == lib.mgp_large_max_nn_count(8, 1) == 1022
    assert lib.mgp_large_max_nn_count(4, 16) == lib.mgp_large_max_nn_count(8, 16) == 1007
    assert lib.mgp_large_max_nn_count(2, 1) == -1


def test_existing_limits_unchanged():
    """mgp_max_nn_count as the parent commit returns it (read there once)."""
    lib = _lib.load()
    assert lib.mgp_max_nn_count(4, 1) == PARENT_MAX_NN_F32
    assert lib.mgp_max_nn_count(8, 1) == PARENT_MAX_NN_F64


PARENT_MAX_NN_F32, PARENT_MAX_NN_F64 = 192, 134


@pytest.mark.parametrize("es", [4, 8])
def test_workspace_sizes(es):
    wb = _lib.load().mgp_large_workspace_bytes
    ks = list(range(1, 70)) + [127, 128, 129, 200, 300, 511, 512, 513, 1000, 1007, 1021, 1022]
    bs = [0, 1, 2, 37, 255, 256, 257, 5000, 10**6]
    for R in (0, 1, 16):
        for b in bs:
            sizes = [wb(es, k, R, b) for k in ks if k + 1 + R <= 1024]
            assert all(s > 0 and s % 16 == 0 and s <= 512 * MIB for s in sizes), (R, b)
            assert sizes == sorted(sizes), ("non-decreasing in k", R, b)
        for k in (1, 33, 200, 1000):
            sizes = [wb(es, k, R, b) for b in bs]
            assert sizes == sorted(sizes), ("non-decreasing in b", R, k)
            assert sizes[0] == sizes[1] == slab(es, k, R)  # (at least one slab)
    # beyond the limit, and for arguments nothing serves
    assert wb(es, 1023, 1, 8) == 0 and wb(es, 1008, 16, 8) == 0 and wb(es, 5000, 1, 8) == 0
    assert wb(es, 0, 1, 8) == 0 and wb(es, 5, -1, 8) == 0 and wb(es, 5, 1, -1) == 0
    assert wb(2, 5, 1, 8) == 0
    # the cap binds for the largest systems
    assert wb(es, 1022, 1, 10**6) == 512 * MIB


def test_no_spills_no_scratch():
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), "kernel_resources.json")
    with open(path) as f:
        res = json.load(f)
    mine = {n: r for n, r in res.items() if "fused_large_kernel" in n or "solve_large_kernel" in n}
    assert len(mine) == 4, sorted(mine)  # two front ends, two float widths
    for name, r in mine.items():
        assert r["VGPRs Spill"] == 0, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
