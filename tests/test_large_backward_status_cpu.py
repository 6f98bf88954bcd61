"""CPU: the hyper-parameter backward beyond LDS (mgp_hyper_backward_large_*, mgp_backward_large_workspace_bytes;
include/muygpys_hip.h) -- the status of every refused or empty call, decided BEFORE any HIP call and in the order the
header states, the workspace sizes, the unchanged mgp_max_nn_count_backward, and the compiler's register record.

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

NAMES = "feat d bi ni b k tg R nm eps nd kid mid ls lsc gm gv gyk gls gnz info ws wsb st".split()
NUMBERS = dict(d=4, b=3, k=5, R=1, nm=0, eps=1e-3, kid=2, mid=0, lsc=1, wsb=1 << 40)
OPTIONAL = ("nd", "st")
BUF = (C.c_double * 64)()
PTR = C.addressof(BUF)  # (16-byte aligned: ctypes arrays of doubles come from malloc)
assert PTR % 16 == 0


def status(suf, **changes):
    args = {n: NUMBERS[n] if n in NUMBERS else (None if n in OPTIONAL else PTR) for n in NAMES}
    unknown = set(changes) - set(NAMES)
    assert not unknown, unknown
    args.update(changes)
    return getattr(_lib.load(), f"mgp_hyper_backward_large_{suf}")(*[args[n] for n in NAMES])


def slab(es, k):
    """What one system occupies: the recommended workspace of a batch of one."""
    return _lib.load().mgp_backward_large_workspace_bytes(es, k, 1)


def _rows():
    # 1. sizes
    rows = [("b < 0", dict(b=-1), EINVAL), ("k < 1", dict(k=0), EINVAL), ("d < 1", dict(d=0), EINVAL),
            ("R < 1", dict(R=0), EINVAL)]
    # 2. the empty batch: nothing else is looked at -- but the sizes are
    nothing = {n: None for n in NAMES if n not in NUMBERS}
    rows.append(("empty batch, all pointers NULL", dict(b=0, wsb=0, **nothing), OK))
    rows.append(("empty batch, wild ids", dict(b=0, wsb=0, **nothing, kid=99, mid=7, nm=8, lsc=9), OK))
    rows.append(("empty batch, k beyond the limit", dict(b=0, k=5000, wsb=0, **nothing), OK))
    rows.append(("empty batch, k < 1", dict(b=0, k=0), EINVAL))
    # 3. pointers, cotangents, outputs, ids, workspace
    rows += [(f"{p} NULL", {p: None}, EINVAL) for p in ("feat", "ni", "tg", "ls")]
    rows.append(("grad_ykinvy with R = 3", dict(R=3), EINVAL))
    rows.append(("all three cotangents NULL", dict(gm=None, gv=None, gyk=None), EINVAL))
    rows.append(("both outputs NULL", dict(gls=None, gnz=None), EINVAL))
    rows += [(f"kernel id {i}", dict(kid=i), EINVAL) for i in (-1, 6, 99)]
    rows += [(f"metric id {i}", dict(mid=i), EINVAL) for i in (-1, 2)]
    rows += [(f"noise mode {i}", dict(nm=i), EINVAL) for i in (-1, 3)]
    rows += [(f"noise mode {i} without noise_dev", dict(nm=i, nd=None), EINVAL) for i in (1, 2)]
    rows += [(f"ls_count {i} at d = 4", dict(lsc=i), EINVAL) for i in (0, 2, 5)]
    rows.append(("workspace NULL", dict(ws=None), EINVAL))
    rows.append(("workspace misaligned", dict(ws=PTR + 8), EINVAL))
    # 4. ... and only then what the kernel does not serve
    rows.append(("the general-nu id", dict(kid=5), EUNSUPPORTED))
    rows.append(("the general-nu id, workspace NULL", dict(kid=5, ws=None), EINVAL))
    rows.append(("k + 2 = 1025", dict(k=1023), EUNSUPPORTED))
    rows.append(("k + 2 = 1025 whatever R is", dict(k=1023, R=3, gyk=None), EUNSUPPORTED))
    rows.append(("k + 2 = 1025, outputs NULL", dict(k=1023, gls=None, gnz=None), EINVAL))
    rows.append(("k + 2 = 1025, workspace misaligned", dict(k=1023, ws=PTR + 4), EINVAL))
    rows.append(("k + 2 = 1025, cotangents NULL", dict(k=1023, gm=None, gv=None, gyk=None), EINVAL))
    # sizes near INT_MAX: the row count is taken in 64 bits, and a slab whose byte count passes int64 is larger than
    # any workspace but the largest
    rows.append(("k = INT_MAX, a workspace of INT64_MAX", dict(k=INT_MAX, wsb=INT64_MAX), EUNSUPPORTED))
    rows.append(("k = INT_MAX, a workspace of 1 TiB", dict(k=INT_MAX), EINVAL))
    return rows


GRID = _rows()


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("name, changes, want", GRID, ids=[n for n, _, _ in GRID])
def test_status_of_refused_and_empty_calls(name, changes, want, suf):
    assert status(suf, **changes) == want


def test_the_forms_that_would_launch_pass_the_checks_up_to_the_workspace():
    """Every accepted combination of cotangents and outputs is refused for its (short) workspace alone: with a
    workspace the same arguments are served -- which a CPU test cannot show -- and a NULL among the required
    pointers is told apart above."""
    for suf in ES:
        short = slab(ES[suf], 5) - 1
        for form in (dict(), dict(gm=None), dict(gv=None), dict(gm=None, gv=None), dict(gyk=None), dict(gyk=None, R=3, gv=None),
                     dict(gyk=None, gm=None), dict(gls=None), dict(gnz=None), dict(bi=None), dict(lsc=4), dict(nm=1, nd=PTR),
                     dict(nm=2, nd=PTR), dict(mid=1), dict(kid=0), dict(kid=4), dict(info=None)):
            assert status(suf, wsb=short, **form) == EINVAL, (suf, form)


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_workspace_one_byte_short_of_a_slab(suf):
    es = ES[suf]
    for k in (5, 200, 1022):
        assert status(suf, k=k, wsb=slab(es, k) - 1) == EINVAL, k
    # ... and in front of the refusal of a system beyond the kernel
    assert status(suf, k=1023, wsb=15) == EINVAL


# mgp_max_nn_count_backward as the parent commit returns it (read there once)
PARENT_MAX_NN_BACKWARD_F32, PARENT_MAX_NN_BACKWARD_F64 = 137, 96


def test_existing_limits_unchanged():
    lib = _lib.load()
    assert lib.mgp_max_nn_count_backward(4) == PARENT_MAX_NN_BACKWARD_F32
    assert lib.mgp_max_nn_count_backward(8) == PARENT_MAX_NN_BACKWARD_F64
    assert lib.mgp_large_max_nn_count(4, 1) == lib.mgp_large_max_nn_count(8, 1) == 1022


@pytest.mark.parametrize("es", [4, 8])
def test_workspace_sizes(es):
    lib = _lib.load()
    wb = lib.mgp_backward_large_workspace_bytes
    ks = list(range(1, 70)) + [126, 127, 128, 129, 200, 300, 511, 512, 513, 1000, 1021, 1022]
    bs = [0, 1, 2, 37, 255, 256, 257, 5000, 10**6]
    for b in bs:
        sizes = [wb(es, k, b) for k in ks]
        assert all(s > 0 and s % 16 == 0 and s <= 512 * MIB for s in sizes), b
        assert sizes == sorted(sizes), ("non-decreasing in k", b)
    for k in (1, 33, 200, 1000, 1022):
        sizes = [wb(es, k, b) for b in bs]
        assert sizes == sorted(sizes), ("non-decreasing in b", k)
        assert sizes[0] == sizes[1] == slab(es, k)  # (at least one slab)
        # a backward slab holds the forward's trapezoid of k + 2 rows and all (k + 1) k / 2 pair distances
        assert slab(es, k) >= lib.mgp_large_workspace_bytes(es, k, 1, 1) + (k + 1) * k // 2 * es
    # beyond the limit, and for arguments nothing serves
    assert wb(es, 1023, 8) == 0 and wb(es, 5000, 8) == 0 and wb(es, INT_MAX, 8) == 0
    assert wb(es, 0, 8) == 0 and wb(es, 5, -1) == 0
    assert wb(2, 5, 8) == 0
    # the cap binds for the largest systems
    assert wb(es, 1022, 10**6) == 512 * MIB


def test_no_spills_no_scratch():
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), "kernel_resources.json")
    with open(path) as f:
        res = json.load(f)
    mine = {n: r for n, r in res.items() if "hyper_backward_large_kernel" in n}
    assert len(mine) == 2, sorted(mine)  # two float widths
    for name, r in mine.items():
        assert r["VGPRs Spill"] == 0, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
    # ... and the name stays clear of the forward kernels' (tests/test_large_status_cpu.py counts those by name)
    assert not any("fused_large_kernel" in n or "solve_large_kernel" in n for n in mine)


def test_edge_sample_of_the_gpu_tests_covers_every_factor():
    """The seeded sample tests/test_gpu_large_backward.py::test_block_and_tile_edges runs: every value of every factor
    appears, and so do the combinations at which the kernel takes a path of its own."""
    from tests.test_gpu_large_backward import EDGE_CASES, EDGE_D, EDGE_K, FORMS, KERNELS, WANTS

    seen = {name: {c[name] for c in EDGE_CASES} for name in EDGE_CASES[0]}
    assert seen["k"] == set(EDGE_K) and seen["d"] == set(EDGE_D) and seen["kernel"] == set(KERNELS)
    assert seen["metric"] == {"l2", "F2"} and seen["noise"] == {"scalar", "table", "batch"}
    assert seen["aniso"] == {False, True} and seen["bi"] == {False, True}
    assert seen["dtype"] == {"float32", "float64"} and seen["form"] == set(FORMS) and seen["want"] == set(WANTS)
    # both float widths on either side of the block-size switch, and two feature chunks with per-feature scales
    assert {(k, t) for k in (126, 127) for t in ("float32", "float64")} <= {(c["k"], c["dtype"]) for c in EDGE_CASES if c["aniso"]}
    assert {"float32", "float64"} == {c["dtype"] for c in EDGE_CASES if c["d"] == 70 and c["aniso"] and "ls" in c["want"]}
