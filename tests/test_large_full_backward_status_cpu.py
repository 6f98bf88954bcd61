"""CPU: the whole posterior backward beyond LDS (mgp_posterior_backward_large_*; include/muygpys_hip.h) -- the status of
every refused or empty call, decided BEFORE any HIP call and in the order the header states, the compiler's register
record of the new kernel next to the pinned counts of its neighbours, the factors of the GPU file's edge sample, and
the opt-in of ``autograd.posterior``.

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

NAMES = "fq fn d bi ni b k tg R nm eps nd kid mid ls lsc gm gv gfq gfn gtg gls gnz info ws wsb st".split()
NUMBERS = dict(d=4, b=3, k=5, R=1, nm=0, eps=1e-3, kid=2, mid=0, lsc=1, wsb=1 << 40)
OPTIONAL = ("nd", "st")
OUTPUTS = ("gfq", "gfn", "gtg", "gls", "gnz")
BUF = (C.c_double * 64)()
PTR = C.addressof(BUF)  # (16-byte aligned: ctypes arrays of doubles come from malloc)
assert PTR % 16 == 0


def status(suf, **changes):
    args = {n: NUMBERS[n] if n in NUMBERS else (None if n in OPTIONAL else PTR) for n in NAMES}
    unknown = set(changes) - set(NAMES)
    assert not unknown, unknown
    args.update(changes)
    return getattr(_lib.load(), f"mgp_posterior_backward_large_{suf}")(*[args[n] for n in NAMES])


def slab(es, k):
    """What one system occupies: the recommended workspace of a batch of one."""
    return _lib.load().mgp_backward_large_workspace_bytes(es, k, 1)


def _rows():
    no_outputs = {n: None for n in OUTPUTS}
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
    rows += [(f"{p} NULL", {p: None}, EINVAL) for p in ("fq", "fn", "ni", "tg", "ls")]
    rows.append(("both cotangents NULL", dict(gm=None, gv=None), EINVAL))
    rows.append(("all five outputs NULL", no_outputs, EINVAL))
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
    rows.append(("k + 2 = 1025 whatever R is", dict(k=1023, R=3), EUNSUPPORTED))
    rows.append(("k + 2 = 1025, outputs NULL", dict(k=1023, **no_outputs), EINVAL))
    rows.append(("k + 2 = 1025, workspace misaligned", dict(k=1023, ws=PTR + 4), EINVAL))
    rows.append(("k + 2 = 1025, cotangents NULL", dict(k=1023, gm=None, gv=None), EINVAL))
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
        forms = [dict(), dict(gm=None), dict(gv=None), dict(R=3), dict(bi=None), dict(lsc=4), dict(nm=1, nd=PTR), dict(nm=2, nd=PTR),
                 dict(mid=1), dict(kid=0), dict(kid=4), dict(info=None), dict(fq=PTR + 16), dict(gfq=None, gfn=None),
                 dict(gtg=None), dict(gls=None, gnz=None)]
        forms += [{n: None for n in OUTPUTS if n != keep} for keep in OUTPUTS]  # one output alone, each in turn
        for form in forms:
            assert status(suf, wsb=short, **form) == EINVAL, (suf, form)


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_workspace_one_byte_short_of_a_slab(suf):
    es = ES[suf]
    for k in (5, 200, 1022):
        assert status(suf, k=k, wsb=slab(es, k) - 1) == EINVAL, k
    # ... and in front of the refusal of a system beyond the kernel
    assert status(suf, k=1023, wsb=15) == EINVAL


def test_no_spills_no_scratch_and_the_pinned_counts():
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), "kernel_resources.json")
    with open(path) as f:
        res = json.load(f)
    mine = {n: r for n, r in res.items() if "posterior_backward_large_kernel" in n}
    assert len(mine) == 2, sorted(mine)  # two float widths
    for name, r in mine.items():
        assert r["VGPRs Spill"] == 0, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
    # the three families other tests count by name are what they were
    hyper = {n: r for n, r in res.items() if "hyper_backward_large_kernel" in n}
    assert len(hyper) == 2, sorted(hyper)
    assert all(r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0 for r in hyper.values()), hyper
    assert len([n for n in res if "fused_large_kernel" in n or "solve_large_kernel" in n]) == 4


def test_edge_sample_of_the_gpu_tests_covers_every_factor():
    """The seeded sample tests/test_gpu_large_full_backward.py::test_block_and_tile_edges runs: every value of every
    factor appears, and so do the combinations at which the kernel takes a path of its own."""
    from tests.test_gpu_large_full_backward import EDGE_CASES, EDGE_D, EDGE_FORMS, EDGE_K, KERNELS
    from tests.test_gpu_large_full_backward import OUTPUTS as WANTS

    seen = {name: {c[name] for c in EDGE_CASES} for name in EDGE_CASES[0]}
    assert seen["k"] == set(EDGE_K) and seen["d"] == set(EDGE_D) and seen["kernel"] == set(KERNELS)
    assert seen["metric"] == {"l2", "F2"} and seen["noise"] == {"scalar", "table", "batch"}
    assert seen["aniso"] == {False, True} and seen["bi"] == {False, True} and seen["shared"] == {False, True}
    assert seen["R"] == {1, 3} and seen["form"] == set(EDGE_FORMS) and seen["want"] == set(WANTS)
    assert seen["dtype"] == {"float32", "float64"}
    assert all(c["metric"] == "l2" or c["kernel"] in ("rbf", "matern05") for c in EDGE_CASES)
    # both float widths on either side of the block-size switch at d = 8 with per-feature scales, and two feature
    # chunks in the sweep with every output
    full = [c for c in EDGE_CASES if c["aniso"] and c["want"] == "all"]
    assert {(k, t) for k in (126, 127) for t in ("float32", "float64")} <= {(c["k"], c["dtype"]) for c in full if c["d"] == 8}
    assert {"float32", "float64"} == {c["dtype"] for c in full if c["d"] == 70 and c["k"] == 33}


def test_autograd_opt_in_parses_without_a_gpu(monkeypatch):
    """Off by default; MUYGPYS_HIP_AUTOGRAD_LARGE=1 turns the module default on (read at import); the context manager
    sets it and restores what was there; ``posterior`` takes the keyword."""
    import importlib
    import inspect

    from muygpys_amd import autograd

    try:
        monkeypatch.delenv("MUYGPYS_HIP_AUTOGRAD_LARGE", raising=False)
        assert importlib.reload(autograd).beyond_lds_default() is False
        for value, want in (("0", False), ("", False), ("1", True)):
            monkeypatch.setenv("MUYGPYS_HIP_AUTOGRAD_LARGE", value)
            assert importlib.reload(autograd).beyond_lds_default() is want, value
        with autograd.beyond_lds(False):
            assert autograd.beyond_lds_default() is False
            with autograd.beyond_lds(True):
                assert autograd.beyond_lds_default() is True
            assert autograd.beyond_lds_default() is False
        assert autograd.beyond_lds_default() is True
    finally:
        monkeypatch.delenv("MUYGPYS_HIP_AUTOGRAD_LARGE", raising=False)
        autograd = importlib.reload(autograd)
    assert autograd.beyond_lds_default() is False
    with pytest.raises(RuntimeError):
        with autograd.beyond_lds(True):
            assert autograd.beyond_lds_default() is True
            raise RuntimeError("leaves the block")
    assert autograd.beyond_lds_default() is False
    p = inspect.signature(autograd.posterior).parameters["beyond_lds"]
    assert p.default is None and list(inspect.signature(autograd.posterior).parameters)[-1] == "beyond_lds"
    # the layers take it after the reference's five positional arguments
    from muygpys_amd.torch import MultivariateMuyGPs_layer, MuyGPs_layer

    for cls in (MuyGPs_layer, MultivariateMuyGPs_layer):
        params = list(inspect.signature(cls.__init__).parameters.values())
        assert params[6].name == "beyond_lds" and params[6].default is False and len(params) == 7
