"""CPU: the vector-Jacobian product of the general-smoothness Matern in LDS (mgp_posterior_backward_gen_*;
include/muygpys_hip.h) -- the status of every refused or empty call, decided BEFORE any HIP call and in the order the
header states; the closed-form entries' unchanged refusal of the general-nu id; the query function; the compiler's
register record of the four instantiations.

One rule is violated per row, starting from arguments that would launch.  Host buffers stand in for device pointers:
nothing dereferences them before the status is decided.  No row here reaches a launch."""

import ctypes as C
import json
import os

import pytest

from muygpys_amd import _lib

OK, EINVAL, EUNSUPPORTED = 0, -1, -2
ES = {"f32": 4, "f64": 8}
INT_MAX = 2**31 - 1

NAMES = "fq fn d bi ni b k tg R nm eps nd nu mid ls lsc gm gv gyk gfq gfn gtg gls gnz gnu info st".split()
NUMBERS = dict(d=4, b=3, k=5, R=1, nm=0, eps=1e-3, nu=1.3, mid=0, lsc=1)
OPTIONAL = ("nd", "st")
OUTPUTS = ("gfq", "gfn", "gtg", "gls", "gnz", "gnu")
COTANGENTS = ("gm", "gv", "gyk")
BUF = (C.c_double * 64)()
PTR = C.addressof(BUF)
NAN = float("nan")


def status(suf, **changes):
    args = {n: NUMBERS[n] if n in NUMBERS else (None if n in OPTIONAL else PTR) for n in NAMES}
    unknown = set(changes) - set(NAMES)
    assert not unknown, unknown
    args.update(changes)
    return getattr(_lib.load(), f"mgp_posterior_backward_gen_{suf}")(*[args[n] for n in NAMES])


def limit(suf):
    return _lib.load().mgp_max_nn_count_backward_gen(ES[suf])


def _rows():
    no_outputs = {n: None for n in OUTPUTS}
    no_cotangents = {n: None for n in COTANGENTS}
    # 1. sizes, and a smoothness that is not > 0
    rows = [("b < 0", dict(b=-1), EINVAL), ("k < 1", dict(k=0), EINVAL), ("d < 1", dict(d=0), EINVAL),
            ("R < 1", dict(R=0), EINVAL), ("nu = 0", dict(nu=0.0), EINVAL), ("nu < 0", dict(nu=-1.5), EINVAL),
            ("nu NaN", dict(nu=NAN), EINVAL)]
    # 2. the empty batch: nothing else is looked at -- but the sizes and the smoothness's sign are
    nothing = {n: None for n in NAMES if n not in NUMBERS}
    rows.append(("empty batch, all pointers NULL", dict(b=0, **nothing), OK))
    rows.append(("empty batch, wild ids", dict(b=0, **nothing, mid=7, nm=8, lsc=9), OK))
    rows.append(("empty batch, k beyond the limit", dict(b=0, k=5000, **nothing), OK))
    rows.append(("empty batch, nu beyond the limit", dict(b=0, nu=31.0, **nothing), OK))
    rows.append(("empty batch, k < 1", dict(b=0, k=0), EINVAL))
    rows.append(("empty batch, nu = 0", dict(b=0, nu=0.0), EINVAL))
    rows.append(("empty batch, nu NaN", dict(b=0, nu=NAN), EINVAL))
    # 3. pointers, cotangents, outputs, ids
    rows += [(f"{p} NULL", {p: None}, EINVAL) for p in ("fq", "fn", "ni", "tg", "ls")]
    rows.append(("all three cotangents NULL", no_cotangents, EINVAL))
    rows.append(("all six outputs NULL", no_outputs, EINVAL))
    rows.append(("grad_ykinvy with R = 3", dict(R=3), EINVAL))
    rows += [(f"metric id {i}", dict(mid=i), EINVAL) for i in (-1, 2)]
    rows += [(f"noise mode {i}", dict(nm=i), EINVAL) for i in (-1, 3)]
    rows += [(f"noise mode {i} without noise_dev", dict(nm=i, nd=None), EINVAL) for i in (1, 2)]
    rows += [(f"ls_count {i} at d = 4", dict(lsc=i), EINVAL) for i in (0, 2, 5)]
    # 4. ... and only then what the kernel does not serve
    rows.append(("nu = 30.5", dict(nu=30.5), EUNSUPPORTED))
    rows.append(("nu = inf", dict(nu=float("inf")), EUNSUPPORTED))
    rows.append(("nu = 30.5, outputs NULL", dict(nu=30.5, **no_outputs), EINVAL))
    rows.append(("nu = 30.5, metric id 2", dict(nu=30.5, mid=2), EINVAL))
    rows.append(("nu = 30.5, cotangents NULL", dict(nu=30.5, **no_cotangents), EINVAL))
    for k in ("limit+1", 1023, INT_MAX):
        rows.append((f"k = {k}", dict(k=k), EUNSUPPORTED))
        rows.append((f"k = {k} whatever R is", dict(k=k, R=3, gyk=None), EUNSUPPORTED))
        rows.append((f"k = {k}, outputs NULL", dict(k=k, **no_outputs), EINVAL))
        rows.append((f"k = {k}, cotangents NULL", dict(k=k, **no_cotangents), EINVAL))
        rows.append((f"k = {k}, noise mode 2 without noise_dev", dict(k=k, nm=2, nd=None), EINVAL))
    return rows


GRID = _rows()


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("name, changes, want", GRID, ids=[n for n, _, _ in GRID])
def test_status_of_refused_and_empty_calls(name, changes, want, suf):
    if changes.get("k") == "limit+1":
        changes = dict(changes, k=limit(suf) + 1)
    assert status(suf, **changes) == want


def test_query_function():
    lib = _lib.load()
    for es in (4, 8):
        got = lib.mgp_max_nn_count_backward_gen(es)
        # the closed-form kernel's carve with both node tables behind it: fewer rows fit, but a useful number of them
        assert 64 <= got <= lib.mgp_max_nn_count_backward(es), (es, got)
    assert lib.mgp_max_nn_count_backward_gen(8) < lib.mgp_max_nn_count_backward_gen(4)
    for es in (0, 2, 16, -4):
        assert lib.mgp_max_nn_count_backward_gen(es) == EINVAL


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("kid_entry", ["posterior_backward", "loocv_backward"])
def test_the_closed_form_entries_still_refuse_the_general_nu_id(kid_entry, suf):
    if kid_entry == "posterior_backward":
        names = "fq fn d bi ni b k tg R nm eps nd kid mid ls lsc gm gv gfq gfn gtg gls gnz info st".split()
    else:
        names = "fq d bi ni b k tg nm eps nd kid mid ls lsc gm gv gyk gls gnz info st".split()
    numbers = dict(d=4, b=3, k=5, R=1, nm=0, eps=1e-3, kid=_lib.KERNEL_IDS["matern_gen"], mid=0, lsc=1)
    args = {n: numbers[n] if n in numbers else (None if n in OPTIONAL else PTR) for n in names}
    fn = getattr(_lib.load(), f"mgp_{kid_entry}_{suf}")
    assert fn(*[args[n] for n in names]) == EINVAL  # (not a kernel id of these entries: refused with the ids)


def test_no_spills_no_scratch():
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), "kernel_resources.json")
    with open(path) as f:
        res = json.load(f)
    mine = {n: r for n, r in res.items() if "backward_gen_kernel" in n}
    assert len(mine) == 4, sorted(mine)  # two float widths, with and without grad_nu
    for name, r in mine.items():
        assert r["VGPRs Spill"] == 0, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
