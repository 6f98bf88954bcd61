"""CPU: the hyper-parameter backward of the general-smoothness Matern on the slab factor
(mgp_hyper_backward_gen_large_*; include/muygpys_hip.h) -- the status of every refused or empty call, decided BEFORE any
HIP call and in the order the header states; the closed-form entry's unchanged refusal of the general-nu id; the query
function; the compiler's register record of the new kernels.

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

NAMES = "feat d bi ni b k tg R nm eps nd nu mid ls lsc gm gv gyk gls gnz gnu info ws wsb st".split()
NUMBERS = dict(d=4, b=3, k=5, R=1, nm=0, eps=1e-3, nu=1.3, mid=0, lsc=1, wsb=1 << 40)
OPTIONAL = ("nd", "st")
OUTPUTS = ("gls", "gnz", "gnu")
COTANGENTS = ("gm", "gv", "gyk")
BUF = (C.c_double * 64)()
PTR = C.addressof(BUF)  # (16-byte aligned: ctypes arrays of doubles come from malloc)
assert PTR % 16 == 0
NAN = float("nan")


def status(suf, **changes):
    args = {n: NUMBERS[n] if n in NUMBERS else (None if n in OPTIONAL else PTR) for n in NAMES}
    unknown = set(changes) - set(NAMES)
    assert not unknown, unknown
    args.update(changes)
    return getattr(_lib.load(), f"mgp_hyper_backward_gen_large_{suf}")(*[args[n] for n in NAMES])


def slab(es, k):
    """What one system occupies: the recommended workspace of a batch of one."""
    return _lib.load().mgp_backward_large_workspace_bytes(es, k, 1)


def _rows():
    no_outputs = {n: None for n in OUTPUTS}
    no_cotangents = {n: None for n in COTANGENTS}
    # 1. sizes, and a smoothness that is not > 0
    rows = [("b < 0", dict(b=-1), EINVAL), ("k < 1", dict(k=0), EINVAL), ("d < 1", dict(d=0), EINVAL),
            ("R < 1", dict(R=0), EINVAL), ("nu = 0", dict(nu=0.0), EINVAL), ("nu < 0", dict(nu=-1.5), EINVAL),
            ("nu NaN", dict(nu=NAN), EINVAL)]
    # 2. the empty batch: nothing else is looked at -- but the sizes and the smoothness's sign are
    nothing = {n: None for n in NAMES if n not in NUMBERS}
    rows.append(("empty batch, all pointers NULL", dict(b=0, wsb=0, **nothing), OK))
    rows.append(("empty batch, wild ids", dict(b=0, wsb=0, **nothing, mid=7, nm=8, lsc=9), OK))
    rows.append(("empty batch, k beyond the limit", dict(b=0, k=5000, wsb=0, **nothing), OK))
    rows.append(("empty batch, nu beyond the limit", dict(b=0, nu=31.0, wsb=0, **nothing), OK))
    rows.append(("empty batch, k < 1", dict(b=0, k=0), EINVAL))
    rows.append(("empty batch, nu = 0", dict(b=0, nu=0.0), EINVAL))
    rows.append(("empty batch, nu NaN", dict(b=0, nu=NAN), EINVAL))
    # 3. pointers, cotangents, outputs, ids, workspace
    rows += [(f"{p} NULL", {p: None}, EINVAL) for p in ("feat", "ni", "tg", "ls")]
    rows.append(("all three cotangents NULL", no_cotangents, EINVAL))
    rows.append(("all three outputs NULL", no_outputs, EINVAL))
    rows.append(("grad_ykinvy with R = 3", dict(R=3), EINVAL))
    rows += [(f"metric id {i}", dict(mid=i), EINVAL) for i in (-1, 2)]
    rows += [(f"noise mode {i}", dict(nm=i), EINVAL) for i in (-1, 3)]
    rows += [(f"noise mode {i} without noise_dev", dict(nm=i, nd=None), EINVAL) for i in (1, 2)]
    rows += [(f"ls_count {i} at d = 4", dict(lsc=i), EINVAL) for i in (0, 2, 5)]
    rows.append(("workspace NULL", dict(ws=None), EINVAL))
    rows.append(("workspace misaligned", dict(ws=PTR + 8), EINVAL))
    # 4. ... and only then what the kernel does not serve
    rows.append(("nu = 30.5", dict(nu=30.5), EUNSUPPORTED))
    rows.append(("nu = inf", dict(nu=float("inf")), EUNSUPPORTED))
    rows.append(("nu = 30.5, workspace NULL", dict(nu=30.5, ws=None), EINVAL))
    rows.append(("nu = 30.5, outputs NULL", dict(nu=30.5, **no_outputs), EINVAL))
    rows.append(("nu = 30.5, metric id 2", dict(nu=30.5, mid=2), EINVAL))
    rows.append(("k + 2 = 1025", dict(k=1023), EUNSUPPORTED))
    rows.append(("k + 2 = 1025 whatever R is", dict(k=1023, R=3, gyk=None), EUNSUPPORTED))
    rows.append(("k + 2 = 1025, outputs NULL", dict(k=1023, **no_outputs), EINVAL))
    rows.append(("k + 2 = 1025, workspace misaligned", dict(k=1023, ws=PTR + 4), EINVAL))
    rows.append(("k + 2 = 1025, cotangents NULL", dict(k=1023, **no_cotangents), EINVAL))
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
        forms = [dict(), dict(gm=None), dict(gv=None), dict(gm=None, gv=None), dict(gyk=None), dict(gyk=None, R=3),
                 dict(gyk=None, gv=None, R=3), dict(bi=None), dict(lsc=4), dict(nm=1, nd=PTR), dict(nm=2, nd=PTR), dict(mid=1),
                 dict(info=None), dict(feat=PTR + 16), dict(nu=0.01), dict(nu=30.0), dict(nu=0.5)]
        # every non-empty subset of the three outputs
        for m in range(1, 8):
            forms.append({n: None for i, n in enumerate(OUTPUTS) if not (m >> i) & 1})
        for form in forms:
            assert status(suf, wsb=short, **form) == EINVAL, (suf, form)


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_workspace_one_byte_short_of_a_slab(suf):
    es = ES[suf]
    for k in (5, 200, 1022):
        assert status(suf, k=k, wsb=slab(es, k) - 1) == EINVAL, k
    assert status(suf, k=1023, wsb=15) == EINVAL


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_the_closed_form_entry_still_refuses_the_general_nu_id(suf):
    names = "feat d bi ni b k tg R nm eps nd kid mid ls lsc gm gv gyk gls gnz info ws wsb st".split()
    numbers = dict(d=4, b=3, k=5, R=1, nm=0, eps=1e-3, kid=5, mid=0, lsc=1, wsb=1 << 40)
    args = {n: numbers[n] if n in numbers else (None if n in OPTIONAL else PTR) for n in names}
    fn = getattr(_lib.load(), f"mgp_hyper_backward_large_{suf}")
    assert fn(*[args[n] for n in names]) == EUNSUPPORTED
    args["ws"] = None  # (... behind the pointer checks, as before)
    assert fn(*[args[n] for n in names]) == EINVAL
    args.update(ws=PTR, kid=2, wsb=slab(ES[suf], 5) - 1)
    assert fn(*[args[n] for n in names]) == EINVAL


def test_query_function():
    lib = _lib.load()
    # both node tables fit LDS next to the closed-form entry's carve over its whole range, in both widths
    assert lib.mgp_backward_gen_large_max_nn_count(4) == 1022
    assert lib.mgp_backward_gen_large_max_nn_count(8) == 1022
    for es in (0, 2, 16, -4):
        assert lib.mgp_backward_gen_large_max_nn_count(es) == EINVAL
    # ... and at the limit the entry gets as far as the workspace, one beyond it is refused
    for suf, es in ES.items():
        assert status(suf, k=1022, wsb=slab(es, 1022) - 1) == EINVAL
        assert status(suf, k=1023) == EUNSUPPORTED


def test_no_spills_no_scratch():
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), "kernel_resources.json")
    with open(path) as f:
        res = json.load(f)
    mine = {n: r for n, r in res.items() if "hyper_backward_gen_large_kernel" in n}
    assert len(mine) == 4, sorted(mine)  # two float widths, with and without grad_nu
    for name, r in mine.items():
        assert r["VGPRs Spill"] == 0, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
    # the closed-form kernel's records are looked at by its own tests: still two
    assert len([n for n in res if "hyper_backward_large_kernel" in n]) == 2
