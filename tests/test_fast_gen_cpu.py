"""CPU: the general-smoothness fast-posterior-mean route (``fused.gen_fast``; mgp_fast_coefficients_gen_*,
mgp_fast_posterior_mean_gen_*; include/muygpys_hip.h) without a device.

* what ``fused.fast_coefficients`` / ``fused.fast_posterior_mean`` / the lazy layer hand the library in either mode
  (tests/call_recorder.py), the mode switch and its environment variable;
* the status grid of the four new entries and the workspace query: one rule violated per row, every status decided
  BEFORE any HIP call, host buffers standing in for device pointers.  No row here reaches a launch;
* the case lists of tests/test_gpu_fast_gen.py (tests/fast_gen_cases.py): every factor meets several k and d, and the
  fp32 evaluator's own error (tests/test_matern_gen_cpu.py::_matern_gen_trapezoid_fp32 in the oracle's place, the solve
  kept in fp64) moves no fp32 case by more than a quarter of the band asserted on the device;
* the half-wave node bound of csrc/mgp_gen_group.h restated in numpy float32 against scipy;
* the compiler's resource records: the new instantiations without spills, the kernels that existed before as recorded
  from the parent build (tests/golden/parent_bits/fast_gen_kernel_resources.json, data only).

Eleven tests here do not need the feature and pass without it, by design: the two coverage tests and the quarter-band
test are conditions on the case lists (numpy and the oracle only), the seven half-wave tests restate arithmetic in
numpy, and test_the_closed_form_entries_still_refuse_the_general_nu_id pins entries that existed before.  Every other
test of this file, and every test of tests/test_gpu_fast_gen.py, fails without the feature at the first missing
symbol or attribute."""

import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from muygpys_amd import _lib, fused
from muygpys_amd.fused import KernelSpec
from tests import fast_gen_cases as G
from tests.call_recorder import STREAM, install, vals
from tests.test_matern_gen_cpu import _gen_step, _matern_gen_trapezoid_fp32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED = 0, -1, -2
ES = {"f32": 4, "f64": 8}
INT_MAX, INT64_MAX = 2**31 - 1, 2**63 - 1
NAN = float("nan")
BUF = (C.c_double * 64)()
PTR = C.addressof(BUF)
assert PTR % 16 == 0


def lds_limit(dtype, R):
    return _lib.load().mgp_max_nn_count_gen(4 if dtype in ("float32", torch.float32) else 8, R)


# ---- routing ------------------------------------------------------------------------------------------------------------
D, N = 3, 40
GEN = KernelSpec("matern_gen", "l2", (2.0, 3.0, 4.0), 1e-3, smoothness=0.8)


@pytest.fixture
def rec(monkeypatch):
    yield install(monkeypatch)
    fused.clear_caches()


@pytest.fixture
def solved(monkeypatch):
    from muygpys_amd._src.gp.muygps import hip as M

    seen = []
    monkeypatch.setattr(M, "_solve", lambda Kin, Kc, Y, kout=1.0, want=("mean",): (
        seen.append(tuple(Kin.shape)), (None, None, None, torch.zeros(Y.shape, dtype=Y.dtype)))[1])
    return seen


def inputs(k, R, dtype=torch.float32, n=N):
    g = torch.Generator().manual_seed(k + R)
    X = torch.randn(n, D, generator=g).to(dtype)
    Y = (torch.randn(n, generator=g) if R == 0 else torch.randn(n, R, generator=g)).to(dtype)
    nn = torch.randint(0, n, (n, k), generator=g)
    return X, Y, nn


def names(rec):
    return [c[0] for c in rec.calls]


def test_mode_switch_nests_and_restores():
    assert fused.GEN_FAST_MODES == ("materialised", "fused")
    assert fused.gen_fast_default() == "materialised"
    with fused.gen_fast("fused"):
        assert fused.gen_fast_default() == "fused"
        with fused.gen_fast("materialised"):
            assert fused.gen_fast_default() == "materialised"
            with pytest.raises(ValueError):
                with fused.gen_fast("wave"):
                    pass
            assert fused.gen_fast_default() == "materialised"
        assert fused.gen_fast_default() == "fused"
        with pytest.raises(RuntimeError):
            with fused.gen_fast("fused"):
                raise RuntimeError("inside")
        assert fused.gen_fast_default() == "fused"
    assert fused.gen_fast_default() == "materialised"


def _child(env_extra, code):
    env = dict(os.environ, PYTHONPATH=ROOT, **env_extra)
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)


def test_environment_variable():
    code = "from muygpys_amd import fused; print('mode', fused.gen_fast_default())"
    r = _child({"MUYGPYS_HIP_GEN_FAST": "fused"}, code)
    assert r.returncode == 0 and "mode fused" in r.stdout, r.stderr[-2000:]
    r = _child({"MUYGPYS_HIP_GEN_FAST": ""}, code)
    assert r.returncode == 0 and "mode materialised" in r.stdout, r.stderr[-2000:]
    r = _child({"MUYGPYS_HIP_GEN_FAST": "wave"}, code)
    assert r.returncode != 0 and "ValueError" in r.stderr and "MUYGPYS_HIP_GEN_FAST='wave'" in r.stderr, r.stderr[-2000:]


@pytest.mark.parametrize("k, R", [(30, 0), (62, 0), (70, 2)])
def test_default_mode_makes_the_calls_it_always_made(rec, solved, k, R):
    X, Y, nn = inputs(k, R)
    fused.fast_coefficients(GEN, X, Y, nn)
    today = names(rec)
    assert "matern_gen" in today and not [n for n in today if n.startswith("fast_")], today
    assert solved == [(N, k, k)]
    rec.calls.clear()
    with fused.gen_fast("materialised"):
        fused.fast_coefficients(GEN, X, Y, nn)
    assert names(rec) == today
    rec.calls.clear()
    with fused.gen_fast("fused"):
        fused.fast_coefficients(GEN, X, Y, nn, fused=False)  # (the caller's own choice of the materialising route stands)
    assert names(rec) == today


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("k, R", [(30, 0), (62, 0), (5, 2), ("L", 3), ("L+1", 3), (300, 0), (1020, 3)])
def test_fused_mode_is_one_call_of_the_new_entry(rec, solved, k, R, dtype):
    # fn, d, ni, b, k, tg, R, noise_mode, eps, nd, smoothness, metric, ls, ls_count, coeffs, info, workspace, workspace_bytes, stream
    L = lds_limit(dtype, max(R, 1))
    k = k if isinstance(k, int) else L + (k == "L+1")
    X, Y, nn = inputs(k, R, dtype)
    with fused.gen_fast("fused"):
        out, nn_fast = fused.fast_coefficients(GEN, X, Y, nn)
    assert out.shape == ((N, k) if R == 0 else (N, k, R)) and out.dtype == dtype and not solved
    (call,) = rec.calls
    v = vals(call)
    assert call[0] == "fast_coefficients_gen" and call[1] == dtype and len(v) == 19
    assert v[0:10] == [X.data_ptr(), D, nn_fast.data_ptr(), N, k, Y.data_ptr(), max(R, 1), 0, 1e-3, None]
    assert v[10] == 0.8 and isinstance(v[10], float)  # the smoothness, where the closed-form entry takes the kernel id
    assert v[11] == 0 and v[12] is not None and v[13] == 3 and v[14] == out.data_ptr() and v[15] is not None
    want = _lib.load().mgp_fast_coefficients_gen_workspace_bytes(dtype.itemsize, k, max(R, 1), N)
    assert (want > 0) == (k > L)
    assert (v[16] is not None) == (k > L) and v[17] == want and v[18] == STREAM
    if k > L:
        assert v[16] % 16 == 0


def test_fused_mode_falls_back_behind_a_refusal_and_raises_on_an_error(rec, solved):
    X, Y, nn = inputs(70, 2)
    rec.statuses["fast_coefficients_gen"] = [-2]  # MGP_EUNSUPPORTED (nu > 30): the materialising route, no error
    with fused.gen_fast("fused"):
        out, _ = fused.fast_coefficients(GEN, X, Y, nn)
    assert names(rec)[0] == "fast_coefficients_gen" and "matern_gen" in names(rec) and solved == [(N, 70, 70)]
    assert out.shape == (N, 70, 2)
    rec.calls.clear()
    rec.statuses["fast_coefficients_gen"] = [-1]
    with fused.gen_fast("fused"), pytest.raises(_lib.HipLibraryError):
        fused.fast_coefficients(GEN, X, Y, nn)
    # more than 1024 rows: no fused call at all, as for the closed forms
    rec.calls.clear()
    solved.clear()
    X, Y, nn = inputs(1021, 3)
    with fused.gen_fast("fused"):
        fused.fast_coefficients(GEN, X, Y, nn)
    assert "fast_coefficients_gen" not in names(rec) and solved == [(N, 1021, 1021)]


@pytest.mark.parametrize("nu", [None, 0.0, -1.0])
def test_a_missing_or_non_positive_smoothness_raises_in_the_fused_mode(rec, nu):
    X, Y, nn = inputs(30, 0)
    spec = KernelSpec("matern_gen", "l2", 2.0, 1e-3, smoothness=nu)
    with fused.gen_fast("fused"):
        with pytest.raises(ValueError, match="needs a positive smoothness"):
            fused.fast_coefficients(spec, X, Y, nn)
        co = torch.zeros(N, 30)
        with pytest.raises(ValueError, match="needs a positive smoothness"):
            fused.fast_posterior_mean(spec, X, X, None, nn, co, torch.arange(N))
    assert not rec.calls


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("k, R", [(30, 0), (63, 3), (100, 3)])
def test_prediction_is_one_call_of_the_new_entry(rec, k, R, dtype):
    # fq, fn, d, bi, ni, b, k, coeffs, crow, R, smoothness, metric, ls, ls_count, mean, stream
    X, _, nn = inputs(k, R, dtype)
    Q = torch.randn(7, D).to(dtype)
    co = torch.randn((N, k) if R == 0 else (N, k, R)).to(dtype)
    crow, bi, ni = torch.arange(7) * 3, torch.arange(7), nn[:7].contiguous()
    with fused.gen_fast("fused"):
        out = fused.fast_posterior_mean(GEN, Q, X, bi, ni, co, crow)
    assert out.shape == ((7,) if R == 0 else (7, R))
    (call,) = rec.calls
    v = vals(call)
    assert call[0] == "fast_posterior_mean_gen" and call[1] == dtype and len(v) == 16
    assert v[0:7] == [Q.data_ptr(), X.data_ptr(), D, bi.data_ptr(), ni.data_ptr(), 7, k]
    assert v[8] == crow.data_ptr() and v[9] == max(R, 1) and v[10] == 0.8 and isinstance(v[10], float)
    assert v[11] == 0 and v[12] is not None and v[13] == 3 and v[14] is not None and v[15] == STREAM
    rec.calls.clear()
    rec.statuses["fast_posterior_mean_gen"] = [-2]
    with fused.gen_fast("fused"), pytest.raises(fused.FusedUnsupported):
        fused.fast_posterior_mean(GEN, Q, X, bi, ni, co, crow)
    rec.statuses["fast_posterior_mean_gen"] = [-1]
    with fused.gen_fast("fused"), pytest.raises(_lib.HipLibraryError):
        fused.fast_posterior_mean(GEN, Q, X, bi, ni, co, crow)
    # the default mode: the closed-form entry with the general-nu id, as before (the library answers MGP_EINVAL there)
    rec.calls.clear()
    fused.fast_posterior_mean(GEN, Q, X, bi, ni, co, crow)
    (call,) = rec.calls
    assert call[0] == "fast_posterior_mean" and vals(call)[10] == _lib.KERNEL_IDS["matern_gen"]


def test_the_lazy_layer_reaches_both_entries_in_the_fused_mode_alone(rec, solved):
    from muygpys_amd import lazy, lazy_eval
    from muygpys_amd._src.gp.muygps import hip as M

    k = 30
    X, Y, nn = inputs(k, 0)
    pair = lazy.LazyDiffs("pairwise", "l2", True, X, nn)
    Kin = lazy.LazyCov(pair, "matern_gen", 1e-3, smoothness=0.8)
    tg = lazy.LazyTargets(Y, nn)
    assert M._precompute_fused(Kin, tg) is None and not rec.calls
    with fused.gen_fast("fused"):
        co = M._precompute_fused(Kin, tg)
    assert names(rec) == ["fast_coefficients_gen"] and tuple(co.shape) == (N, k, 1)
    assert vals(rec.calls[0])[10] == 0.8
    rec.calls.clear()
    Q, bi, rows = torch.randn(7, D), torch.arange(7), torch.arange(7) * 2
    ni = nn[:7].contiguous()
    Kcross = lazy.LazyCov(lazy.LazyDiffs("crosswise", "l2", True, X, ni, Q, bi), "matern_gen", smoothness=0.8)

    class OnDevice(torch.Tensor):  # (fast_mean serves device tensors only; nothing dereferences this one)
        is_cuda = property(lambda self: True)

    table = torch.randn(N, k).as_subclass(OnDevice)
    assert lazy_eval.fast_mean(Kcross, table, rows=rows) is None and not rec.calls
    with fused.gen_fast("fused"):
        out = lazy_eval.fast_mean(Kcross, table, rows=rows)
        assert names(rec) == ["fast_posterior_mean_gen"] and tuple(out.shape) == (7,)
        assert vals(rec.calls[0])[10] == 0.8
        rec.statuses["fast_posterior_mean_gen"] = [-2]
        assert lazy_eval.fast_mean(Kcross, table, rows=rows) is None  # (a refusal: the caller materialises)


# ---- the status grid --------------------------------------------------------------------------------------------------------
COEF_NAMES = "fn d ni b k tg R nm eps nd nu mid ls lsc coeffs info ws wsb st".split()
COEF_NUMBERS = dict(d=4, b=3, k=300, R=1, nm=0, eps=1e-3, nu=30.5, mid=0, lsc=1, wsb=1 << 40)
MEAN_NAMES = "fq fn d bi ni b k coeffs crow R nu mid ls lsc mean st".split()
MEAN_NUMBERS = dict(d=4, b=3, k=300, R=1, nu=30.5, mid=0, lsc=1)


def coef_status(suf, **changes):
    """Starting from arguments every check but the last accepts (k = 300: beyond LDS for either width, a workspace of
    1 TiB; nu = 30.5: MGP_EUNSUPPORTED instead of a launch)."""
    args = {n: COEF_NUMBERS[n] if n in COEF_NUMBERS else (None if n in ("nd", "st", "info") else PTR) for n in COEF_NAMES}
    assert not set(changes) - set(COEF_NAMES)
    args.update(changes)
    return getattr(_lib.load(), f"mgp_fast_coefficients_gen_{suf}")(*[args[n] for n in COEF_NAMES])


def mean_status(suf, **changes):
    args = {n: MEAN_NUMBERS[n] if n in MEAN_NUMBERS else (None if n in ("bi", "st") else PTR) for n in MEAN_NAMES}
    assert not set(changes) - set(MEAN_NAMES)
    args.update(changes)
    return getattr(_lib.load(), f"mgp_fast_posterior_mean_gen_{suf}")(*[args[n] for n in MEAN_NAMES])


def _nothing(names_, numbers):
    return {n: None for n in names_ if n not in numbers}


COEF_ROWS = [("b < 0", dict(b=-1), EINVAL), ("k < 1", dict(k=0), EINVAL), ("d < 1", dict(d=0), EINVAL), ("R < 1", dict(R=0), EINVAL),
             ("nu = 0", dict(nu=0.0), EINVAL), ("nu < 0", dict(nu=-1.5), EINVAL), ("nu NaN", dict(nu=NAN), EINVAL)]
COEF_ROWS += [(f"{p} NULL", {p: None}, EINVAL) for p in "fn tg ni ls coeffs".split()]
COEF_ROWS += [(f"metric id {i}", dict(mid=i), EINVAL) for i in (-1, 2)]
COEF_ROWS += [(f"noise mode {i}", dict(nm=i), EINVAL) for i in (-1, 3)]
COEF_ROWS += [(f"noise mode {i} without noise_dev", dict(nm=i, nd=None), EINVAL) for i in (1, 2)]
COEF_ROWS += [(f"ls_count {i} at d = 4", dict(lsc=i), EINVAL) for i in (0, 2, 5)]
COEF_ROWS += [
    ("nu = 30.5", dict(), EUNSUPPORTED),
    ("nu = inf", dict(nu=float("inf")), EUNSUPPORTED),
    ("nu = 30.5, info NULL", dict(info=None), EUNSUPPORTED),
    ("nu = 30.5, coeffs NULL", dict(coeffs=None), EINVAL),
    ("workspace NULL beyond LDS", dict(ws=None), EINVAL),
    ("workspace misaligned", dict(ws=PTR + 8), EINVAL),
    ("k + 1 + R = 1024, nu = 30.5", dict(k=1022), EUNSUPPORTED),
    ("k + 1 + R = 1025", dict(k=1023, nu=1.3), EUNSUPPORTED),
    ("k + 1 + R = 1025 by responses", dict(k=1008, R=16, nu=1.3), EUNSUPPORTED),
    ("k + 1 + R = 1025, coeffs NULL", dict(k=1023, nu=1.3, coeffs=None), EINVAL),
    ("k + 1 + R = 1025, workspace NULL", dict(k=1023, nu=1.3, ws=None), EINVAL),
    ("k + 1 + R = 1025, workspace misaligned", dict(k=1023, nu=1.3, ws=PTR + 4), EINVAL),
    ("k = INT_MAX", dict(k=INT_MAX, nu=1.3, wsb=INT64_MAX), EUNSUPPORTED),
    ("k = R = INT_MAX", dict(k=INT_MAX, R=INT_MAX, nu=1.3, wsb=INT64_MAX), EUNSUPPORTED),
    ("k = INT_MAX, a workspace of 1 TiB", dict(k=INT_MAX, nu=1.3), EINVAL),
    ("empty batch, all pointers NULL", dict(b=0, wsb=0, **_nothing(COEF_NAMES, COEF_NUMBERS)), OK),
    ("empty batch, ids not looked at", dict(b=0, wsb=0, **_nothing(COEF_NAMES, COEF_NUMBERS), mid=7, nm=8, lsc=9), OK),
    ("empty batch, k < 1", dict(b=0, k=0), EINVAL),
    ("empty batch, nu = 0", dict(b=0, nu=0.0), EINVAL),
    ("empty batch, nu NaN", dict(b=0, nu=NAN), EINVAL),
]

MEAN_ROWS = [("b < 0", dict(b=-1), EINVAL), ("k < 1", dict(k=0), EINVAL), ("d < 1", dict(d=0), EINVAL), ("R < 1", dict(R=0), EINVAL),
             ("nu = 0", dict(nu=0.0), EINVAL), ("nu < 0", dict(nu=-1.5), EINVAL), ("nu NaN", dict(nu=NAN), EINVAL)]
MEAN_ROWS += [(f"{p} NULL", {p: None}, EINVAL) for p in "fq fn ni coeffs crow ls mean".split()]
MEAN_ROWS += [(f"metric id {i}", dict(mid=i), EINVAL) for i in (-1, 2)]
MEAN_ROWS += [(f"ls_count {i} at d = 4", dict(lsc=i), EINVAL) for i in (0, 2, 5)]
MEAN_ROWS += [
    ("nu = 30.5", dict(), EUNSUPPORTED),
    ("nu = inf", dict(nu=float("inf")), EUNSUPPORTED),
    ("nu = 30.5 at k = 30", dict(k=30), EUNSUPPORTED),
    ("nu = 30.5, coeffs NULL", dict(coeffs=None), EINVAL),
    ("nu = 30.5, metric id 2", dict(mid=2), EINVAL),
    # the widest list a coefficient entry writes is k = 1022 (k + 1 + R <= 1024); the prediction kernel's LDS carve is
    # sized for lists up to 1023 and the entry refuses what lies beyond, whatever R is
    ("k = 1024", dict(k=1024, nu=1.3), EUNSUPPORTED),
    ("k = 1024, R = 3", dict(k=1024, R=3, nu=1.3), EUNSUPPORTED),
    ("k = 1024, mean NULL", dict(k=1024, nu=1.3, mean=None), EINVAL),
    ("k = INT_MAX", dict(k=INT_MAX, nu=1.3), EUNSUPPORTED),
    ("empty batch, all pointers NULL", dict(b=0, **_nothing(MEAN_NAMES, MEAN_NUMBERS)), OK),
    ("empty batch, ids not looked at", dict(b=0, **_nothing(MEAN_NAMES, MEAN_NUMBERS), mid=7, lsc=9), OK),
    ("empty batch, nu beyond the limit", dict(b=0, nu=31.0), OK),
    ("empty batch, k < 1", dict(b=0, k=0), EINVAL),
    ("empty batch, nu = 0", dict(b=0, nu=0.0), EINVAL),
    ("empty batch, nu NaN", dict(b=0, nu=NAN), EINVAL),
]


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("name, changes, want", COEF_ROWS, ids=[r[0] for r in COEF_ROWS])
def test_status_of_the_coefficient_entry(name, changes, want, suf):
    assert coef_status(suf, **changes) == want


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("name, changes, want", MEAN_ROWS, ids=[r[0] for r in MEAN_ROWS])
def test_status_of_the_prediction_entry(name, changes, want, suf):
    assert mean_status(suf, **changes) == want


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("R", [1, 3, 16])
def test_workspace_is_asked_for_exactly_beyond_the_general_nu_lds_limit(suf, R):
    lib, es = _lib.load(), ES[suf]
    ws_bytes = lib.mgp_fast_coefficients_gen_workspace_bytes
    fits = lib.mgp_max_nn_count_gen(es, R)
    assert 64 < fits <= lib.mgp_max_nn_count(es, R)  # (the node table takes its share)
    for k in (1, 62, 63, 64, fits):
        assert ws_bytes(es, k, R, 1000) == 0, k
        assert coef_status(suf, k=k, R=R, ws=None, wsb=0) == EUNSUPPORTED, k
        assert coef_status(suf, k=k, R=R, ws=PTR + 4, wsb=1) == EUNSUPPORTED, k  # (not looked at)
    for k in (fits + 1, 300, 1023 - R):
        for b in (1, 37, 10**6):
            assert ws_bytes(es, k, R, b) == lib.mgp_large_workspace_bytes(es, k, R, b) > 0, (k, b)
        slab = ws_bytes(es, k, R, 1)
        assert coef_status(suf, k=k, R=R, ws=None, wsb=0) == EINVAL, k
        assert coef_status(suf, k=k, R=R, wsb=slab - 1) == EINVAL, k
        assert coef_status(suf, k=k, R=R, wsb=slab) == EUNSUPPORTED, k
    assert ws_bytes(es, 1024 - R, R, 8) == 0 and ws_bytes(es, 5000, R, 8) == 0
    assert ws_bytes(es, 0, R, 8) == 0 and ws_bytes(es, 300, 0, 8) == 0 and ws_bytes(es, 300, R, -1) == 0
    assert ws_bytes(2, 300, R, 8) == 0


def test_the_closed_form_entries_still_refuse_the_general_nu_id():
    lib = _lib.load()
    gen = _lib.KERNEL_IDS["matern_gen"]
    for suf in ("f32", "f64"):
        fast = getattr(lib, f"mgp_fast_posterior_mean_{suf}")
        anyk = getattr(lib, f"mgp_fast_coefficients_any_{suf}")
        for k in (30, 64, 300):
            assert fast(PTR, PTR, 4, None, PTR, 3, k, PTR, PTR, 1, gen, 0, PTR, 1, PTR, None) == EINVAL
            assert anyk(PTR, 4, PTR, 3, k, PTR, 1, 0, 1e-3, None, gen, 0, PTR, 1, PTR, None, PTR, 1 << 40, None) == EUNSUPPORTED


# ---- the case lists ---------------------------------------------------------------------------------------------------------
def test_prediction_cases_cover_every_factor():
    cases = [c for c in G.prediction_cases() if c["k"] in G.PRED_K and not c["zero"] and c["nu"] != 30.0]
    assert {(c["k"], c["d"]) for c in cases} == {(k, d) for k in G.PRED_K for d in G.PRED_D} and len(cases) == 40
    for key, values in (("dtype", ("float32", "float64")), ("nu", G.NUS), ("aniso", (False, True)), ("R", (1, 3)),
                        ("batch_idx", (False, True))):
        for v in values:
            mine = [c for c in cases if c[key] == v]
            assert len({c["d"] for c in mine}) == len(G.PRED_D), (key, v)
            assert len({c["k"] for c in mine}) >= 4, (key, v)
    extra = [c for c in G.prediction_cases() if c not in cases]
    assert sum(c["zero"] for c in extra) >= 1 and sum(c["nu"] == 30.0 for c in extra) == 1


def test_coefficient_cases_cover_the_edges_and_keep_the_rules():
    cases = G.coefficient_cases()
    grid = [c for c in cases if c["b"] == 24]
    assert {(c["k"], c["d"]) for c in grid} == {(k, d) for k in G.COEF_K for d in G.COEF_D}
    for c in cases:
        k = G.resolve_k(c, lds_limit)
        assert k + 1 + c["R"] <= 1024
        if c["dtype"] == "float32":
            assert not (c["nu"] == 8.0 and c["d"] <= 3), c  # in fp32, nu = 8 stays out of d <= 3
            assert not (c["d"] == 1 and k >= 31), c          # d = 1 with k >= 31 runs in fp64 only
    assert sum(c["aniso"] for c in cases) == 1 and sum(c["noise"] == "rows" for c in cases) == 1
    assert [c for c in cases if c["k"] == 1020 and c["R"] == 3 and c["dtype"] == "float64" and c["d"] == 3 and c["b"] == 3]
    for key, values in (("dtype", ("float32", "float64")), ("R", (1, 3))):
        for v in values:
            mine = [c for c in grid if c[key] == v]
            assert len({c["d"] for c in mine}) >= 3 and len({str(c["k"]) for c in mine}) >= 4, (key, v)
    assert {c["nu"] for c in grid} == set(G.NUS)


def tz32(r, nu):
    return _matern_gen_trapezoid_fp32(r, nu)[0].astype(np.float64)


def _share_of_band(got, ref, rtol):
    return float((np.abs(got - ref) / (rtol * np.abs(ref) + rtol * np.sqrt((ref ** 2).mean()))).max())


def test_the_fp32_evaluator_moves_no_fp32_case_by_more_than_a_quarter_of_the_band():
    """A condition on the case lists (not a measurement of the kernels): with scipy's kv replaced by the fp32
    evaluator restated in numpy and everything else in fp64, every fp32 case of the two GPU lists stays within a
    quarter of the band asserted there."""
    worst = {}
    for c in G.prediction_cases():
        if c["dtype"] != "float32":
            continue
        problem = G.prediction_problem(c)
        share = _share_of_band(G.prediction_reference(c, problem, fn=tz32), G.prediction_reference(c, problem), G.BAND["float32"])
        worst["prediction"] = max(worst.get("prediction", 0.0), share)
        assert share <= 0.25, (c, share)
    for c in G.coefficient_cases():
        if c["dtype"] != "float32":
            continue
        k = G.resolve_k(c, lds_limit)
        problem = G.coefficient_problem(c, k)
        share = _share_of_band(G.coefficient_reference(c, problem, fn=tz32), G.coefficient_reference(c, problem), G.BAND["float32"])
        worst["coefficients"] = max(worst.get("coefficients", 0.0), share)
        assert share <= 0.25, (c, k, share)
    print(worst)


# ---- the half-wave node bound (csrc/mgp_gen_group.h: matern_gen_eval_group) ---------------------------------------------------
def _trapezoid_fp32_grouped(r, nu, group=32):
    """matern_gen_eval_group in numpy float32: _matern_gen_trapezoid_fp32's table, constants and term arithmetic, but
    every group of ``group`` consecutive values sums to the node count of ITS OWN largest span -- the terms a longer
    neighbouring group would have run are masked."""
    f = np.float32
    h = f(_gen_step(nu))
    t = np.arange(128, dtype=f) * h
    a = f(nu) * t
    negc = (-np.cosh(t) * f(1.44269504088896)).astype(f)
    l = ((a + np.log1p(np.exp(f(-2.0) * a)) - f(0.693147180559945)) * f(1.44269504088896)).astype(f)
    l[0] -= f(1.0)
    lc = f((np.log(float(h)) + (1.0 - nu) * np.log(2.0) - math.lgamma(nu)) / np.log(2.0))
    r = np.asarray(r, dtype=f)
    assert r.size % group == 0
    x = np.minimum(np.maximum(r * np.sqrt(f(2.0) * f(nu)), f(1e-6)), f(3.0e4)).astype(f)
    lx = np.log2(x).astype(f)
    inner = f(22.0) + f(nu) * np.maximum(f(1.0), (f(5.4594316) - lx) * f(0.693147181))
    T = np.maximum(f(1.0), (np.log2(f(2.0) * inner).astype(f) - lx) * f(0.693147181))
    N = np.minimum((T / h).astype(np.int64) + 3, 128)
    N = np.repeat(N.reshape(-1, group).max(axis=1), group)
    L = (f(nu) * lx + lc).astype(f)
    acc = np.zeros_like(x)
    for i in range(int(N.max())):
        e = np.exp2((x * negc[i] + (L + l[i])).astype(f)).astype(f)
        acc = acc + np.where(i < N, e, f(0.0))
    return np.where(r > 0, acc, f(1.0)), N


@pytest.mark.parametrize("nu", [0.42, 1.0, 1.5, 2.2, 3.7, 8.0, 25.0])
def test_the_half_wave_node_bound_is_harmless(nu):
    """Groups of 32 scaled distances of very different reach side by side (one group near 1e-4, its neighbour of order
    1): summed to the group's own node count every value stays within the evaluator's documented error of scipy --
    <= 5e-6 for nu <= 4, <= 4e-5 up to 25 -- and the short group really stops earlier than the long one."""
    from scipy.special import kv

    rng = np.random.default_rng(3)
    groups = [10.0 ** rng.uniform(-5, -3, 32), rng.uniform(0.3, 3.0, 32), 10.0 ** rng.uniform(-2, 0, 32), rng.uniform(2.0, 60.0 / np.sqrt(2 * nu), 32),
              np.concatenate([[1e-5], rng.uniform(1.0, 5.0, 31)])]
    r = np.concatenate(groups)
    got, N = _trapezoid_fp32_grouped(r, nu)
    x = np.sqrt(2 * nu) * r
    ref = np.exp((1 - nu) * np.log(2.0) - math.lgamma(nu) + nu * np.log(x)) * kv(nu, x)
    ref = np.where(np.isfinite(ref), ref, 0.0)
    err = np.abs(got.astype(np.float64) - ref)
    assert err.max() <= (5e-6 if nu <= 4 else 4e-5), (nu, err.max(), r[err.argmax()])
    assert N[32] < N[0] and N[96] < N[0]
    # every group alone gives the bits it gives next to the others: that is what the mask is for
    for g, rr in enumerate(groups):
        alone, _ = _trapezoid_fp32_grouped(rr, nu)
        assert np.array_equal(alone, got[32 * g:32 * g + 32])
    # ... and the wave-wide count (every value to the longest tail) differs from it by less than the documented error too
    wide, _ = _matern_gen_trapezoid_fp32(r, nu)
    assert np.abs(wide.astype(np.float64) - got.astype(np.float64)).max() <= (5e-6 if nu <= 4 else 4e-5)
    assert float(_trapezoid_fp32_grouped(np.zeros(32), nu)[0][0]) == 1.0


# ---- the compiler's records -------------------------------------------------------------------------------------------------
def _resources():
    with open(os.path.join(os.path.dirname(_lib.LIB_PATH), "kernel_resources.json")) as f:
        return json.load(f)


def test_new_instantiations_no_spills_no_scratch():
    res = _resources()
    mine = {n: r for n, r in res.items() if any(s in n for s in ("fused_generic_gen_coeffs_kernel", "fused_large_gen_coeffs_kernel",
                                                                 "fast_mean_gen_kernel", "fast_mean_wide_gen_kernel"))}
    assert len(mine) == 10, sorted(mine)  # two coefficient families and three prediction kernels, two float widths
    for name, r in mine.items():
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (name, r)


def test_kernels_that_existed_before_keep_their_records():
    """The closed-form coefficient and prediction kernels, and every other kernel of the three files the new
    instantiations live in, against the records of the parent commit's build."""
    with open(os.path.join(ROOT, "tests", "golden", "parent_bits", "fast_gen_kernel_resources.json")) as f:
        then = json.load(f)
    now = _resources()
    for family in ("fast_mean_kernel", "fast_mean_wide_kernel", "fused_generic_coeffs_kernel", "fused_large_coeffs_kernel"):
        assert len([n for n in then if family in n]) >= 2, family
    assert len(then) == 22
    for name, r in then.items():
        assert now.get(name) == r, (name, r, now.get(name))
