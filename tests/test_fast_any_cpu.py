"""CPU: the fast-posterior-mean workflow beyond a wavefront, without a device.

* the status grid of ``mgp_fast_coefficients_any_*`` and of ``mgp_fast_coefficients_workspace_bytes`` (include/muygpys_hip.h),
  in the style of test_large_status_cpu.py: one rule violated per row, every status decided BEFORE any HIP call, host
  buffers standing in for device pointers.  No row here reaches a launch: where a call would, the general-nu kernel id
  (refused last, MGP_EUNSUPPORTED) stands in for "every other check passed";
* what ``fused.fast_coefficients`` hands the library, in the style of test_fused_calls_cpu.py;
* ``muygpys_amd.examples.fast_posterior_mean`` on host arrays through injected backend callables against the oracle.
"""

import ctypes as C

import numpy as np
import pytest
import torch

from muygpys_amd import _lib, fused
from muygpys_amd.fused import KernelSpec
from oracle import muygps_oracle as orc
from tests.call_recorder import STREAM, install, vals

OK, EINVAL, EUNSUPPORTED = 0, -1, -2
ES = {"f32": 4, "f64": 8}
INT_MAX, INT64_MAX = 2**31 - 1, 2**63 - 1
GEN = 5  # MGP_KERNEL_MATERN_GEN

NAMES = "fn d ni b k tg R nm eps nd kid mid ls lsc coeffs info ws wsb st".split()
NUMBERS = dict(d=4, b=3, k=300, R=1, nm=0, eps=1e-3, kid=GEN, mid=0, lsc=1, wsb=1 << 40)
OPTIONAL = ("nd", "st", "info")
BUF = (C.c_double * 64)()
PTR = C.addressof(BUF)
assert PTR % 16 == 0


def status(suf, **changes):
    """Status of a call that violates what ``changes`` says, starting from arguments every check but the last accepts
    (k = 300: beyond LDS for either width, a workspace of 1 TiB; the general-nu id: MGP_EUNSUPPORTED instead of a launch)."""
    args = {n: NUMBERS[n] if n in NUMBERS else (None if n in OPTIONAL else PTR) for n in NAMES}
    assert not set(changes) - set(NAMES)
    args.update(changes)
    return getattr(_lib.load(), f"mgp_fast_coefficients_any_{suf}")(*[args[n] for n in NAMES])


def ws_bytes(es, k, R, b):
    return _lib.load().mgp_fast_coefficients_workspace_bytes(es, k, R, b)


ROWS = [("b < 0", dict(b=-1), EINVAL), ("k < 1", dict(k=0), EINVAL), ("d < 1", dict(d=0), EINVAL), ("R < 1", dict(R=0), EINVAL)]
ROWS += [(f"{p} NULL", {p: None}, EINVAL) for p in "fn tg ni ls coeffs".split()]
ROWS += [(f"kernel id {i}", dict(kid=i), EINVAL) for i in (-1, 6, 99)]
ROWS += [(f"metric id {i}", dict(mid=i), EINVAL) for i in (-1, 2)]
ROWS += [(f"noise mode {i}", dict(nm=i), EINVAL) for i in (-1, 3)]
ROWS += [(f"noise mode {i} without noise_dev", dict(nm=i, nd=None), EINVAL) for i in (1, 2)]
ROWS += [(f"ls_count {i} at d = 4", dict(lsc=i), EINVAL) for i in (0, 2, 5)]
ROWS += [
    ("the general-nu id", dict(), EUNSUPPORTED),
    ("the general-nu id, info NULL", dict(info=None), EUNSUPPORTED),
    ("the general-nu id, workspace NULL beyond LDS", dict(ws=None), EINVAL),
    ("workspace misaligned", dict(ws=PTR + 8), EINVAL),
    ("k + 1 + R = 1024, the general-nu id", dict(k=1022), EUNSUPPORTED),
    ("k + 1 + R = 1024 by responses", dict(k=1007, R=16), EUNSUPPORTED),
    ("k + 1 + R = 1025", dict(k=1023, kid=2), EUNSUPPORTED),
    ("k + 1 + R = 1025 by responses", dict(k=1008, R=16, kid=2), EUNSUPPORTED),
    ("k + 1 + R = 1025, coeffs NULL", dict(k=1023, kid=2, coeffs=None), EINVAL),
    ("k + 1 + R = 1025, workspace NULL", dict(k=1023, kid=2, ws=None), EINVAL),
    ("k + 1 + R = 1025, workspace misaligned", dict(k=1023, kid=2, ws=PTR + 4), EINVAL),
    ("k = INT_MAX", dict(k=INT_MAX, kid=2, wsb=INT64_MAX), EUNSUPPORTED),
    ("k = R = INT_MAX", dict(k=INT_MAX, R=INT_MAX, kid=2, wsb=INT64_MAX), EUNSUPPORTED),
    ("k = INT_MAX, a workspace of 1 TiB", dict(k=INT_MAX, kid=2), EINVAL),
    ("empty batch, all pointers NULL", dict(b=0, wsb=0, **{n: None for n in NAMES if n not in NUMBERS}), OK),
    ("empty batch, ids not looked at", dict(b=0, wsb=0, **{n: None for n in NAMES if n not in NUMBERS}, kid=99, mid=7, nm=8, lsc=9), OK),
    ("empty batch, k < 1", dict(b=0, k=0), EINVAL),
]


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("name, changes, want", ROWS, ids=[r[0] for r in ROWS])
def test_status_of_refused_and_empty_calls(name, changes, want, suf):
    assert status(suf, **changes) == want


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("R", [1, 3, 16])
def test_workspace_is_asked_for_exactly_beyond_lds(suf, R):
    """The query returns 0 up to mgp_max_nn_count (NULL accepted there: the call gets as far as the refusal of the
    general-nu id) and the size of mgp_large_workspace_bytes beyond (NULL, or one byte short of a slab: MGP_EINVAL)."""
    lib, es = _lib.load(), ES[suf]
    fits = lib.mgp_max_nn_count(es, R)
    assert 64 < fits < 300
    for k in (1, 62, 63, 64, fits):
        assert ws_bytes(es, k, R, 1000) == 0, k
        assert status(suf, k=k, R=R, ws=None, wsb=0) == EUNSUPPORTED, k
        assert status(suf, k=k, R=R, ws=PTR + 4, wsb=1) == EUNSUPPORTED, k  # (not looked at)
    for k in (fits + 1, 300, 1023 - R):
        for b in (1, 37, 10**6):
            assert ws_bytes(es, k, R, b) == lib.mgp_large_workspace_bytes(es, k, R, b) > 0, (k, b)
        slab = ws_bytes(es, k, R, 1)
        assert ws_bytes(es, k, R, 0) == slab
        assert status(suf, k=k, R=R, ws=None, wsb=0) == EINVAL, k
        assert status(suf, k=k, R=R, wsb=slab - 1) == EINVAL, k
        assert status(suf, k=k, R=R, wsb=slab) == EUNSUPPORTED, k
    assert ws_bytes(es, 1024 - R, R, 8) == 0 and ws_bytes(es, 5000, R, 8) == 0
    assert ws_bytes(es, 0, R, 8) == 0 and ws_bytes(es, 300, 0, 8) == 0 and ws_bytes(es, 300, R, -1) == 0
    assert ws_bytes(2, 300, R, 8) == 0


def test_the_wave_entry_keeps_its_limits_and_the_prediction_entry_its_refusal():
    """mgp_fast_coefficients_* is untouched (its own checks), and the general-nu id is not a kernel id of
    mgp_fast_posterior_mean_* (MGP_EINVAL, as before), whatever k is."""
    lib = _lib.load()
    for suf in ("f32", "f64"):
        fast = getattr(lib, f"mgp_fast_posterior_mean_{suf}")
        for k in (30, 64, 300):
            assert fast(PTR, PTR, 4, None, PTR, 3, k, PTR, PTR, 1, GEN, 0, PTR, 1, PTR, None) == EINVAL
            assert fast(PTR, PTR, 4, None, PTR, 0, k, None, None, 1, 2, 0, None, 1, None, None) == OK
            assert fast(PTR, PTR, 4, None, PTR, 3, k, None, PTR, 1, 2, 0, PTR, 1, PTR, None) == EINVAL


# ---- what fused.fast_coefficients hands the library -------------------------------------------------------------------

D, N = 3, 40


@pytest.fixture
def rec(monkeypatch):
    yield install(monkeypatch)
    fused.clear_caches()


def inputs(k, R, dtype=torch.float32, n=N):
    g = torch.Generator().manual_seed(k + R)
    X = torch.randn(n, D, generator=g).to(dtype)
    Y = (torch.randn(n, generator=g) if R == 0 else torch.randn(n, R, generator=g)).to(dtype)
    nn = torch.randint(0, n, (n, k), generator=g)
    return X, Y, nn


SPEC = KernelSpec("matern15", "l2", (2.0, 3.0, 4.0), 1e-3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("k, R, workspace", [(63, 0, False), (5, 2, False), (64, 3, False), (300, 0, True), (300, 3, True)])
def test_one_call_of_the_new_entry(rec, k, R, workspace, dtype):
    # fn, d, ni, b, k, tg, R, noise_mode, eps, nd, kernel, metric, ls, ls_count, coeffs, info, workspace, workspace_bytes, stream
    X, Y, nn = inputs(k, R, dtype)
    out, nn_fast = fused.fast_coefficients(SPEC, X, Y, nn)
    assert out.shape == ((N, k) if R == 0 else (N, k, R)) and out.dtype == dtype
    (call,) = rec.calls
    v = vals(call)
    assert call[0] == "fast_coefficients_any" and call[1] == dtype and len(v) == 19
    assert v[0:11] == [X.data_ptr(), D, nn_fast.data_ptr(), N, k, Y.data_ptr(), max(R, 1), 0, 1e-3, None, 2]
    assert v[11] == 0 and v[12] is not None and v[13] == 3 and v[14] == out.data_ptr() and v[15] is not None
    want = _lib.load().mgp_fast_coefficients_workspace_bytes(4 if dtype == torch.float32 else 8, k, max(R, 1), N)
    assert (want > 0) == workspace
    assert (v[16] is not None) == workspace and v[17] == want and v[18] == STREAM
    if workspace:
        assert v[16] % 16 == 0


def test_the_wave_entry_comes_first_where_it_serves(rec):
    X, Y, nn = inputs(62, 0)
    out, _ = fused.fast_coefficients(SPEC, X, Y, nn)
    assert [c[0] for c in rec.calls] == ["fast_coefficients"] and out.shape == (N, 62)
    assert vals(rec.calls[0])[13] == out.data_ptr()
    # ... and the new entry behind its refusal
    rec.calls.clear()
    rec.statuses["fast_coefficients"] = [-2]
    out, _ = fused.fast_coefficients(SPEC, X, Y, nn)
    assert [c[0] for c in rec.calls] == ["fast_coefficients", "fast_coefficients_any"]
    assert vals(rec.calls[1])[14] == out.data_ptr()


def test_materialising_route_on_request_and_behind_a_refusal(rec, monkeypatch):
    from muygpys_amd._src.gp.muygps import hip as M

    solved = []

    def fake_solve(Kin, Kcross, Y, kout=1.0, want=("mean",)):
        solved.append((tuple(Kin.shape), tuple(Y.shape), want))
        return None, None, None, torch.zeros(Y.shape, dtype=Y.dtype)

    monkeypatch.setattr(M, "_solve", fake_solve)
    X, Y, nn = inputs(70, 2)
    out, _ = fused.fast_coefficients(SPEC, X, Y, nn, fused=False, chunk=16)
    assert out.shape == (N, 70, 2)
    assert "fast_coefficients_any" not in [c[0] for c in rec.calls]
    assert [s[0] for s in solved] == [(16, 70, 70), (16, 70, 70), (8, 70, 70)] and solved[0][2] == ("coeffs",)
    rec.calls.clear()
    solved.clear()
    rec.statuses["fast_coefficients_any"] = [-2]  # MGP_EUNSUPPORTED (the general nu): fall back, do not raise
    out, _ = fused.fast_coefficients(SPEC, X, Y, nn)
    assert rec.calls[0][0] == "fast_coefficients_any" and len(solved) == 1 and out.shape == (N, 70, 2)
    rec.calls.clear()
    rec.statuses["fast_coefficients_any"] = [-1]
    with pytest.raises(_lib.HipLibraryError):
        fused.fast_coefficients(SPEC, X, Y, nn)


def test_no_fused_call_for_the_general_nu_or_beyond_1024_rows(rec, monkeypatch):
    """The general-smoothness Matern (not a kernel id of the wave entry: it would answer MGP_EINVAL) and systems of more
    than 1024 rows (the query function returns 0 there and the entry would refuse the NULL workspace) never reach a
    fused coefficient entry: the chunked route serves them, the general nu through mgp_matern_gen_*."""
    from muygpys_amd._src.gp.muygps import hip as M

    solved = []
    monkeypatch.setattr(M, "_solve", lambda Kin, Kc, Y, kout=1.0, want=("mean",): (
        solved.append(tuple(Kin.shape)), (None, None, None, torch.zeros(Y.shape, dtype=Y.dtype)))[1])
    gen = KernelSpec("matern_gen", "l2", 2.0, 1e-3, smoothness=0.8)
    for k, R in ((30, 0), (62, 0), (70, 0), (70, 2)):
        rec.calls.clear()
        X, Y, nn = inputs(k, R)
        out, _ = fused.fast_coefficients(gen, X, Y, nn)
        names = [c[0] for c in rec.calls]
        assert "matern_gen" in names and "kernel_apply" not in names, names
        assert not {"fast_coefficients", "fast_coefficients_any"} & set(names), names
        assert out.shape == ((N, k) if R == 0 else (N, k, R))
    for k, R in ((1023, 0), (1021, 3)):
        rec.calls.clear()
        solved.clear()
        X, Y, nn = inputs(k, R)
        fused.fast_coefficients(SPEC, X, Y, nn)
        assert not {"fast_coefficients", "fast_coefficients_any"} & {c[0] for c in rec.calls}
        assert solved == [(N, k, k)]
    rec.calls.clear()
    X, Y, nn = inputs(1020, 3)  # 1024 rows: served
    fused.fast_coefficients(SPEC, X, Y, nn)
    assert [c[0] for c in rec.calls] == ["fast_coefficients_any"]


# ---- the example workflow on host arrays ------------------------------------------------------------------------------

class HostNeighbours:
    """Brute-force stand-in for NN_Wrapper over host arrays."""

    def __init__(self, X, k):
        self.X, self.k = X, k

    def _nn(self, Q, k):
        d2 = ((Q[:, None, :] - self.X[None, :, :]) ** 2).sum(-1)
        idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
        return idx, np.take_along_axis(d2, idx, 1)

    def get_nns(self, Q):
        return self._nn(Q, self.k)

    def get_batch_nns(self, batch):
        idx, d2 = self._nn(self.X[batch], self.k + 1)
        return idx[:, 1:], d2[:, 1:]


def host_model(kernel, metric_name, ls, noise):
    from tests.test_functor_layer_cpu import numpy_model

    return numpy_model(dict(kernel=kernel, metric=metric_name, length_scale=ls, noise=noise), {})


@pytest.mark.parametrize("R", [1, 3])
def test_example_workflow_through_injected_backends(R):
    from muygpys_amd.examples import fast_posterior_mean as ex

    rng = np.random.default_rng(5)
    n, d, k, nq = 90, 4, 70, 11
    X, Q = rng.uniform(size=(n, d)), rng.uniform(size=(nq, d))
    Y = np.sin(3 * X @ rng.normal(size=(d, R))) + 0.05 * rng.normal(size=(n, R))
    y = Y[:, 0] if R == 1 else Y
    m = host_model("matern15", "l2", 1.3, 1e-2)
    nbrs = HostNeighbours(X, k)
    spec = orc.Spec("matern15", "l2", 1.3, 1e-2)
    nn = nbrs.get_batch_nns(np.arange(n))[0]
    nn_fast = orc.fast_nn_update(nn)
    pd = orc.pairwise_tensor(X, nn_fast)
    _, Kin = orc.kernel_tensors(spec, pd[:, 0], pd)
    coeffs_ref = orc.fast_posterior_mean_precompute(orc.perturb(spec, Kin, nn_fast), y[nn_fast])
    closest = nbrs.get_nns(Q)[0][:, 0]
    Kc, _ = orc.kernel_tensors(spec, orc.crosswise_tensor(Q, X, np.arange(nq), nn_fast[closest]), pd[:1])
    mean_ref = orc.fast_posterior_mean(Kc, coeffs_ref[closest])

    coeffs, idx = ex.make_fast_regressor(m, nbrs, X, y)
    assert np.array_equal(idx, nn_fast)  # (fast_nn_update applied once)
    np.testing.assert_allclose(coeffs, coeffs_ref, rtol=1e-9, atol=1e-11)
    mean, coeffs2, timing = ex.fast_posterior_mean_any(m, Q, X, nbrs, y)
    assert sorted(timing) == ["agree", "nn", "precompute", "pred"]
    np.testing.assert_allclose(coeffs2, coeffs_ref, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(mean, mean_ref, rtol=1e-9, atol=1e-11)
    if R == 3:
        # one model per response column: the same numbers when the models agree
        class Multi:
            models = [m, m, m]

        cm, idx_m = ex.make_fast_multivariate_regressor(Multi(), nbrs, X, Y)
        assert cm.shape == (n, k, 3) and np.array_equal(idx_m, nn_fast)
        np.testing.assert_allclose(cm, coeffs_ref, rtol=1e-9, atol=1e-11)
        mean_m, _, _ = ex.fast_posterior_mean_any(Multi(), Q, X, nbrs, Y)
        np.testing.assert_allclose(mean_m, mean_ref, rtol=1e-9, atol=1e-11)


# ---- the seeds of the GPU tests: fp32 numpy itself stays inside the band ------------------------------------------------

def test_fp32_numpy_solve_stays_inside_the_band():
    """``np.linalg.solve`` in fp32 on the coefficient cases of tests/test_gpu_fast_any.py (same builders, same seeds)
    against the fp64 solve, within tests.util.RTOL['float32']: the band is one fp32 arithmetic can hold on these
    systems, so a kernel that misses it is wrong rather than unlucky."""
    from tests import test_gpu_fast_any as G
    from tests.util import RTOL, assert_close

    lib = _lib.load()
    seen = set()
    for c in G.coefficient_cases():
        k = c["k"] if isinstance(c["k"], int) else lib.mgp_max_nn_count(4 if c["dtype"] == "float32" else 8, c["R"]) + (c["k"] == "kmax+1")
        key = (k, c["R"], c["noise_mode"], c["aniso"])
        if key in seen:
            continue
        seen.add(key)
        _, _, _, _, _, Kin, Yn = G.coefficient_problem(k, c["R"], c["noise_mode"], c["aniso"], seed=k + c["R"])
        ref = np.linalg.solve(Kin, Yn)
        got = np.linalg.solve(Kin.astype(np.float32), Yn.astype(np.float32))
        assert_close(got, ref, RTOL["float32"], f"fp32 numpy, {key}")
    for R in (1, 3):
        _, _, _, _, _, Kin, Yn = G.coefficient_problem(1023 - R, R, "scalar", False, seed=1023 - R, b=3)
        assert_close(np.linalg.solve(Kin.astype(np.float32), Yn.astype(np.float32)), np.linalg.solve(Kin, Yn), RTOL["float32"],
                     f"fp32 numpy, k = {1023 - R}")


def test_coefficient_kernels_no_spills_no_scratch():
    """The compiler's register record of the four coefficient instantiations (LDS / slab, two float widths)."""
    import json
    import os

    with open(os.path.join(os.path.dirname(_lib.LIB_PATH), "kernel_resources.json")) as f:
        res = json.load(f)
    mine = {n: r for n, r in res.items() if "fused_generic_coeffs_kernel" in n or "fused_large_coeffs_kernel" in n}
    assert len(mine) == 4, sorted(mine)
    for name, r in mine.items():
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (name, r)
