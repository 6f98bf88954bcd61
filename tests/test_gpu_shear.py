"""The shear model on the GPU: tensor kernels, nuggets, the materialised multi-output solve and the fused one-launch
posterior (mgp_shear_posterior_*) against the reference's fixtures and the numpy oracle (BASELINE.md sec. 3 metric:
1e-5 fp64, 1e-3 fp32; fp32 only where eps >= 1e-3)."""

import json
import os

import numpy as np
import pytest
import torch

from tests import shear_oracle as O

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "shear")
DEV = "cuda"


def _load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def _close(got, ref, rtol, what):
    got = got.double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    atol = rtol * np.sqrt(np.mean(ref**2))
    err = np.abs(got - ref)
    assert np.all(err <= rtol * np.abs(ref) + atol), (what, float(err.max()))


def _dtypes(eps):
    return [(torch.float64, 1e-5)] + ([(torch.float32, 1e-3)] if eps >= 1e-3 else [])


def _t(x, dt):
    return torch.as_tensor(np.asarray(x), device=DEV, dtype=dt)


def _model(kind, ell, eps):
    from muygpys_amd.gp.muygps import MuyGPS
    from muygpys_amd.gp.deformation import F2, DifferenceIsotropy
    from muygpys_amd.gp.hyperparameter import FixedScale, ScalarParam
    from muygpys_amd.gp.kernels import ShearKernel, ShearKernel2in3out
    from muygpys_amd.gp.noise import HomoscedasticNoise, ShearNoise33

    dfm = DifferenceIsotropy(F2, length_scale=ScalarParam(ell))
    if kind == "33":
        return MuyGPS(kernel=ShearKernel(deformation=dfm), noise=ShearNoise33(eps), scale=FixedScale())
    return MuyGPS(kernel=ShearKernel2in3out(deformation=dfm), noise=HomoscedasticNoise(eps), scale=FixedScale())


@pytest.mark.parametrize("name", ["shear_33_k10", "shear_23_k10"])
def test_a_b_c_tensor_kernels_perturb_and_materialised_posterior(name):
    from muygpys_amd._src.gp.kernels.shear import hip as K
    from muygpys_amd._src.gp.muygps import hip as M
    from muygpys_amd._src.gp.noise import hip as N

    g = _load(name)
    meta = json.loads(str(g["meta"]))
    ell, eps, kind = meta["length_scale"], meta["noise"], meta["kind"]
    P = g["Kin_perturbed"]
    print("condition number", np.linalg.cond(P.reshape(P.shape[0], P.shape[1] * P.shape[2], -1)).max())
    for dt, rtol in _dtypes(eps):
        pair, cross = _t(g["pairwise"], dt), _t(g["crosswise"], dt)[..., None, :]
        if kind == "33":
            Kin, Kc = K._shear_33_fn(pair, length_scale=ell), K._shear_33_fn(cross, length_scale=ell)
            Kp = N._shear_perturb33(Kin, eps)
        else:
            Kin, Kc = K._shear_Kin23_fn(pair, length_scale=ell), K._shear_Kcross23_fn(cross, length_scale=ell)
            Kp = N._homoscedastic_perturb(Kin, eps)
        _close(Kin, g["Kin"], rtol, "Kin")
        _close(Kc, g["Kcross"], rtol, "Kcross")
        _close(Kp, P, rtol, "perturbed Kin")
        mean = M._muygps_posterior_mean(Kp, Kc, _t(g["batch_nn_targets"], dt))
        var = M._muygps_diagonal_variance(Kp, Kc, _t(g["Kout"], dt))
        _close(mean, g["mean"], 10 * rtol, "materialised mean")
        _close(var, g["variance"], 10 * rtol, "materialised covariance")


def test_a_squeezed_b1_shapes():
    from muygpys_amd._src.gp.kernels.shear import hip as K

    g = _load("shear_b1")
    ell = float(g["length_scale"])
    for dt, rtol in _dtypes(1.0):
        pair, cross = _t(g["pairwise"], dt), _t(g["crosswise"], dt)[..., None, :]
        _close(K._shear_33_fn(pair, length_scale=ell), g["Kin33"], rtol, "Kin33 b=1")
        _close(K._shear_33_fn(cross, length_scale=ell), g["Kcross33"], rtol, "Kcross33 b=1")
        _close(K._shear_Kin23_fn(pair, length_scale=ell), g["Kin23"], rtol, "Kin23 b=1")
        _close(K._shear_Kcross23_fn(cross, length_scale=ell), g["Kcross23"], rtol, "Kcross23 b=1")


def test_b_shear_noise_refuses_other_shapes():
    from muygpys_amd._src.gp.noise import hip as N

    x = torch.zeros((2, 4, 4), device=DEV, dtype=torch.float64)
    for err in (NotImplementedError, ValueError):
        with pytest.raises(err):
            N._shear_perturb33(x, 1e-3)
    with pytest.raises(ValueError):
        N._homoscedastic_perturb(x[0], 1e-3)


@pytest.mark.parametrize("name", ["shear_33_k10", "shear_23_k10", "shear_33_k50", "shear_23_k50"])
def test_d_fused_route_through_muygps(name, monkeypatch):
    from muygpys_amd import _lib, lazy, lazy_eval

    g = _load(name)
    meta = json.loads(str(g["meta"]))
    ell, eps, kind, b = meta["length_scale"], meta["noise"], meta["kind"], meta["b"]
    launches = []
    real = lazy_eval._shear_launch
    monkeypatch.setattr(lazy_eval, "_shear_launch", lambda *a: launches.append(1) or real(*a))
    for dt, rtol in _dtypes(eps):
        launches.clear()
        X, Y = _t(g["features"], dt), _t(g["targets"], dt)
        if kind == "23":
            Y = Y[:, 1:].contiguous()  # the table of the observed components (gamma1, gamma2)
        bi, ni = g["batch_indices"], torch.as_tensor(g["nn_indices"], device=DEV)
        m = _model(kind, ell, eps)
        cross, pair, nn_t = m.make_predict_tensors(torch.arange(b, device=DEV), ni, X[torch.as_tensor(bi, device=DEV)],
                                                   X, Y)
        nn_t = nn_t.swapaxes(-2, -1)
        assert isinstance(nn_t, lazy.LazyTargets)
        Kin, Kc = m.kernel(pair), m.kernel(cross)
        assert isinstance(Kin, lazy.LazyShearCov) and isinstance(Kc, lazy.LazyShearCov)
        mean = m.posterior_mean(Kin, Kc, nn_t)
        assert "shear_posterior_kernel" in _lib.last_kernel()
        var = m.posterior_variance(Kin, Kc)
        assert len(launches) == 1, "mean and variance of one evaluation share one launch"
        _close(mean, g["mean"], 10 * rtol, "fused mean")
        _close(var, g["variance"], 10 * rtol, "fused covariance")
        # ... the gathered (b, in, k) responses (what the reference's own gather hands over) take the same launch
        # with the responses read from the batch tensor, against the fixtures too
        tg = nn_t.materialize()
        assert tuple(tg.shape) == (b, Kin.in_count, Kin.diffs.nn_indices.shape[1])
        launches.clear()
        mean_g = m.posterior_mean(Kin, Kc, tg)
        var_g = m.posterior_variance(Kin, Kc)
        assert len(launches) == 1 and "shear_posterior_kernel" in _lib.last_kernel()
        _close(mean_g, g["mean"], 10 * rtol, "fused mean, gathered responses")
        _close(var_g, g["variance"], 10 * rtol, "fused covariance, gathered responses")
        # ... and the materialised route agrees
        Kp = m.noise.perturb(Kin).materialize()
        _close(m._backend_mean_fn(Kp, Kc.materialize(), tg), mean.double().cpu().numpy(), 10 * rtol,
               "materialised vs fused mean")
        # a trial length scale with the stored Kout (what the optimiser evaluates)
        trial = 1.3 * ell
        Kin2, Kc2 = m.kernel(pair, length_scale=trial), m.kernel(cross, length_scale=trial)
        var2 = m.posterior_variance(Kin2, Kc2)
        _, cov_ref, *_ = O.posterior(g["features"], g["targets"], bi, g["nn_indices"], trial, eps, kind,
                                     "shear33" if kind == "33" else "homoscedastic", Kout=O.kout(ell))
        _close(var2, cov_ref, 10 * rtol, "trial length scale, stored Kout")


def test_e_full_size_fp64_k50():

    torch.manual_seed(0)
    N, b, k, ell, eps = 50_000, 200_000, 50, 0.002, 1e-3
    X = torch.rand((N, 2), device=DEV, dtype=torch.float64)
    Y = torch.randn((N, 3), device=DEV, dtype=torch.float64)
    bi = torch.randint(0, N, (b,), device=DEV)
    ni = torch.randint(0, N, (b, k), device=DEV)
    m = _model("33", ell, eps)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    cross, pair, nn_t = m.make_predict_tensors(bi, ni, X, X, Y)
    nn_t = nn_t.swapaxes(-2, -1)
    Kin, Kc = m.kernel(pair), m.kernel(cross)
    mean = m.posterior_mean(Kin, Kc, nn_t)
    cov = m.posterior_variance(Kin, Kc)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    assert rise < 256 * 2**20, rise
    assert torch.isfinite(mean).all() and torch.isfinite(cov).all()
    c = cov.cpu().numpy()
    np.testing.assert_allclose(c, np.swapaxes(c, 1, 2), rtol=1e-8, atol=1e-8 * np.abs(c).max())
    scale = np.abs(np.diagonal(c, axis1=1, axis2=2)).max()
    assert np.linalg.eigvalsh(c).min() >= -1e-6 * scale
    # a 2 000-row sample against the materialised route
    s = torch.arange(0, b, b // 2000, device=DEV)[:2000]
    m2 = _model("33", ell, eps)
    cr, pr, _ = m2.make_predict_tensors(bi[s], ni[s], X, X, Y, materialize=True)
    Kin_s, Kc_s = m2.kernel(pr), m2.kernel(cr)
    mean_s = m2.posterior_mean(Kin_s, Kc_s, Y[ni[s]].swapaxes(-2, -1))
    cov_s = m2.posterior_variance(Kin_s, Kc_s)
    _close(mean[s], mean_s.double().cpu().numpy(), 1e-5, "sample mean")
    _close(cov[s], cov_s.double().cpu().numpy(), 1e-5, "sample covariance")
    # duplicate points with eps = 0: NaN outputs and LinAlgError
    ni_bad = ni[:4].clone()
    ni_bad[0] = ni_bad[0, 0]
    m0 = _model("33", ell, 0.0)
    cr, pr, nt = m0.make_predict_tensors(bi[:4], ni_bad, X, X, Y)
    Kin0, Kc0 = m0.kernel(pr), m0.kernel(cr)
    with pytest.raises(np.linalg.LinAlgError):
        m0.posterior_mean(Kin0, Kc0, nt.swapaxes(-2, -1))
    mean0, kk0, _, info0 = _raw_launch(Kin0, Kc0, Y)
    assert int(info0.item()) == 1
    assert torch.isnan(mean0[0]).all() and torch.isnan(kk0[0]).all() and torch.isfinite(mean0[1:]).all()


def _raw_launch(Kin, Kc, Y):
    """mgp_shear_posterior_f64 without the LinAlgError check: what the kernel leaves behind."""
    from muygpys_amd import _lib
    from muygpys_amd._src.gp.tensors import hip as T

    a, c = Kin.diffs, Kc.diffs
    b, k = a.nn_indices.shape
    out = [torch.empty(s, device=DEV, dtype=torch.float64) for s in ((b, 3), (b, 3, 3), (b,))]
    info = torch.zeros(1, device=DEV, dtype=torch.int32)
    rc = _lib.fn("shear_posterior", torch.float64)(
        _lib.ptr(c.data), _lib.ptr(a.nn_data), _lib.ptr(T._idx(c.data_indices)), _lib.ptr(T._idx(a.nn_indices)), b, k,
        3, _lib.ptr(Y), 3, 0, float(Kin.length_scale), _lib.SHEAR_NOISE_33, 0.0, *(_lib.ptr(t) for t in out),
        _lib.ptr(info), _lib.stream_ptr(),
    )
    _lib.check(rc, "mgp_shear_posterior")
    torch.cuda.synchronize()
    return out[0], out[1], out[2], info


def test_d_two_input_model_refuses_three_component_responses():
    """As the reference: (b, 3, k) responses against a 2-in Kin (b, 2, k, 2, k) do not flatten -- on the fused route
    (which then hands over to the materialised one) and on the materialised route alike."""
    from muygpys_amd._src.gp.muygps import hip as M

    g = _load("shear_23_k10")
    meta = json.loads(str(g["meta"]))
    X, Y = _t(g["features"], torch.float64), _t(g["targets"], torch.float64)
    m = _model("23", meta["length_scale"], meta["noise"])
    ni = torch.as_tensor(g["nn_indices"], device=DEV)
    cross, pair, nn_t = m.make_predict_tensors(torch.arange(meta["b"], device=DEV), ni,
                                               X[torch.as_tensor(g["batch_indices"], device=DEV)], X, Y)
    Kin, Kc = m.kernel(pair), m.kernel(cross)
    with pytest.raises(ValueError):
        m.posterior_mean(Kin, Kc, nn_t.swapaxes(-2, -1))
    with pytest.raises(ValueError):
        M._muygps_posterior_mean(m.noise.perturb(Kin).materialize(), Kc.materialize(),
                                 nn_t.swapaxes(-2, -1).materialize())


def test_d_unit_axis_of_the_reference_functors():
    """``crosswise[..., None, :]`` -- what the reference's ShearKernel.__call__ does to crosswise differences -- keeps
    the lazy handle (a unit axis), which the shear functions evaluate as Kcross; materialised it is the (b, k, 1, 2)
    tensor."""
    from muygpys_amd import lazy
    from muygpys_amd._src.gp.kernels.shear import hip as K

    g = _load("shear_33_k10")
    meta = json.loads(str(g["meta"]))
    X = _t(g["features"], torch.float64)
    m = _model("33", meta["length_scale"], meta["noise"])
    ni = torch.as_tensor(g["nn_indices"], device=DEV)
    cross, _, _ = m.make_predict_tensors(torch.arange(meta["b"], device=DEV), ni,
                                         X[torch.as_tensor(g["batch_indices"], device=DEV)], X, X)
    u = cross[..., None, :]
    assert isinstance(u, lazy.LazyDiffs) and u.unit_axis and tuple(u.shape) == (meta["b"], ni.shape[1], 1, 2)
    _close(u.materialize()[..., 0, :], g["crosswise"], 1e-12, "unit-axis differences")
    Kc = K._shear_33_fn(u, length_scale=meta["length_scale"])
    assert isinstance(Kc, lazy.LazyShearCov) and Kc.kind == "crosswise"
    _close(Kc.materialize(), g["Kcross"], 1e-5, "Kcross of the unit-axis handle")


def _grid_problem(kind):
    """The seeded 25 x 25 grid (l = 0.05, eps = 1e-4): a model started at l = 0.08 and its lazy training tensors
    (200 batch points, 50 nearest neighbours); the 2-in model observes (gamma1, gamma2) and is scored on them."""
    from muygpys_amd.gp.deformation import F2, DifferenceIsotropy
    from muygpys_amd.gp.hyperparameter import ScalarParam

    g = _load("shear_grid")
    ell, eps = float(g["length_scale"]), float(g["noise"])
    X, Y = g["features"], g["targets"]
    n, k = X.shape[0], 50
    rng = np.random.default_rng(5)
    batch = np.sort(rng.choice(n, size=200, replace=False))
    d2 = ((X[batch][:, None, :] - X[None, :, :]) ** 2).sum(-1)
    d2[np.arange(len(batch)), batch] = np.inf
    nn = np.argsort(d2, axis=1)[:, :k]
    Xd, Yd = _t(X, torch.float64), _t(Y, torch.float64)
    m = _model(kind, ell, eps)
    m = type(m)(kernel=type(m.kernel)(deformation=DifferenceIsotropy(F2, length_scale=ScalarParam(0.08, (0.01, 0.2)))),
                noise=m.noise, scale=m.scale)
    bt = torch.as_tensor(batch, device=DEV)
    cross, pair, bt_y, nn_t = m.make_train_tensors(bt, torch.as_tensor(nn, device=DEV), Xd, Yd)
    nn_t = nn_t.swapaxes(-2, -1)
    kw = {}
    if kind == "23":
        nn_t = nn_t[:, 1:, :]
        kw["target_mask"] = (1, 2)
        bt_y = bt_y[:, 1:]
    return m, ell, (bt_y, nn_t, cross, pair), kw


@pytest.mark.parametrize("kind", ["33", "23"])
@pytest.mark.parametrize("driver", ["L_BFGS_B", "Bayes"])
def test_f_optimisers_recover_the_grid_length_scale(kind, driver, monkeypatch):
    from muygpys_amd import _lib, lazy_eval
    from muygpys_amd.optimize import Bayes_optimize, L_BFGS_B_optimize
    from muygpys_amd.optimize.loss import mse_fn

    from muygpys_amd._src.gp.muygps import hip as M

    launches, solves = [], []
    real, real_solve = lazy_eval._shear_launch, M._solve_multi
    monkeypatch.setattr(lazy_eval, "_shear_launch", lambda *a: launches.append(1) or real(*a))
    monkeypatch.setattr(M, "_solve_multi", lambda *a, **k: solves.append(1) or real_solve(*a, **k))
    m, ell, tensors, kw = _grid_problem(kind)
    if driver == "L_BFGS_B":
        opt = L_BFGS_B_optimize(m, *tensors, loss_fn=mse_fn, **kw)
    else:
        opt = Bayes_optimize(m, *tensors, loss_fn=mse_fn, verbose=False, init_points=5, n_iter=20, **kw)
    got = float(opt.kernel.deformation.length_scale())
    print(driver, kind, "finds length scale", got, "in", len(launches), "fused launches")
    # the fused route served the evaluations: fused launches, none of the materialised solve
    assert launches and not solves and "shear_posterior_kernel" in _lib.last_kernel()
    assert abs(got - ell) <= 0.015


def test_g_shear_kernels_do_not_spill_and_fit_lds():
    from muygpys_amd import _lib, build

    res = json.load(open(os.path.join(build.LIBDIR, "kernel_resources.json")))
    names = [n for n in res if "shear" in n or "solve_multi" in n]
    assert len(names) >= 10, names
    for n in names:
        assert res[n].get("VGPRs Spill", 0) == 0, (n, res[n])
    assert _lib.shear_max_nn_count(torch.float64, 3) >= 50


def test_analytic_gradient_and_scale_refused_on_shear_models():
    from muygpys_amd._src.optimize.chassis import hip as CH
    from muygpys_amd._src.optimize.scale import hip as SC

    m = _model("33", 0.1, 1e-3)
    with pytest.raises(ValueError):
        CH._analytic_value_and_grad(m, lambda **kw: 0.0, ["length_scale"])
    x = torch.zeros((2, 3, 4, 3, 4), device=DEV, dtype=torch.float64)
    with pytest.raises(ValueError):
        SC._analytic_scale_optim(x, torch.zeros((2, 3, 4), device=DEV, dtype=torch.float64))
