"""GPU: a length scale per neighbourhood in one fused launch -- the two named entries (mgp_posterior_ns_generic_*,
mgp_posterior_ns_large_*) against the fp64 reference of tests/nonstationary_cases.py, their bits against the scalar
launches of the same families, position independence, bad scales, the ladder of ``fused.posterior_mean_var``, and the
functor route (HierarchicalParameter -> Isotropy -> MuyGPS on lazy handles -> optimisers) against fixtures written by
the real reference (tests/golden/hier/hier_*.npz).

The band is RTOL of tests/util.py (fp64 1e-5, fp32 1e-3): ``assert_close`` for the mean, the pure relative
``assert_rel_close`` for the variance and y^T K^-1 y, as tests/test_gpu_posterior_modes.py holds them.  Every test
prints its figures before it asserts."""

import json
import os

import numpy as np
import pytest
import torch

from tests import nonstationary_cases as NC
from tests.posterior_cases import band_error, rel_error
from tests.util import RTOL, assert_close, assert_rel_close, to_dev

pytestmark = pytest.mark.gpu

TORCH = {"float32": torch.float32, "float64": torch.float64}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hier")
KERNEL_NAME = {"generic": "mgp::fused_generic_ns_kernel<{}>", "large": "mgp::fused_large_ns_kernel<{}>"}
SCALAR_NAME = {"generic": "mgp::fused_generic_kernel<{}>", "large": "mgp::fused_large_kernel<{}>"}


def _noise(c, P, dt):
    if c["noise"] == "scalar":
        return NC.NOISE
    return to_dev(P.table if c["noise"] == "table" else P.noise_rows, dt)


def _run(c, P, ls, path=None, rows=None, scalar=False, info=None):
    """One launch of the case's entry on neighbourhoods ``rows`` (default: all) with the (b, ls_count) scales ``ls``;
    ``scalar``: the scalar launch of the same family at the scales ``ls[0]``.  Returns numpy (mean, var, ykinvy)."""
    from muygpys_amd import _lib
    from muygpys_amd.fused import KernelSpec, posterior_mean_var

    dt = TORCH[c["dtype"]]
    rows = np.arange(P.b) if rows is None else np.asarray(rows)
    noise = _noise(c, P, dt)
    if c["noise"] == "batch":
        noise = noise[to_dev(rows)].contiguous()
    lsd = to_dev(np.ascontiguousarray(ls), dt)
    if scalar:
        spec = KernelSpec(c["kernel"], c["metric"], lsd[0].clone(), noise)  # (the rounded values the NS launch reads)
    else:
        spec = KernelSpec(c["kernel"], c["metric"], 1.0, noise, length_scale_batch=lsd)
    Xq, Xn = to_dev(P.Xq, dt), to_dev(P.Xn, dt)
    ni = to_dev(P.ni[rows])
    # (no batch index: neighbourhood i reads query row i, so a subset brings its own query rows)
    bi = to_dev(P.bi[rows]) if c["bi"] else None
    if not c["bi"]:
        Xq = Xq[to_dev(rows)].contiguous()
    tg = to_dev(P.Y[P.ni[rows]] if c["gathered"] else P.Y, dt)
    out = posterior_mean_var(spec, Xq, Xn, bi, ni, tg, want_ykinvy=True, path=path or c["entry"], packed=False,
                             gathered=c["gathered"], info=info)
    torch.cuda.synchronize()
    want = (SCALAR_NAME if scalar else KERNEL_NAME)[path or c["entry"]].format(NC.CNAME[c["dtype"]])
    assert _lib.last_kernel() == want, (_lib.last_kernel(), want)
    return tuple(o.double().cpu().numpy().reshape(len(rows), -1) for o in out)


# ---- 1. both named entries against the fp64 reference -------------------------------------------------------------------
@pytest.mark.parametrize("case_id", [c["id"] for c in NC.CASES])
def test_a_named_entries_against_the_fp64_reference(case_id):
    c, P = NC.BY_ID[case_id], NC.problem(case_id)
    m_ref, v_ref, y_ref = NC.reference(case_id)
    rtol = RTOL[c["dtype"]]
    mean, var, yk = _run(c, P, P.ls)
    var = var.reshape(-1)
    print(f"FIGURES {case_id} mean {band_error(mean, m_ref) / rtol:.2e} var {rel_error(var, v_ref) / rtol:.2e} "
          f"ykinvy {rel_error(yk, y_ref) / rtol:.2e} of the band")
    assert_close(mean, m_ref, rtol, f"{case_id}: mean")
    assert_rel_close(var, v_ref, rtol, f"{case_id}: var")
    assert_rel_close(yk, y_ref, rtol, f"{case_id}: ykinvy")


# ---- 2. the bits of the scalar launch ------------------------------------------------------------------------------------
BIT_CASES = [NC._case(e, dt, k, 8, R=3, aniso=aniso, kernel=kern, metric=metric, noise="table")
             for e, k in (("generic", 31), ("large", 40)) for dt in ("float32", "float64")
             for aniso in (False, True) for kern, metric in (("matern15", "l2"), ("rbf", "F2"))]
for _c in BIT_CASES:
    NC.BY_ID.setdefault(_c["id"], _c)


@pytest.mark.parametrize("case_id", [c["id"] for c in BIT_CASES])
def test_b_constant_scales_give_the_bits_of_the_scalar_launch(case_id):
    c, P = NC.BY_ID[case_id], NC.problem(case_id)
    const = np.repeat(np.array(P.ls[:1]) * 0.37 + 0.9, P.b, axis=0)  # (b, ls_count), every row the same
    ns = _run(c, P, const)
    sc = _run(c, P, const, scalar=True)
    for name, a, s in zip(("mean", "var", "ykinvy"), ns, sc):
        assert a.tobytes() == s.tobytes(), f"{case_id}: {name} differs from the scalar launch by {np.abs(a - s).max():.3e}"


# ---- 3. position independence --------------------------------------------------------------------------------------------
PERM_CASES = [NC._case(e, "float32", 10, 8, b=300, aniso=aniso, noise="batch", bi=bi)
              for e, aniso, bi in (("generic", False, True), ("large", True, False))]
for _c in PERM_CASES:
    NC.BY_ID.setdefault(_c["id"], _c)


@pytest.mark.parametrize("case_id", [c["id"] for c in PERM_CASES])
def test_c_permuting_neighbourhoods_with_their_scales_permutes_the_outputs(case_id):
    c, P = NC.BY_ID[case_id], NC.problem(case_id)
    perm = np.random.default_rng(5).permutation(P.b)
    plain = _run(c, P, P.ls)
    moved = _run(c, P, P.ls[perm], rows=perm)
    for name, a, m in zip(("mean", "var", "ykinvy"), plain, moved):
        assert a[perm].tobytes() == m.tobytes(), f"{case_id}: {name} depends on the position in the batch"


# ---- 4. bad scales -------------------------------------------------------------------------------------------------------
BAD_CASES = [NC._case(e, dt, k, 3, b=5, aniso=aniso, R=3)
             for e, k, dt, aniso in (("generic", 12, "float32", False), ("generic", 12, "float64", True),
                                     ("large", 12, "float32", True), ("large", 12, "float64", False))]
for _c in BAD_CASES:
    NC.BY_ID.setdefault(_c["id"], _c)


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan")], ids=["zero", "negative", "nan"])
@pytest.mark.parametrize("case_id", [c["id"] for c in BAD_CASES])
def test_d_a_bad_scale_spoils_its_own_neighbourhood_alone(case_id, bad, monkeypatch):
    from muygpys_amd.config import config
    from muygpys_amd.fused import KernelSpec, posterior_mean_var

    c, P = NC.BY_ID[case_id], NC.problem(case_id)
    clean = _run(c, P, P.ls)
    ls = np.array(P.ls)
    ls[2, -1] = bad
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    with monkeypatch.context() as mp:
        mp.setattr(config.state, "check_spd", False)  # (this launch: look at info ourselves)
        got = _run(c, P, ls, info=info)
    assert int(info.item()) == 1
    keep = [0, 1, 3, 4]
    for name, a, g in zip(("mean", "var", "ykinvy"), clean, got):
        assert np.isnan(g[2]).all(), f"{case_id}: {name} of the bad neighbourhood is {g[2]}"
        assert a[keep].tobytes() == g[keep].tobytes(), f"{case_id}: {name} of a clean neighbourhood changed"
    dt = TORCH[c["dtype"]]
    spec = KernelSpec(c["kernel"], c["metric"], 1.0, NC.NOISE, length_scale_batch=to_dev(ls, dt))
    with pytest.raises(np.linalg.LinAlgError, match="length scale"):
        posterior_mean_var(spec, to_dev(P.Xq, dt), to_dev(P.Xn, dt), to_dev(P.bi), to_dev(P.ni), to_dev(P.Y, dt), path=c["entry"])


# ---- 5. the ladder -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_e_ladder(dtype):
    from muygpys_amd import _lib
    from muygpys_amd.fused import KernelSpec, posterior_mean_var

    dt, t = TORCH[dtype], NC.CNAME[dtype]
    rng = np.random.default_rng(11)
    n, d, b = 1100, 2, 3
    X, y = to_dev(rng.uniform(size=(n, d)), dt), to_dev(rng.normal(size=n), dt)
    ls = to_dev(NC.draw_scales(rng, b, 1), dt)

    def call(k, **kw):
        ni = to_dev(np.stack([rng.choice(n, size=k, replace=False) for _ in range(b)]))
        spec = KernelSpec(kw.pop("kernel", "matern15"), "l2", 1.0, 0.05, length_scale_batch=ls, **kw)
        out = posterior_mean_var(spec, X, X, to_dev(np.arange(b)), ni, y)
        torch.cuda.synchronize()
        return out

    call(10)
    assert _lib.last_kernel() == f"mgp::fused_generic_ns_kernel<{t}>"
    call(NC.lds_max(dtype, 1) + 1)
    assert _lib.last_kernel() == f"mgp::fused_large_ns_kernel<{t}>"
    with pytest.raises(ValueError):
        call(1023)  # k + 1 + R = 1025
    with pytest.raises(ValueError, match="length_scale_batch"):
        call(10, kernel="matern_gen", smoothness=1.3)


# ---- 6. the functor route against the fixtures of the real reference ------------------------------------------------------
def _hier_model(meta, knots, values, lower=None, upper=None):
    from muygpys_amd.gp.deformation import F2, Isotropy, l2
    from muygpys_amd.gp.hyperparameter import AnalyticScale, Parameter, VectorParameter
    from muygpys_amd.gp.hyperparameter.experimental import HierarchicalParameter
    from muygpys_amd.gp.kernels import RBF, Matern
    from muygpys_amd.gp.muygps import MuyGPS
    from muygpys_amd.gp.noise import HomoscedasticNoise

    bounds = (meta["bounds"][0] if lower is None else lower, meta["bounds"][1] if upper is None else upper)
    higher = RBF() if meta["higher"] == "rbf" else Matern(smoothness=Parameter(0.5))
    hp = HierarchicalParameter(knots, VectorParameter(*[Parameter(float(v), bounds) for v in values]), higher)
    deformation = Isotropy(l2 if meta["metric"] == "l2" else F2, length_scale=hp)
    kernel = RBF(deformation=deformation) if meta["kernel"] == "rbf" else Matern(smoothness=Parameter(1.5), deformation=deformation)
    return MuyGPS(kernel=kernel, noise=HomoscedasticNoise(meta["noise"]), scale=AnalyticScale())


def _count_ns_launches(monkeypatch):
    from muygpys_amd import lazy_eval

    launches = []
    real = lazy_eval._ns_launch
    monkeypatch.setattr(lazy_eval, "_ns_launch", lambda *a: launches.append(1) or real(*a))
    return launches


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", ["hier_rbf_F2", "hier_m15_l2"])
def test_f_functor_route_against_the_reference_fixtures(name, dtype, monkeypatch):
    from muygpys_amd import _lib, lazy
    from muygpys_amd.gp.tensors import batch_features_tensor
    from muygpys_amd.optimize import L_BFGS_B_optimize
    from muygpys_amd.optimize.loss import lool_fn, mse_fn

    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.loads(str(g["meta"]))
    dt, rtol = TORCH[dtype], RTOL[dtype]
    launches = _count_ns_launches(monkeypatch)
    X, y = to_dev(g["features"], dt), to_dev(g["targets"], dt)
    bi, ni = to_dev(g["batch_idx"]), to_dev(g["nn_idx"])
    m = _hier_model(meta, g["knots"], g["knot_values"])
    cross, pair, y_b, y_nn = m.make_train_tensors(bi, ni, X, y)
    assert isinstance(pair, lazy.LazyDiffs) and isinstance(y_nn, lazy.LazyTargets)
    bf = batch_features_tensor(X, bi)
    scales = m.kernel.deformation.length_scale(bf)
    assert scales.is_cuda and tuple(scales.shape) == (meta["b"],)
    Kin, Kc = m.kernel(pair, batch_features=bf), m.kernel(cross, batch_features=bf)
    assert isinstance(Kin, lazy.LazyCov) and Kin.diffs.length_scale_batch is not None
    mean = m.posterior_mean(Kin, Kc, y_nn)
    assert _lib.last_kernel() == f"mgp::fused_generic_ns_kernel<{NC.CNAME[dtype]}>"
    var = m.get_opt_var_fn()(Kin, Kc)
    sigma_sq = m.scale.get_opt_fn(m)(Kin, y_nn)
    assert len(launches) == 1, "mean, variance and analytic scale of one evaluation share one fused NS launch"
    host = lambda t: t.double().cpu().numpy()  # noqa: E731
    sig = host(sigma_sq).reshape(-1)
    print(f"FIGURES {name} {dtype} scales {band_error(host(scales), g['scales']) / rtol:.2e} mean "
          f"{band_error(host(mean), g['mean']) / rtol:.2e} var {rel_error(host(var), g['var_unscaled']) / rtol:.2e} sigma_sq "
          f"{rel_error(sig, g['sigma_sq']) / rtol:.2e} of the band")
    assert_close(host(scales), g["scales"], rtol, "scales")
    assert_close(host(mean), g["mean"], rtol, "mean")
    assert_rel_close(host(var), g["var_unscaled"], rtol, "var")
    assert_rel_close(sig, g["sigma_sq"], rtol, "sigma_sq")
    # the objective at the two probes, through the reference's own call: make_obj_fn(..., batch_features=)
    names = m.get_opt_params()[0]
    for lname, lfn in (("lool", lool_fn), ("mse", mse_fn)):
        obj = L_BFGS_B_optimize.make_obj_fn(m, y_b, y_nn, cross, pair, batch_features=bf, loss_fn=lfn)
        got = np.array([float(obj(**{n: float(v) for n, v in zip(names, p)})) for p in g["probes"]])
        print(f"FIGURES {name} {dtype} obj_{lname} {band_error(got, g['obj_' + lname]) / rtol:.2e} of the band")
        assert_close(got, g["obj_" + lname], rtol, f"obj_{lname}")
    # the materialised route: the per-function kernels with the scale broadcast along axis 0
    Kin_m, Kc_m = lazy.force(Kin), lazy.force(Kc)
    assert_close(host(Kin_m), g["Kin"], rtol, "materialised Kin")
    assert_close(host(Kc_m), g["Kcross"], rtol, "materialised Kcross")
    # a handle that carries per-batch scales divided by a scalar: the scales are kept (materialised), not replaced
    halved = Kc.diffs / 2.0
    assert isinstance(halved, torch.Tensor)
    assert_close(host(halved), host(lazy.force(Kc.diffs)) / 2.0, rtol, "scaled distances / 2")
    before = len(launches)
    mean_m = m.posterior_mean(Kin_m, Kc_m, lazy.force(y_nn))
    var_m = m.get_opt_var_fn()(Kin_m, Kc_m)
    assert len(launches) == before  # (mgp_solve_* on the materialised tensors: no fused NS launch)
    assert_close(host(mean_m), host(mean), rtol, "materialised mean against the fused one")
    assert_rel_close(host(var_m), host(var), rtol, "materialised variance against the fused one")
    # ... and Isotropy on materialised distances with a (b,) scale: broadcast along axis 0, as the reference does
    dist = m.kernel.deformation.pairwise_tensor(X, ni)
    scaled = m.kernel.deformation(dist, length_scale=scales)
    p = 1 if meta["metric"] == "l2" else 2
    assert_close(host(scaled), host(dist) / g["scales"][:, None, None] ** p, rtol, "Isotropy on materialised distances")


# ---- 7. the optimisers ----------------------------------------------------------------------------------------------------
def _optimiser_problem():
    from muygpys_amd.gp.tensors import batch_features_tensor

    rng = np.random.default_rng(77)
    n, d, k, b = 1500, 2, 10, 256
    Xh = rng.uniform(size=(n, d))
    yh = np.sin(2 * np.pi * (1.0 + 5.0 * (1.0 - Xh[:, 0]) ** 2) * Xh[:, 0]) + 0.05 * rng.normal(size=n)
    bi = np.sort(rng.choice(n, size=b, replace=False))
    d2 = ((Xh[bi][:, None, :] - Xh[None, :, :]) ** 2).sum(-1)
    ni = np.argsort(d2, axis=1, kind="stable")[:, 1:k + 1]
    # (a Matern-1/2 higher level and moderate bounds: the scales between positive knot values stay positive)
    meta = dict(kernel="matern15", metric="l2", noise=1e-2, higher="matern05", bounds=[0.05, 0.6])
    knots = np.array([[0.05, 0.5], [0.5, 0.5], [0.95, 0.5]])
    m = _hier_model(meta, knots, [0.3, 0.3, 0.3])
    X, y = to_dev(Xh, torch.float64), to_dev(yh, torch.float64)
    bi, ni = to_dev(bi), to_dev(ni)
    cross, pair, y_b, y_nn = m.make_train_tensors(bi, ni, X, y)
    return m, (y_b, y_nn, cross, pair), batch_features_tensor(X, bi)


@pytest.mark.parametrize("driver", ["L_BFGS_B", "Bayes"])
def test_g_optimisers_work_on_a_hierarchical_model(driver, monkeypatch):
    from muygpys_amd import _lib
    from muygpys_amd.optimize import Bayes_optimize, L_BFGS_B_optimize

    m, tensors, bf = _optimiser_problem()
    launches = _count_ns_launches(monkeypatch)
    names, x0, bounds = m.get_opt_params()
    assert list(names) == ["length_scale0", "length_scale1", "length_scale2"]
    obj = L_BFGS_B_optimize.make_obj_fn(m, *tensors, batch_features=bf)
    at_x0 = float(obj(**dict(zip(names, map(float, x0)))))
    if driver == "L_BFGS_B":
        opt = L_BFGS_B_optimize(m, *tensors, batch_features=bf)
    else:
        opt = Bayes_optimize(m, *tensors, batch_features=bf, init_points=3, n_iter=5, random_state=0)
    got = np.asarray(opt.kernel.deformation.length_scale.knot_values(), dtype=np.float64)
    at_opt = float(obj(**dict(zip(names, map(float, got)))))
    print(f"FIGURES {driver}: knot values {x0} -> {got}; objective {at_x0:.6g} -> {at_opt:.6g} in {len(launches)} fused launches")
    assert launches and "ns_kernel" in _lib.last_kernel()
    assert np.all(got >= bounds[:, 0]) and np.all(got <= bounds[:, 1])
    assert at_opt >= at_x0, "the objective (maximised) at the returned knot values is no worse than at x0"
    assert opt is not m and np.array_equal(m.kernel.deformation.length_scale.knot_values(), x0)


def test_g_analytic_gradient_raises():
    from muygpys_amd.optimize import L_BFGS_B_optimize

    m, tensors, bf = _optimiser_problem()
    with pytest.raises(ValueError, match="hierarchical"):
        L_BFGS_B_optimize(m, *tensors, batch_features=bf, analytic_gradient=True)
