"""GPU: the hyper-parameter backward with a length scale per neighbourhood -- the three kernel rungs of
mgp_hyper_backward_ns_* / mgp_hyper_backward_ns_large_* against the torch-CPU fp64 autograd reference of
tests/nonstationary_backward_cases.py, the bits of the scalar launches at constant scales, position independence, bad
scales, and ``fused.loocv_value_and_grad`` / ``L_BFGS_B_optimize(analytic_gradient="knots")`` on a hierarchical model.

The band is the backward tests' own: RTOL of tests/backward_cases.py (fp64 1e-5, fp32 3e-3) on ``band_error``, printed
before it is asserted."""

import numpy as np
import pytest
import torch

from tests import nonstationary_backward_cases as BC
from tests import nonstationary_cases as NC
from tests.backward_cases import RTOL, band_error
from tests.util import to_dev

pytestmark = pytest.mark.gpu

TORCH = {"float32": torch.float32, "float64": torch.float64}


def expected_kernel(c):
    T, k, d = NC.CNAME[c["dtype"]], c["k"], c["d"]
    if c["rung"] == "slab":
        return f"mgp::ns_slab_backward_kernel<{T}>"
    if c["rung"] == "lds":
        return f"mgp::ns_lds_backward_kernel<{T}> [threads={64 if k + 2 <= 64 else 128}"
    pieces = -(-d // (16 // NC.ES[c["dtype"]]))
    dg = next(g for g in (4, 8, 10, 12, 16) if pieces <= g)
    return f"mgp::ns_wave_backward_kernel<{T},{32 if k + 2 <= 32 else 64},{dg}>"


def run(c, P, ls, loocv, rows=None, scalar=False):
    """One launch of the case's rung on neighbourhoods ``rows`` with the (b, ls_count) scales ``ls``; ``scalar``: the
    scalar launch of the same kernel family at ``ls[0]``.  Returns numpy (g_l, g_n, info)."""
    from muygpys_amd import _lib

    dt, P_ = TORCH[c["dtype"]], _lib.ptr
    rows = np.arange(P.b) if rows is None else np.asarray(rows)
    b, k = len(rows), c["k"]
    gm, gv, gyk = BC.cotangents(c["id"], P.b)
    X, ni, bi = to_dev(P.Xn, dt), to_dev(P.ni[rows]), to_dev(P.bi[rows])
    Y = to_dev(P.Y[:, :1] if loocv else P.Y, dt)
    gm, gv, gyk = to_dev((gm[:, :1] if loocv else gm)[rows], dt), to_dev(gv[rows], dt), to_dev(gyk[rows], dt)
    table = to_dev(P.table, dt)
    noise = (_lib.NOISE_SCALAR, NC.NOISE, None) if c["noise"] == "scalar" else (_lib.NOISE_TABLE, 0.0, P_(table))
    lsd = to_dev(np.ascontiguousarray(ls), dt)
    g_l = torch.zeros((b, lsd.shape[1]), device="cuda", dtype=dt)
    g_n = torch.zeros((b, k), device="cuda", dtype=dt)
    info = torch.zeros(1, device="cuda", dtype=torch.int32)
    slab = c["rung"] == "slab"
    base = "hyper_backward_large" if scalar else "hyper_backward_ns_large" if slab else "hyper_backward_ns"
    args = (P_(X), c["d"], P_(bi), P_(ni), b, k, P_(Y), Y.shape[1], *noise, _lib.KERNEL_IDS[c["kernel"]],
            _lib.METRIC_IDS[c["metric"]], P_(lsd), lsd.shape[1], P_(gm), P_(gv), P_(gyk) if loocv else None)
    ws = _lib.backward_large_workspace(dt, k, b, X.device)
    tail = (P_(ws), ws.numel(), _lib.stream_ptr()) if slab else (_lib.stream_ptr(),)
    if scalar and not slab:  # (a shape whose scalar ladder ends on the LDS workgroup kernel: asserted by name below)
        assert loocv
        base = "loocv_backward"
        rc = _lib.fn(base, dt)(*args[:7], *args[8:], P_(g_l), P_(g_n), P_(info), *tail)
    else:
        rc = _lib.fn(base, dt)(*args, P_(g_l), P_(g_n), P_(info), *tail)
    _lib.check(rc, base)
    torch.cuda.synchronize()
    want = ("mgp::hyper_backward_large_kernel<" if slab else "mgp::backward_kernel<") if scalar else expected_kernel(c)
    assert _lib.last_kernel().startswith(want), (_lib.last_kernel(), want)
    return g_l.double().cpu().numpy(), g_n.double().cpu().numpy(), int(info.item())


# ---- 1. every rung against the reference, both forms ---------------------------------------------------------------------
@pytest.mark.parametrize("loocv", [True, False], ids=["loocv", "posterior"])
@pytest.mark.parametrize("case_id", [c["id"] for c in BC.REFERENCE_CASES])
def test_a_rungs_against_the_fp64_reference(case_id, loocv):
    c, P = NC.BY_ID[case_id], NC.problem(case_id)
    ref_l, ref_n = BC.reference(case_id, loocv)
    g_l, g_n, info = run(c, P, P.ls, loocv)
    rtol = RTOL[c["dtype"]]
    print(f"FIGURES {case_id} {'loocv' if loocv else 'posterior'} g_l {band_error(g_l, ref_l) / rtol:.2e} "
          f"g_n {band_error(g_n, ref_n) / rtol:.2e} of the band")
    assert info == 0
    assert band_error(g_l, ref_l) <= rtol and band_error(g_n, ref_n) <= rtol


# ---- 2. constant scales: the bits of the scalar launch of the same family ------------------------------------------------
# (LDS: 67 features -- beyond the wave-sized kernels of the scalar entry and no multiple of a 16-byte piece, so its ladder
# ends on backward_kernel -- at one wave per workgroup: with several, the order of that kernel's LDS atomics is free and
# its Anisotropy partials are not reproducible between two launches of itself)
BIT_CASES = [BC.case(rung, dt, k, d, aniso=aniso, kernel=kern, metric=metric, noise="table")
             for rung, k, d in (("lds", 10, 67), ("slab", 40, 8)) for dt in ("float32", "float64") for aniso in (False, True)
             for kern, metric in (("matern15", "l2"), ("rbf", "F2"))]
# (... and the 128-thread form of the LDS kernel under Isotropy, whose one two-term sum across waves commutes)
BIT_CASES += [BC.case("lds", dt, 70, 8, kernel=kern, metric=metric, noise="table")
              for dt in ("float32", "float64") for kern, metric in (("matern15", "l2"), ("rbf", "F2"))]


@pytest.mark.parametrize("case_id", [c["id"] for c in BIT_CASES])
def test_b_constant_scales_give_the_bits_of_the_scalar_launch(case_id):
    c, P = NC.BY_ID[case_id], NC.problem(case_id)
    const = np.repeat(np.array(P.ls[:1]) * 0.37 + 0.9, P.b, axis=0)
    ns, sc = run(c, P, const, True), run(c, P, const, True, scalar=True)
    for name, a, s in zip(("g_l", "g_n"), ns, sc):
        assert a.tobytes() == s.tobytes(), f"{case_id}: {name} differs from the scalar launch by {np.abs(a - s).max():.3e}"


# ---- 3. position independence (on the wave rung: a scale taken from the wrong half of the wave) --------------------------
PERM_CASES = [BC.case("wave", "float32", 5, 3, b=33), BC.case("wave", "float64", 20, 8, b=33), BC.case("wave", "float64", 40, 8, b=9),
              BC.case("lds", "float32", 10, 12, aniso=True, b=33), BC.case("slab", "float32", 40, 8, b=33)]


@pytest.mark.parametrize("case_id", [c["id"] for c in PERM_CASES])
def test_c_permuting_neighbourhoods_with_their_scales_permutes_the_rows(case_id):
    c, P = NC.BY_ID[case_id], NC.problem(case_id)
    perm = np.random.default_rng(5).permutation(P.b)
    base, moved = run(c, P, P.ls, True), run(c, P, P.ls[perm], True, rows=perm)
    for name, a, m in zip(("g_l", "g_n"), base, moved):
        assert a[perm].tobytes() == m.tobytes(), f"{case_id}: {name}"


# ---- 4. bad scales ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [0.0, -1.0, np.inf, np.nan])
@pytest.mark.parametrize("case_id", [c["id"] for c in PERM_CASES])
def test_d_a_bad_scale_costs_its_own_neighbourhood_alone(case_id, value):
    c, P = NC.BY_ID[case_id], NC.problem(case_id)
    at = 3  # (wave rung at two neighbourhoods per wave: the second half of a wave)
    ls = np.array(P.ls)
    ls[at, -1] = value
    keep = np.delete(np.arange(P.b), at)
    g_l, g_n, info = run(c, P, ls, True)
    ref_l, ref_n, _ = run(c, P, ls[keep], True, rows=keep)
    assert info == 1
    assert np.isnan(g_l[at]).all() and np.isnan(g_n[at]).all()
    assert g_l[keep].tobytes() == ref_l.tobytes() and g_n[keep].tobytes() == ref_n.tobytes()


# ---- 5. end to end: loocv_value_and_grad on a hierarchical model, pulled back to the knots -------------------------------
def hierarchical_problem():
    """60 neighbourhoods of 12 neighbours on a line, 6 knots: (the parameter, its named form as Isotropy holds it, X, y,
    bi, ni, batch features), fp64 on the device.  The higher-level kernel is the Matern 1/2, whose 1-D posterior mean
    between two knots is a positive combination of their values: positive knot values give positive scales."""
    from muygpys_amd.gp.deformation import Isotropy, l2
    from muygpys_amd.gp.hyperparameter import Parameter, VectorParameter
    from muygpys_amd.gp.hyperparameter.experimental import HierarchicalParameter
    from muygpys_amd.gp.kernels import Matern

    rng = np.random.default_rng(NC.SEED)
    X = np.sort(rng.uniform(size=(400, 1)), axis=0)
    y = np.sin(2.0 * np.pi * (1.0 + 5.0 * (1.0 - X[:, 0]) ** 2) * X[:, 0]) + 0.05 * rng.normal(size=400)
    bi = rng.choice(400, size=60, replace=False)
    dist = ((X[bi][:, None, :] - X[None, :, :]) ** 2).sum(-1)
    ni = np.argsort(dist, axis=1)[:, 1:13]  # (the nearest is the point itself)
    values = VectorParameter(*[Parameter(v, (0.01, 1.0)) for v in (0.05, 0.08, 0.1, 0.15, 0.2, 0.3)])
    higher = Matern(smoothness=Parameter(0.5), deformation=Isotropy(l2, length_scale=Parameter(0.5)))
    raw = HierarchicalParameter(np.linspace(0.0, 1.0, 6)[:, None], values, higher)
    Xd = to_dev(X)
    return raw, Isotropy(l2, length_scale=raw).length_scale, Xd, to_dev(y), to_dev(bi), to_dev(ni), Xd[to_dev(bi)].contiguous()


def reference_loss(loss, scale, sigma_noise, noise, X, y, bi, ni, C, Kin, v):
    """(value, d / d knot values, d / d noise) by torch-CPU fp64 autograd through the knot GP, the dense posterior and
    the loss (reference: _src/optimize/loss/numpy.py:22-117, gp/hyperparameter/scale.py:205-217)."""
    v = v.clone().requires_grad_(True)
    eps = torch.tensor(float(noise), dtype=torch.float64, requires_grad=True)
    ls = (C @ torch.linalg.solve(Kin, v))[:, None]
    b, k = ni.shape
    mean, var, yk = BC.dense_posterior("matern15", "l2", X, bi, ni, y[:, None], ls, eps.expand(b, k))
    if sigma_noise is not None:
        yk = BC.dense_posterior("matern15", "l2", X, bi, ni, y[:, None], ls, torch.full((b, k), float(sigma_noise), dtype=torch.float64))[2]
    mean, yk = mean[:, 0], yk[:, 0]
    r = mean - y[bi]
    s = f0 = yk.sum() / (b * k)
    for _ in range(1, scale[1]):
        s = 0.5 * (s + f0 / s)
    if loss == "lool":
        value = (r * r / (s * var) + torch.log(s * var)).sum()
    elif loss == "mse":
        value = (r * r).mean()
    elif loss == "pseudo_huber":
        value = 1.5**2 * (torch.sqrt(1.0 + (r / 1.5) ** 2) - 1.0).sum()
    else:
        value = (2.0 * 9.0 * (torch.sqrt(1.0 + r * r / (9.0 * s * var)) - 1.0) + torch.log(s * var)).sum()
    g_v, g_eps = torch.autograd.grad(value, [v, eps])
    return float(value.detach()), g_v.numpy(), float(g_eps)


@pytest.mark.parametrize("loss, scale, sigma_noise", [("lool", ("analytic", 1), None), ("lool", ("analytic", 3), None),
                                                     ("lool", ("analytic", 1), 2e-2), ("mse", ("analytic", 1), None),
                                                     ("pseudo_huber", ("analytic", 1), None), ("looph", ("analytic", 1), None)])
def test_e_loocv_value_and_grad_pulled_back_to_the_knots(loss, scale, sigma_noise):
    from muygpys_amd.fused import KernelSpec, loocv_value_and_grad

    raw, hp, X, y, bi, ni, bf = hierarchical_problem()
    noise = 5e-2
    spec = KernelSpec("matern15", "l2", 1.0, noise, length_scale_batch=hp(bf))
    value, g_l, g_noise = loocv_value_and_grad(spec, X, y, bi, ni, loss=loss, scale=scale, sigma_noise=sigma_noise)
    assert isinstance(g_l, torch.Tensor) and g_l.is_cuda and tuple(g_l.shape) == (60, 1)
    g_knots = hp.pullback(bf, g_l)
    cpu = lambda t: t.cpu()  # noqa: E731
    ref = reference_loss(loss, scale, sigma_noise, noise, cpu(X), cpu(y), cpu(bi), cpu(ni), cpu(hp._lower_cross(bf)),
                         cpu(hp._knots_on(bf.device)[1]), torch.tensor(hp.knot_values(), dtype=torch.float64))
    rtol = RTOL["float64"]
    print(f"FIGURES {loss} {scale} split={sigma_noise}: value {abs(value - ref[0]) / abs(ref[0]) / rtol:.2e} "
          f"knots {band_error(g_knots, ref[1]) / rtol:.2e} noise {abs(g_noise - ref[2]) / abs(ref[2]) / rtol:.2e} of the band")
    assert abs(value - ref[0]) <= rtol * abs(ref[0])
    assert band_error(g_knots, ref[1]) <= rtol
    assert abs(g_noise - ref[2]) <= rtol * abs(ref[2])


# ---- 6. the optimiser ------------------------------------------------------------------------------------------------------
def test_f_lbfgsb_with_the_analytic_gradient(monkeypatch):
    from muygpys_amd import _lib
    from muygpys_amd.gp import MuyGPS
    from muygpys_amd.gp.deformation import Isotropy, l2
    from muygpys_amd.gp.hyperparameter import AnalyticScale, Parameter
    from muygpys_amd.gp.kernels import Matern
    from muygpys_amd.gp.noise import HomoscedasticNoise
    from muygpys_amd.optimize import L_BFGS_B_optimize
    from muygpys_amd.optimize.loss import lool_fn

    raw, hp, X, y, bi, ni, bf = hierarchical_problem()
    model = MuyGPS(kernel=Matern(smoothness=Parameter(1.5), deformation=Isotropy(l2, length_scale=raw)),
                   noise=HomoscedasticNoise(5e-2), scale=AnalyticScale())
    cross, pair, y_b, y_nn = model.make_train_tensors(bi, ni, X, y)
    launches = {"n": 0}
    real_fn = _lib.fn

    def counting_fn(base, dtype):
        launches["n"] += base.startswith(("posterior", "hyper_backward", "loocv"))
        return real_fn(base, dtype)

    monkeypatch.setattr(_lib, "fn", counting_fn)
    obj = L_BFGS_B_optimize.make_obj_fn(model, y_b, y_nn, cross, pair, batch_features=bf, loss_fn=lool_fn)
    names, x0, bounds = model.get_opt_params()
    start = float(obj(**dict(zip(names, x0))))
    report = {}
    for analytic in ("knots", False):
        launches["n"] = 0
        fitted = L_BFGS_B_optimize(model, y_b, y_nn, cross, pair, batch_features=bf, loss_fn=lool_fn, analytic_gradient=analytic)
        knots = np.asarray(fitted.kernel.deformation.length_scale.knot_values(), dtype=np.float64)
        count = launches["n"]
        report[analytic] = (float(obj(**dict(zip(names, knots)))), count, knots)
    print(f"FIGURES objective at the start {start:.6f}; analytic gradient: {report['knots'][0]:.6f} after {report['knots'][1]} "
          f"launches; finite differences: {report[False][0]:.6f} after {report[False][1]} launches")
    value, _, knots = report["knots"]
    assert np.all(knots >= np.asarray(bounds)[:, 0]) and np.all(knots <= np.asarray(bounds)[:, 1])
    assert value >= start  # (the objective is maximised)


# ---- 7. what stays refused ---------------------------------------------------------------------------------------------------
def test_g_refusals():
    from muygpys_amd.fused import KernelSpec, class_value_and_grad, loocv_value_and_grad

    raw, hp, X, y, bi, ni, bf = hierarchical_problem()
    spec = KernelSpec("matern15", "l2", 1.0, 5e-2, length_scale_batch=hp(bf))
    with pytest.raises(ValueError, match="length_scale_batch.*sharded"):
        loocv_value_and_grad(spec, X, y, bi, ni, reduce_fn=lambda t: t)
    with pytest.raises(ValueError, match="length_scale_batch"):
        class_value_and_grad(spec, X, torch.stack([y, -y], dim=1), bi, ni)
    spec.kernel, spec.smoothness = "matern_gen", 1.3
    with pytest.raises(ValueError, match="length_scale_batch: the general-smoothness"):
        loocv_value_and_grad(spec, X, y, bi, ni)
