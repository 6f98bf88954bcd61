"""GPU: the hyper-parameter backward beyond LDS (csrc/mgp_backward_large.hip: ``mgp_hyper_backward_large_*`` on the
slab factor of csrc/mgp_large_factor.h) against a numpy fp64 reference -- ``np.linalg.solve`` on ``orc.kernel_tensors`` +
nugget, the cotangent formulas of include/muygpys_hip.h contracted with ``orc._kernel_adjoint`` -- at every block and
tile edge through the C entry, over the nn_count range no gradient served before through ``fused.loocv_value_and_grad``
/ ``fused.class_value_and_grad``, against the LDS backward where both serve, placement invariance bit for bit, failure
semantics and the L-BFGS-B driver.

Inputs as in tests/test_gpu_large.py: uniform [0, 1]^d points, length scale 0.5 (per feature: 0.5 x uniform(0.7, 1.5)),
nugget 1e-2, responses sin(3 sum x) + 0.1 noise, random distinct neighbours, random normal cotangents.  Tolerances: the
project's for gradients -- fp64 1e-5, fp32 3 x 1e-3 -- through tests/util.assert_close, per element of the
(b, ls_count) and (b, k) partials."""

import numpy as np
import pytest
import torch

from oracle import muygps_oracle as orc
from tests.util import RTOL, assert_close, to_dev

pytestmark = pytest.mark.gpu

TORCH = {"float32": torch.float32, "float64": torch.float64}
GRAD_RTOL = {"float64": 1e-5, "float32": 3e-3}
KERNELS = ("rbf", "matern05", "matern15", "matern25", "maternInf")
LS, NUGGET = 0.5, 1e-2


def limit(dtype):
    """The last nn_count the LDS backward serves."""
    from muygpys_amd import _lib

    return _lib.load().mgp_max_nn_count_backward(4 if dtype == "float32" else 8)


def make_table(rng, n, d, R=1):
    X = rng.uniform(size=(n, d))
    Y = np.stack([np.sin(3.0 * X.sum(1) + r) + 0.1 * rng.normal(size=n) for r in range(R)], axis=1)
    return X, Y


def neighbourhoods(rng, n, b, k):
    return np.stack([rng.choice(n, size=k, replace=False) for _ in range(b)])


def length_scales(rng, d, aniso):
    return LS * rng.uniform(0.7, 1.5, size=d) if aniso else LS


# ---- the fp64 reference ------------------------------------------------------------------------------------------------
def _systems(ospec, X, bi, ni, noise_rows):
    for i in range(len(bi)):
        cd = orc.crosswise_tensor(X, X, bi[i:i + 1], ni[i:i + 1])
        pd = orc.pairwise_tensor(X, ni[i:i + 1])
        Kc, Kin = orc.kernel_tensors(ospec, cd, pd)
        yield i, cd, pd, Kc[0], Kin[0] + np.diag(noise_rows[i])


def reference_partials(ospec, X, bi, ni, Y, noise_rows, gm, gv, gyk):
    """(grad_ls (b, ls_count), grad_noise (b, k)) in fp64.  ``gyk`` given: the LOOCV form (``gm`` (b,), one response);
    else the posterior form (``gm`` (b, R)).  ``gm`` / ``gv`` may be None (= 0).  ``noise_rows``: the (b, k) diagonal."""
    b, k = ni.shape
    g_ls = np.zeros((b, np.size(ospec.length_scale)))
    g_n = np.zeros((b, k))
    for i, cd, pd, c, K in _systems(ospec, X, bi, ni, noise_rows):
        Yn = Y[ni[i]]
        if gyk is not None:
            yt, gm1, gy = Yn[:, 0], (0.0 if gm is None else gm[i]), gyk[i]
        else:
            yt, gm1, gy = (np.zeros(k) if gm is None else Yn @ gm[i]), 1.0, 0.0
        g = 0.0 if gv is None else gv[i]
        a, w = np.linalg.solve(K, np.stack([c, yt], axis=1)).T
        G = g * np.outer(a, a) - gm1 * np.outer(a, w) - gy * np.outer(w, w)  # d / d K, every entry its own variable
        gc = gm1 * w - 2.0 * g * a                                            # d / d c
        g_n[i] = np.diag(G)
        g_ls[i] = orc._kernel_adjoint(ospec, pd, G[None])[1] + orc._kernel_adjoint(ospec, cd, gc[None])[1]
    return g_ls, g_n


def reference_outputs(ospec, X, bi, ni, Y, noise_rows):
    """mean (b, R), var (b,), ykinvy (b, R) in fp64."""
    b, R = len(bi), Y.shape[1]
    mean, var, yk = np.zeros((b, R)), np.zeros(b), np.zeros((b, R))
    for i, _, _, c, K in _systems(ospec, X, bi, ni, noise_rows):
        Yn = Y[ni[i]]
        S = np.linalg.solve(K, np.concatenate([c[:, None], Yn], axis=1))
        mean[i], var[i], yk[i] = c @ S[:, 1:], 1.0 - c @ S[:, 0], np.einsum("kr,kr->r", Yn, S[:, 1:])
    return mean, var, yk


# ---- the C entry -------------------------------------------------------------------------------------------------------
def entry(dtype, X_d, bi_d, ni_d, Y_d, noise, kernel, metric, ls, gm, gv, gyk, want=("ls", "noise"), workspace=None,
          sentinel=0.0):
    """One ``mgp_hyper_backward_large_*`` call.  ``noise``: a float, a (n,) table or a (b, k) tensor on the device;
    ``workspace``: a uint8 tensor (None: the recommended size).  Returns (grad_ls, grad_noise, info) -- the outputs
    pre-filled with ``sentinel``, None where not asked for."""
    from muygpys_amd import _lib
    from muygpys_amd.fused import KernelSpec

    t = TORCH[dtype]
    lib, P = _lib.load(), _lib.ptr
    b, k = ni_d.shape
    d, R = X_d.shape[1], Y_d.shape[1]
    spec = KernelSpec(kernel, metric, 1.0, 0.0)
    ls_d = to_dev(np.atleast_1d(ls), t)
    if isinstance(noise, float):
        mode = (0, noise, None)
    else:
        mode = (1 if noise.ndim == 1 else 2, 0.0, P(noise))
    if workspace is None:
        workspace = torch.empty(lib.mgp_backward_large_workspace_bytes(X_d.element_size(), k, b), dtype=torch.uint8, device="cuda")
    g_l = torch.full((b, ls_d.numel()), sentinel, device="cuda", dtype=t) if "ls" in want else None
    g_n = torch.full((b, k), sentinel, device="cuda", dtype=t) if "noise" in want else None
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    cot = [None if g is None else to_dev(g, t) for g in (gm, gv, gyk)]
    rc = _lib.fn("hyper_backward_large", t)(P(X_d), d, P(bi_d), P(ni_d), b, k, P(Y_d), R, *mode, spec.kernel_id(),
                                            spec.metric_id(), P(ls_d), ls_d.numel(), *[P(g) for g in cot], P(g_l), P(g_n),
                                            P(info), P(workspace), workspace.numel(), _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert _lib.last_kernel() == f"mgp::hyper_backward_large_kernel<{'float' if dtype == 'float32' else 'double'}>"
    return g_l, g_n, int(info.item())


def cotangents(rng, form, b):
    """(gm, gv, gyk, R) of the three forms the entry takes."""
    if form == "loocv":
        return rng.normal(size=b), rng.normal(size=b), rng.normal(size=b), 1
    if form == "posterior":
        return rng.normal(size=(b, 1)), rng.normal(size=b), None, 1
    return rng.normal(size=(b, 3)), None, None, 3  # "posterior3": three responses, no variance cotangent


def check_partials(got, ref, dtype, what):
    for g, r, name in zip(got, ref, ("grad_ls", "grad_noise")):
        if g is None:
            continue
        g = g.double().cpu().numpy()
        print(f"{what}: {name} max |err| {np.abs(g - r).max():.3e}, rms(ref) {np.sqrt(np.mean(r * r)):.3e}")
        assert_close(g, r, GRAD_RTOL[dtype], f"{what}: {name}")


# ---- 0. the reference itself -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aniso", [False, True])
@pytest.mark.parametrize("kernel, metric", [("matern15", "l2"), ("rbf", "F2")])
def test_kernel_where_the_reference_is_pinned_to_the_oracle(kernel, metric, aniso):
    """One small case on which the reference above is itself pinned: where grad_ykinvy is NULL its sum over the batch is
    ``orc.posterior_vjp``; with all three cotangents it is the central difference of sum gm mean + gv var + gyk ykinvy.
    The kernel is then checked against it in both forms."""
    rng = np.random.default_rng(5)
    n, d, b, k = 60, 3, 4, 7
    X, Y = make_table(rng, n, d, 3)
    ni, bi = neighbourhoods(rng, n, b, k), rng.choice(n, size=b, replace=False)
    ls = length_scales(rng, d, aniso)
    ospec = orc.Spec(kernel, metric, ls, NUGGET)
    rows = np.full((b, k), NUGGET)
    gm, gv = rng.normal(size=(b, 3)), rng.normal(size=b)
    p_ls, p_n = reference_partials(ospec, X, bi, ni, Y, rows, gm, gv, None)
    vjp = orc.posterior_vjp(ospec, X, X, bi, ni, Y, gm, gv)
    np.testing.assert_allclose(p_ls.sum(0), vjp["length_scale"], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(p_n.sum(), vjp["noise"], rtol=1e-10, atol=1e-12)
    # the LOOCV form against central differences, per neighbourhood
    gm1, gyk = rng.normal(size=b), rng.normal(size=b)
    g_ls, g_n = reference_partials(ospec, X, bi, ni, Y[:, :1], rows, gm1, gv, gyk)

    def value(ls_, rows_):
        m, v, yk = reference_outputs(orc.Spec(kernel, metric, ls_, NUGGET), X, bi, ni, Y[:, :1], rows_)
        return gm1 * m[:, 0] + gv * v + gyk * yk[:, 0]  # (b,): one term per neighbourhood

    h = 1e-6
    for c in range(np.size(ls)):
        e = np.zeros(np.size(ls))
        e[c] = h
        up, dn = (ls + e, ls - e) if aniso else (ls + h, ls - h)
        np.testing.assert_allclose(g_ls[:, c], (value(up, rows) - value(dn, rows)) / (2 * h), rtol=2e-6, atol=1e-7)
    for r in (0, k - 1):
        e = np.zeros((b, k))
        e[:, r] = h
        np.testing.assert_allclose(g_n[:, r], (value(ls, rows + e) - value(ls, rows - e)) / (2 * h), rtol=2e-6, atol=1e-7)
    # the kernel on this very case, posterior form (three responses) and LOOCV form
    t = TORCH["float64"]
    Xd, Yd, bi_d, ni_d = to_dev(X, t), to_dev(Y, t), to_dev(bi), to_dev(ni)
    got = entry("float64", Xd, bi_d, ni_d, Yd, NUGGET, kernel, metric, ls, gm, gv, None)
    assert got[2] == 0
    check_partials(got[:2], (p_ls, p_n), "float64", "posterior form")
    got = entry("float64", Xd, bi_d, ni_d, Yd[:, :1].contiguous(), NUGGET, kernel, metric, ls, gm1, gv, gyk)
    assert got[2] == 0
    check_partials(got[:2], (g_ls, g_n), "float64", "LOOCV form")


# ---- 1. block and tile edges at small size -----------------------------------------------------------------------------
# k: one and two rows, the panel edge (32), the fp64 tile edge inside it, two and three panels, and 126 / 127 on either
# side of the 256 / 512-thread switch at 128 rows (k + 2).  d = 70 takes two feature chunks.  F2 goes with rbf and
# matern05 only (tests/test_gpu_large.py: the other three are no covariance functions of the squared distance).
EDGE_K = (1, 2, 31, 32, 33, 67, 96, 126, 127)
EDGE_D = (1, 3, 8, 40, 70)
FORMS = ("loocv", "posterior", "posterior3")
WANTS = (("ls", "noise"), ("ls",), ("noise",))


def _edge_cases():
    rng = np.random.default_rng(20261019)
    n_cases = 30

    def spread(values):
        reps = -(-n_cases // len(values))
        return [values[i] for i in rng.permutation(np.tile(np.arange(len(values)), reps))[:n_cases]]

    cols = dict(k=spread(EDGE_K), d=spread(EDGE_D), kernel=spread(KERNELS), metric=spread(("l2", "F2")), aniso=spread((False, True)),
                noise=spread(("scalar", "table", "batch")), bi=spread((True, False)), dtype=spread(("float32", "float64")),
                form=spread(FORMS), want=spread(WANTS))
    cases = [{name: vals[i] for name, vals in cols.items()} for i in range(n_cases)]
    # ... and the combinations at which the kernel takes a path of its own, which a sample of single factors need not
    # hit: either block size next to the switch in both widths with per-feature scales, and the per-feature sums over
    # two feature chunks (one of them narrower than the group of eight features a pass sums)
    for j, (k, d, dtype) in enumerate([(126, 8, "float32"), (127, 8, "float32"), (126, 3, "float64"), (127, 3, "float64"),
                                       (33, 70, "float32"), (33, 70, "float64")]):
        base = dict(cases[j])
        base.update(k=k, d=d, dtype=dtype, aniso=True, kernel="matern15", want=("ls", "noise"))
        cases.append(base)
    for c in cases:
        if c["kernel"] in ("matern15", "matern25", "maternInf"):
            c["metric"] = "l2"
    return cases


EDGE_CASES = _edge_cases()


def _edge_id(c):
    return (f"k{c['k']}-d{c['d']}-{c['kernel']}-{c['metric']}-{'aniso' if c['aniso'] else 'iso'}-{c['noise']}"
            f"-{'bi' if c['bi'] else 'nobi'}-{c['form']}-{'+'.join(c['want'])}-{c['dtype']}")


# (that the sample below holds every value of every factor is asserted on the CPU: tests/test_large_backward_status_cpu.py)
@pytest.mark.parametrize("c", EDGE_CASES, ids=[_edge_id(c) for c in EDGE_CASES])
def test_block_and_tile_edges(c):
    rng = np.random.default_rng(sum(map(ord, _edge_id(c))))
    k, d, dtype, b, n = c["k"], c["d"], c["dtype"], 5, 300
    gm, gv, gyk, R = cotangents(rng, c["form"], b)
    X, Y = make_table(rng, n, d, R)
    ni = neighbourhoods(rng, n, b, k)
    bi = rng.choice(n, size=b, replace=False) if c["bi"] else np.arange(b)
    ls = length_scales(rng, d, c["aniso"])
    table = NUGGET * (1.0 + rng.uniform(size=n))
    t = TORCH[dtype]
    if c["noise"] == "scalar":
        rows, noise = np.full((b, k), NUGGET), NUGGET
    elif c["noise"] == "table":
        rows, noise = table[ni], to_dev(table, t)
    else:
        rows, noise = table[ni], to_dev(table[ni], t)
    ref = reference_partials(orc.Spec(c["kernel"], c["metric"], ls, 0.0), X, bi, ni, Y, rows, gm, gv, gyk)
    g_l, g_n, info = entry(dtype, to_dev(X, t), to_dev(bi) if c["bi"] else None, to_dev(ni), to_dev(Y, t), noise, c["kernel"],
                           c["metric"], ls, gm, gv, gyk, want=c["want"])
    assert info == 0
    assert (g_l is None) == ("ls" not in c["want"]) and (g_n is None) == ("noise" not in c["want"])
    check_partials((g_l, g_n), ref, dtype, _edge_id(c))


# ---- 2. the range that did not exist -----------------------------------------------------------------------------------
# Value and gradient against the fp64 reference alone: reference_outputs gives mean / var / ykinvy, the loss's
# cotangents are formed from them in fp64, reference_partials contracts them, and the sums over the batch are compared
# through assert_close in the gradient band (the value in the forward's, tests/util.RTOL).
def reference_loocv(loss, ospec, X, bi, ni, Y, scale=("analytic", 1), sigma_noise=None):
    """(value, d / d length scale(s) (ls_count,), d / d noise) of a LOOCV loss in fp64, as fused.loocv_value_and_grad
    defines it: sigma^2 from ``scale``, evaluated at ``sigma_noise`` when that is given (the trial / stored split)."""
    b, k = ni.shape
    y = Y[bi, 0]
    rows = np.full((b, k), float(ospec.noise))
    m, v, yk = (x.reshape(b) for x in reference_outputs(ospec, X, bi, ni, Y, rows))
    rows_s = rows if sigma_noise is None else np.full((b, k), float(sigma_noise))
    cy = yk.sum() if sigma_noise is None else reference_outputs(ospec, X, bi, ni, Y, rows_s)[2].sum()
    if scale[0] == "analytic":
        s = f0 = cy / (b * k)
        ds = 1.0
        for _ in range(1, int(scale[1])):
            s, ds = 0.5 * (s + f0 / s), 0.5 * (ds + 1.0 / s - f0 * ds / (s * s))
    else:
        s, ds = float(scale[1]), 0.0
    r = m - y
    gv, dL_ds = np.zeros(b), 0.0
    if loss == "lool":
        value, gm, gv = (r * r / v).sum() / s + np.log(v).sum() + b * np.log(s), 2.0 * r / (s * v), 1.0 / v - r * r / (s * v * v)
        dL_ds = b / s - (r * r / v).sum() / (s * s)
    elif loss == "mse":
        value, gm = (r * r).sum() / b, 2.0 * r / b
    elif loss == "pseudo_huber":
        delta = 1.5
        value, gm = delta**2 * (np.sqrt(1.0 + (r / delta) ** 2) - 1.0).sum(), r / np.sqrt(1.0 + (r / delta) ** 2)
    else:  # looph
        delta = 3.0
        g = np.sqrt(1.0 + r * r / (delta**2 * s * v))
        value = (2.0 * delta**2 * (g - 1.0) + np.log(s * v)).sum()
        gm, gv = 2.0 * r / (g * s * v), 1.0 / v - r * r / (g * s * v * v)
        dL_ds = b / s - (r * r / (g * v)).sum() / (s * s)
    gyk = np.full(b, dL_ds * ds / (b * k))
    if sigma_noise is None:
        p_ls, p_n = reference_partials(ospec, X, bi, ni, Y, rows, gm, gv, gyk)
    else:  # the cotangent of y^T K^-1 y goes back at the stored noise and does not reach the trial noise's gradient
        p_ls, p_n = reference_partials(ospec, X, bi, ni, Y, rows, gm, gv, np.zeros(b))
        p_ls = p_ls + reference_partials(ospec, X, bi, ni, Y, rows_s, np.zeros(b), np.zeros(b), gyk)[0]
    return value, p_ls.sum(0), p_n.sum()


def check_value_and_gradient(got, ref, dtype, what):
    (value, g_ls, g_noise), (r_value, r_ls, r_noise) = got, ref
    print(f"{what}: value {value!r} against {r_value!r}; d / d length scale {np.asarray(g_ls)!r} against {r_ls!r}; "
          f"d / d noise {g_noise!r} against {r_noise!r}")
    assert_close([value], [r_value], RTOL[dtype], f"{what}: value")
    assert_close(g_ls, r_ls, GRAD_RTOL[dtype], f"{what}: d / d length scale")
    assert_close([g_noise], [r_noise], GRAD_RTOL[dtype], f"{what}: d / d noise")


RANGE_CASES = [("float32", "limit+1", 8, True), ("float64", "limit+1", 8, False), ("float32", 300, 8, False),
               ("float64", 520, 6, True), ("float32", 1022, 4, False)]


def _range_problem(dtype, k, b, aniso):
    k = limit(dtype) + 1 if k == "limit+1" else k
    rng = np.random.default_rng(k)
    n, d = 1500, 8
    X, Y = make_table(rng, n, d)
    ni, bi = neighbourhoods(rng, n, b, k), rng.choice(n, size=b, replace=False)
    return X, Y, bi, ni, length_scales(rng, d, aniso)


@pytest.mark.parametrize("dtype, k, b, aniso", RANGE_CASES, ids=[f"{c[0]}-k{c[1]}-{'aniso' if c[3] else 'iso'}" for c in RANGE_CASES])
def test_loocv_gradient_beyond_the_lds_backward(dtype, k, b, aniso):
    from muygpys_amd import _lib, fused

    X, Y, bi, ni, ls = _range_problem(dtype, k, b, aniso)
    t = TORCH[dtype]
    spec = fused.KernelSpec("matern15", "l2", list(ls) if aniso else ls, NUGGET)
    got = fused.loocv_value_and_grad(spec, to_dev(X, t), to_dev(Y[:, 0], t), to_dev(bi), to_dev(ni), loss="lool")
    assert _lib.last_kernel().startswith("mgp::hyper_backward_large_kernel<")
    check_value_and_gradient(got, reference_loocv("lool", orc.Spec("matern15", "l2", ls, NUGGET), X, bi, ni, Y), dtype, "lool")


# the four losses, sigma^2 analytic / iterated / fixed, and the trial / stored noise split (two forward and two backward
# launches), at the first nn_count the LDS backward refuses
LOSS_CASES = [("mse", ("analytic", 1), None), ("pseudo_huber", ("analytic", 1), None), ("looph", ("analytic", 3), None),
              ("lool", ("fixed", 0.7), None), ("lool", ("analytic", 3), None), ("lool", ("analytic", 1), 5e-2),
              ("looph", ("analytic", 1), 5e-2), ("mse", ("analytic", 1), 5e-2)]


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("loss, scale, sigma_noise", LOSS_CASES, ids=[f"{c[0]}-{c[1][0]}{c[1][1]}-{'split' if c[2] else 'one'}" for c in LOSS_CASES])
def test_every_loss_and_scale_beyond_the_lds_backward(loss, scale, sigma_noise, dtype):
    from muygpys_amd import _lib, fused

    X, Y, bi, ni, ls = _range_problem(dtype, "limit+1", 8, True)
    t = TORCH[dtype]
    got = fused.loocv_value_and_grad(fused.KernelSpec("matern15", "l2", list(ls), NUGGET), to_dev(X, t), to_dev(Y[:, 0], t), to_dev(bi),
                                     to_dev(ni), loss=loss, scale=scale, sigma_noise=sigma_noise)
    assert _lib.last_kernel().startswith("mgp::hyper_backward_large_kernel<")
    ref = reference_loocv(loss, orc.Spec("matern15", "l2", ls, NUGGET), X, bi, ni, Y, scale, sigma_noise)
    check_value_and_gradient(got, ref, dtype, f"{loss}, sigma^2 {scale}, sigma_noise {sigma_noise}")


@pytest.mark.parametrize("dtype, k, b", [("float32", "limit+1", 8), ("float64", "limit+1", 8), ("float32", 300, 8), ("float64", 520, 6)])
def test_classification_gradient_beyond_the_lds_backward(dtype, k, b):
    from muygpys_amd import _lib, fused

    k = limit(dtype) + 1 if k == "limit+1" else k
    rng = np.random.default_rng(k + 3)
    n, d, R = 1500, 8, 3
    X = rng.uniform(size=(n, d))
    labels = np.eye(R)[(np.floor(3.0 * X[:, :2].sum(1)) % R).astype(int)]  # one-hot, a function of the position
    ni, bi = neighbourhoods(rng, n, b, k), rng.choice(n, size=b, replace=False)
    t, rows = TORCH[dtype], np.full((b, k), NUGGET)
    ospec, spec = orc.Spec("matern15", "l2", LS, NUGGET), fused.KernelSpec("matern15", "l2", LS, NUGGET)
    got = fused.class_value_and_grad(spec, to_dev(X, t), to_dev(labels, t), to_dev(bi), to_dev(ni), loss="mse")
    assert _lib.last_kernel().startswith("mgp::hyper_backward_large_kernel<")
    r = reference_outputs(ospec, X, bi, ni, labels, rows)[0] - labels[bi]
    p_ls, p_n = reference_partials(ospec, X, bi, ni, labels, rows, 2.0 * r / (b * R), None, None)
    check_value_and_gradient(got, ((r * r).sum() / (b * R), p_ls.sum(0), p_n.sum()), dtype, "classification mse")


def _functor_problem(seed, n, b, k, d, planted):
    """An objective with a real optimum: true nearest neighbours in the planted metric (tests/test_gpu_analytic_gradient.py)."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d))
    y = np.sin((X / planted) @ rng.normal(size=d) / np.sqrt(d)) + 0.05 * rng.normal(size=n)
    bi = rng.choice(n, size=b, replace=False)
    d2 = (((X / planted)[bi, None, :] - (X / planted)[None, :, :]) ** 2).sum(-1)
    d2[np.arange(b), bi] = np.inf
    return X, y, bi, np.argsort(d2, axis=1)[:, :k]


def _matern15_model(ls0, noise=1e-2):
    from muygpys_amd.gp import MuyGPS
    from muygpys_amd.gp.deformation import Isotropy, l2
    from muygpys_amd.gp.hyperparameter import AnalyticScale, Parameter
    from muygpys_amd.gp.kernels import Matern
    from muygpys_amd.gp.noise import HomoscedasticNoise

    return MuyGPS(kernel=Matern(smoothness=Parameter(1.5), deformation=Isotropy(l2, Parameter(float(ls0), (0.2, 20.0)))),
                  noise=HomoscedasticNoise(noise), scale=AnalyticScale())


def test_gradient_is_the_central_difference_of_the_functor_layers_objective():
    """fp64 at the first nn_count the LDS backward refuses: rtol = 2e-6, atol = 2e-7 max |fd|, as
    tests/test_gpu_analytic_gradient.py."""
    from muygpys_amd._src.optimize.chassis.hip import _analytic_value_and_grad
    from muygpys_amd.optimize import L_BFGS_B_optimize
    from muygpys_amd.optimize.loss import lool_fn

    k, d = limit("float64") + 1, 4
    X, y, bi, ni = _functor_problem(31, 1500, 64, k, d, np.full(d, 1.2))
    m = _matern15_model(1.4)
    Xd, yd = to_dev(X, torch.float64), to_dev(y, torch.float64)
    cross, pair, y_b, y_nn = m.make_train_tensors(to_dev(bi), to_dev(ni), Xd, yd)
    obj = L_BFGS_B_optimize.make_obj_fn(m, y_b, y_nn, cross, pair, loss_fn=lool_fn)
    names, x0, _ = m.get_opt_params()
    value, grad = _analytic_value_and_grad(m, obj, names)(np.asarray(x0, dtype=np.float64))
    f = lambda x: -float(obj(**{n_: float(v) for n_, v in zip(names, x)}))  # noqa: E731  (the minimised function)
    np.testing.assert_allclose(value, f(x0), rtol=1e-10)
    h = 1e-5 * max(1.0, abs(x0[0]))
    fd = np.array([(f([x0[0] + h]) - f([x0[0] - h])) / (2 * h)])
    print(f"analytic {grad!r} against central difference {fd!r}")
    np.testing.assert_allclose(grad, fd, rtol=2e-6, atol=2e-7 * np.abs(fd).max())


# ---- 3. agreement where both serve -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, k", [("float32", 20), ("float64", 20), ("float32", 70), ("float64", 70), ("float32", 120)])
def test_agrees_with_the_lds_backward(dtype, k):
    from muygpys_amd import _lib

    rng = np.random.default_rng(k)
    n, d, b = 1500, 8, 16
    X, Y = make_table(rng, n, d)
    ni, bi = neighbourhoods(rng, n, b, k), rng.choice(n, size=b, replace=False)
    gm, gv, gyk, _ = cotangents(rng, "loocv", b)
    t, P = TORCH[dtype], _lib.ptr
    Xd, Yd, bi_d, ni_d = to_dev(X, t), to_dev(Y, t), to_dev(bi), to_dev(ni)
    ls_d = to_dev(np.array([LS]), t)
    cot = [to_dev(g, t) for g in (gm, gv, gyk)]
    o_l, o_n = torch.zeros((b, 1), device="cuda", dtype=t), torch.zeros((b, k), device="cuda", dtype=t)
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = _lib.fn("loocv_backward", t)(P(Xd), d, P(bi_d), P(ni_d), b, k, P(Yd), 0, NUGGET, None, 2, 0, P(ls_d), 1,
                                      *[P(g) for g in cot], P(o_l), P(o_n), P(info), _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    g_l, g_n, bad = entry(dtype, Xd, bi_d, ni_d, Yd, NUGGET, "matern15", "l2", LS, gm, gv, gyk)
    assert bad == 0 and int(info.item()) == 0
    check_partials((g_l, g_n), (o_l.double().cpu().numpy(), o_n.double().cpu().numpy()), dtype, f"large vs LDS backward, k = {k}")


# ---- 4. placement invariance, bitwise ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_placement_invariance_bitwise(dtype):
    from muygpys_amd import _lib

    rng = np.random.default_rng(300)
    n, d, k, b = 1200, 8, 300, 9
    X, Y = make_table(rng, n, d)
    ni, bi = neighbourhoods(rng, n, b, k), rng.choice(n, size=b, replace=False)
    ls = length_scales(rng, d, True)
    gm, gv, gyk, _ = cotangents(rng, "loocv", b)
    t = TORCH[dtype]
    Xd, Yd = to_dev(X, t), to_dev(Y, t)
    slab = _lib.load().mgp_backward_large_workspace_bytes(Xd.element_size(), k, 1)

    def run(rows, slabs=None):
        """The neighbourhoods `rows`, on a workspace of `slabs` slabs (None: the recommended size) filled with 0xFF."""
        rows = np.asarray(rows)
        size = _lib.load().mgp_backward_large_workspace_bytes(Xd.element_size(), k, len(rows)) if slabs is None else slabs * slab
        ws = torch.empty(size, dtype=torch.uint8, device="cuda")
        ws.fill_(0xFF)  # (what the slab held before must not matter: NaN in every element, either width)
        g_l, g_n, info = entry(dtype, Xd, to_dev(bi[rows]), to_dev(ni[rows]), Yd, NUGGET, "matern15", "l2", ls, gm[rows], gv[rows],
                               gyk[rows], workspace=ws)
        assert info == 0
        return g_l.cpu().numpy(), g_n.cpu().numpy()

    alone = run([0])
    assert np.isfinite(alone[0]).all() and np.isfinite(alone[1]).all()
    for name, got, pos in (("first of 9", run([0, 1, 2, 3, 4, 5, 6, 7, 8]), 0), ("last of 9", run([1, 2, 3, 4, 5, 6, 7, 8, 0]), 8),
                           ("one slab", run([3, 4, 0, 5, 6], 1), 2), ("recommended", run([3, 4, 0, 5, 6]), 2)):
        for a, g, what in zip(alone, got, ("grad_ls", "grad_noise")):
            assert a[0].tobytes() == g[pos].tobytes(), (name, what, a[0], g[pos])


# ---- 5. failure semantics ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_singular_neighbourhoods_are_counted_and_left_untouched(dtype):
    rng = np.random.default_rng(6)
    n, d, k, b = 1000, 8, 200, 8
    X, Y = make_table(rng, n, d)
    ni, bi = neighbourhoods(rng, n, b, k), rng.choice(n, size=b, replace=False)
    broken = np.array([2, 7])
    ni[broken, 1] = ni[broken, 0]  # a duplicated neighbour ...
    noise = np.full((b, k), NUGGET)
    noise[broken] = 0.0            # ... and no nugget: exactly singular
    good = np.setdiff1d(np.arange(b), broken)
    gm, gv, gyk, _ = cotangents(rng, "loocv", b)
    ref = reference_partials(orc.Spec("matern15", "l2", LS, 0.0), X, bi[good], ni[good], Y, noise[good], gm[good], gv[good], gyk[good])
    t, sentinel = TORCH[dtype], -777.0
    g_l, g_n, info = entry(dtype, to_dev(X, t), to_dev(bi), to_dev(ni), to_dev(Y, t), to_dev(noise, t), "matern15", "l2", LS,
                           gm, gv, gyk, sentinel=sentinel)
    assert info == 2
    assert (g_l[to_dev(broken)] == sentinel).all() and (g_n[to_dev(broken)] == sentinel).all()
    check_partials((g_l[to_dev(good)], g_n[to_dev(good)]), ref, dtype, "the six good neighbourhoods")


# ---- 6. the driver -----------------------------------------------------------------------------------------------------
def test_lbfgsb_with_analytic_gradients_beyond_the_lds_backward(monkeypatch):
    """Isotropic Matern-3/2 with a free length scale, fp64, nn_count = limit + 5, scipy's default stopping rules: the
    analytic and the finite-difference driver reach the same optimum (1e-4 relative), the analytic one in fewer fused
    forward launches, the calls tests/test_gpu_analytic_gradient.py counts.  "Fewer library calls" in all cannot hold
    for a one-parameter model: a forward and a backward launch replace two forward launches."""
    from muygpys_amd import fused as F
    from muygpys_amd.optimize import L_BFGS_B_optimize

    k, d = limit("float64") + 5, 4
    X, y, bi, ni = _functor_problem(4, 3000, 100, k, d, np.full(d, 1.1))
    Xd, yd = to_dev(X, torch.float64), to_dev(y, torch.float64)
    calls = {"fwd": 0, "bwd": 0}

    def counted(fn, key):
        return lambda *a, **kw: (calls.__setitem__(key, calls[key] + 1), fn(*a, **kw))[1]

    for name, key in (("posterior_mean_var", "fwd"), ("loocv_partials", "fwd"), ("_hyper_partials", "bwd")):
        monkeypatch.setattr(F, name, counted(getattr(F, name), key))
    results = {}
    for analytic in (False, True):
        m = _matern15_model(2.0, 1e-3)
        cross, pair, y_b, y_nn = m.make_train_tensors(to_dev(bi), to_dev(ni), Xd, yd)
        calls.update(fwd=0, bwd=0)
        new = L_BFGS_B_optimize(m, y_b, y_nn, cross, pair, analytic_gradient=analytic)
        results[analytic] = (float(new.kernel.deformation.length_scale()), dict(calls))
    (ls_fd, n_fd), (ls_an, n_an) = results[False], results[True]
    print(f"length scale {ls_an!r} in {n_an} launches (analytic) against {ls_fd!r} in {n_fd} launches (finite differences)")
    np.testing.assert_allclose(ls_an, ls_fd, rtol=1e-4)
    assert n_fd["bwd"] == 0 and n_an["bwd"] == n_an["fwd"]
    assert 0 < n_an["fwd"] < n_fd["fwd"], (n_an, n_fd)
    assert 0.2 < ls_an < 20.0 and abs(ls_an - 2.0) > 0.1  # (inside the bounds, away from the start)


def test_beyond_the_limit_is_an_error_that_names_it():
    from muygpys_amd.optimize import L_BFGS_B_optimize

    rng = np.random.default_rng(1023)
    n, d, k, b = 1100, 4, 1023, 2
    X, Y = make_table(rng, n, d)
    Xd, yd = to_dev(X, torch.float32), to_dev(Y[:, 0], torch.float32)
    m = _matern15_model(LS)
    cross, pair, y_b, y_nn = m.make_train_tensors(to_dev(np.arange(b)), to_dev(neighbourhoods(rng, n, b, k)), Xd, yd)
    with pytest.raises(ValueError, match="mgp_large_max_nn_count"):
        L_BFGS_B_optimize(m, y_b, y_nn, cross, pair, analytic_gradient=True)
