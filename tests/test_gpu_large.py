"""GPU: local systems beyond LDS (csrc/mgp_large.hip: blocked Cholesky on a slab of global memory, panels of NB = 32)
against a numpy fp64 oracle (oracle.muygps_oracle + np.linalg.solve) -- every block edge at small size through
``path="large"``, the nn_count range nothing served before on ``path="auto"``, agreement with the LDS kernel where
both serve, placement invariance bit for bit, failure semantics, the materialised front end and the functor layer.

Inputs as the fp32 arithmetic allows the project's tolerances (tests/util.py: fp64 1e-5, fp32 1e-3) at these sizes:
uniform [0, 1]^d points, length scale 0.5, nugget 1e-2, responses sin(3 sum x) + 0.1 noise."""

import numpy as np
import pytest
import torch

from oracle import muygps_oracle as orc
from tests.util import RTOL, assert_close, assert_rel_close, to_dev

pytestmark = pytest.mark.gpu

NB = 32  # panel width of the factorisation = side of the fp32 tile (the fp64 tile has 16 rows)
TORCH = {"float32": torch.float32, "float64": torch.float64}
KERNELS = ("rbf", "matern05", "matern15", "matern25", "maternInf")
LS, NUGGET = 0.5, 1e-2


def k0(dtype, R=1):
    """The first nn_count the LDS-resident kernels refuse."""
    from muygpys_amd import _lib

    return _lib.load().mgp_max_nn_count(4 if dtype == "float32" else 8, R) + 1


def make_table(rng, n, d, R=1):
    X = rng.uniform(size=(n, d))
    Y = np.stack([np.sin(3.0 * X.sum(1) + r) + 0.1 * rng.normal(size=n) for r in range(R)], axis=1)
    return X, Y


def neighbourhoods(rng, n, b, k):
    return np.stack([rng.choice(n, size=k, replace=False) for _ in range(b)])


def oracle_outputs(ospec, Xq, Xn, bi, ni, Y, noise_rows=None):
    """mean (b, R), var (b,), ykinvy (b, R) in fp64.  ``noise_rows``: a (b, k) noise diagonal instead of ospec.noise."""
    cd = orc.crosswise_tensor(Xq, Xn, bi, ni)
    pd = orc.pairwise_tensor(Xn, ni)
    Kc, Kin = orc.kernel_tensors(ospec, cd, pd)
    if noise_rows is not None:
        Kin = Kin + np.stack([np.diag(r) for r in noise_rows])
    else:
        Kin = orc.perturb(ospec, Kin, ni)
    Yn = Y[ni]  # (b, k, R)
    A = np.linalg.solve(Kin, np.concatenate([Kc[:, :, None], Yn], axis=2))
    mean = np.einsum("bk,bkr->br", Kc, A[:, :, 1:])
    var = 1.0 - np.einsum("bk,bk->b", Kc, A[:, :, 0])
    yk = np.einsum("bkr,bkr->br", Yn, A[:, :, 1:])
    return mean, var, yk


def check(got, ref, dtype, what):
    (mean, var, yk), (m_ref, v_ref, y_ref) = got, ref
    torch.cuda.synchronize()
    rtol = RTOL[dtype]
    assert_close(mean.cpu().numpy().reshape(m_ref.shape), m_ref, rtol, f"{what}: mean")
    assert_rel_close(var.cpu().numpy(), v_ref, rtol, f"{what}: var")
    assert_rel_close(yk.cpu().numpy().reshape(y_ref.shape), y_ref, rtol, f"{what}: ykinvy")


# ---- 1. block edges at small size --------------------------------------------------------------------------------------
# The factors of the issue -- k in {1, 2, NB-1, NB, NB+1, 2NB+3, 3NB}, R in {1, 3, 16}, d in {1, 3, 8, 40, 70}, the five
# kernels, both metrics, Isotropy / Anisotropy, the three noise modes, gathered / table responses, batch_idx or None, a
# query table of its own -- as a seeded sample in which every value of every factor appears, plus the (k, R) pairs
# that put the row count k + 1 + R on, one below and one above a tile edge (16 rows in fp64, 32 in fp32): the k of the
# list above never land there with these R, so those pairs bring their own k.
# Kernel and metric are paired as far as the pair is a covariance function at all: F2 (the squared distance) goes with
# RBF and Matern-1/2 -- exp(-r^2 / 2 l^2), exp(-r^2 / l^2) -- while (1 + sqrt(3) r^2) exp(-sqrt(3) r^2), its 5/2 sibling and
# exp(-r^4 / 2) are not positive definite (at d = 8 and nn_count = 32 five of 37 such matrices have an eigenvalue below
# -0.05, nugget included); those three kernels take l2.
def _edge_cases():
    rng = np.random.default_rng(20261019)
    n_cases = 30

    def spread(values):
        reps = -(-n_cases // len(values))
        return [values[i] for i in rng.permutation(np.tile(np.arange(len(values)), reps))[:n_cases]]

    cols = dict(k=spread([1, 2, NB - 1, NB, NB + 1, 2 * NB + 3, 3 * NB]), R=spread([1, 3, 16]), d=spread([1, 3, 8, 40, 70]),
                kernel=spread(list(KERNELS)), metric=spread(["l2", "F2"]), aniso=spread([False, True]),
                noise=spread(["scalar", "table", "batch"]), gathered=spread([False, True]), bi=spread([True, False]),
                own_query=spread([False, True]), dtype=spread(["float32", "float64"]))
    cases = [{name: vals[i] for name, vals in cols.items()} for i in range(n_cases)]
    for c in cases:
        if c["kernel"] in ("matern15", "matern25", "maternInf"):
            c["metric"] = "l2"
    # rows = 15, 16, 17 / 31, 32, 33 / 63, 64, 65
    for j, (k, R) in enumerate([(13, 1), (12, 3), (15, 1), (29, 1), (28, 3), (31, 1), (46, 16), (47, 16), (48, 16), (61, 1), (62, 1), (63, 1)]):
        base = dict(cases[j % n_cases])
        base.update(k=k, R=R, dtype=("float32", "float64")[j % 2])
        cases.append(base)
        other = dict(base)
        other.update(dtype=("float64", "float32")[j % 2], kernel="matern15", metric="l2")
        cases.append(other)
    return cases


EDGE_CASES = _edge_cases()


def _edge_id(c):
    return (f"k{c['k']}-R{c['R']}-d{c['d']}-{c['kernel']}-{c['metric']}-{'aniso' if c['aniso'] else 'iso'}-{c['noise']}"
            f"-{'gathered' if c['gathered'] else 'table'}-{'bi' if c['bi'] else 'nobi'}-{'q' if c['own_query'] else 'same'}-{c['dtype']}")


def test_edge_sample_covers_every_factor():
    seen = {name: {c[name] for c in EDGE_CASES} for name in EDGE_CASES[0]}
    assert {1, 2, NB - 1, NB, NB + 1, 2 * NB + 3, 3 * NB} <= seen["k"]
    assert seen["R"] == {1, 3, 16} and {1, 3, 8, 40, 70} <= seen["d"] and seen["kernel"] == set(KERNELS)
    assert seen["metric"] == {"l2", "F2"} and seen["noise"] == {"scalar", "table", "batch"}
    for name in ("aniso", "gathered", "bi", "own_query"):
        assert seen[name] == {False, True}, name
    rows = {(c["k"] + 1 + c["R"], c["dtype"]) for c in EDGE_CASES}
    for dtype in ("float32", "float64"):
        assert {(r, dtype) for r in (15, 16, 17, 31, 32, 33, 63, 64, 65)} <= rows


@pytest.mark.parametrize("c", EDGE_CASES, ids=[_edge_id(c) for c in EDGE_CASES])
def test_block_edges(c):
    from muygpys_amd.fused import KernelSpec, posterior_mean_var

    rng = np.random.default_rng(sum(map(ord, _edge_id(c))))
    k, R, d, dtype, b = c["k"], c["R"], c["d"], c["dtype"], 37
    n, nq = 300, 53
    Xn, Y = make_table(rng, n, d, R)
    Xq = make_table(rng, nq, d)[0] if c["own_query"] else Xn
    ni = neighbourhoods(rng, n, b, k)
    bi = rng.choice(Xq.shape[0], size=b, replace=False) if c["bi"] else np.arange(b)
    ls = LS * (1.0 + 0.3 * rng.uniform(size=d)) if c["aniso"] else LS
    table = NUGGET * (1.0 + rng.uniform(size=n))
    t = TORCH[dtype]
    if c["noise"] == "scalar":
        o_noise, d_noise = NUGGET, NUGGET
    elif c["noise"] == "table":
        o_noise, d_noise = table, to_dev(table, t)
    else:
        o_noise, d_noise = table, to_dev(table[ni], t)
    ref = oracle_outputs(orc.Spec(c["kernel"], c["metric"], ls, o_noise), Xq, Xn, bi, ni, Y)
    Xn_d, Y_d = to_dev(Xn, t), to_dev(Y, t)
    Xq_d = to_dev(Xq, t) if c["own_query"] else Xn_d
    tg = Y_d[to_dev(ni)] if c["gathered"] else Y_d
    spec = KernelSpec(c["kernel"], c["metric"], list(ls) if c["aniso"] else ls, d_noise)
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = posterior_mean_var(spec, Xq_d, Xn_d, to_dev(bi) if c["bi"] else None, to_dev(ni), tg, want_ykinvy=True,
                             info=info, path="large", gathered=c["gathered"])
    check(got, ref, dtype, _edge_id(c))
    assert int(info.item()) == 0


# ---- 2. the range that did not exist -----------------------------------------------------------------------------------
# k0 = the first nn_count the LDS kernels refuse (read from mgp_max_nn_count when the test runs)
RANGE_CASES = [(dtype, k, R, d, b, kernel) for dtype in ("float32", "float64") for k, R, d, b, kernel in (
    ("k0", 1, 8, 8, "matern15"), ("k0+1", 1, 8, 8, "rbf"), (520, 1, 8, 6, "matern25"), (1022, 1, 8, 4, "matern15"),
    (1007, 16, 8, 4, "matern05"))]
RANGE_CASES += [("float32", 300, 3, 40, 8, "maternInf"), ("float64", 200, 3, 40, 8, "maternInf")]


@pytest.mark.parametrize("dtype, k, R, d, b, kernel", RANGE_CASES, ids=[f"{c[0]}-k{c[1]}-R{c[2]}-d{c[3]}-{c[5]}" for c in RANGE_CASES])
def test_nn_counts_beyond_lds(dtype, k, R, d, b, kernel):
    from muygpys_amd import _lib
    from muygpys_amd.fused import KernelSpec, posterior_mean_var

    k = {"k0": k0(dtype), "k0+1": k0(dtype) + 1}.get(k, k)
    rng = np.random.default_rng(k * 7 + R)
    n = 1500
    X, Y = make_table(rng, n, d, R)
    ni = neighbourhoods(rng, n, b, k)
    bi = rng.choice(n, size=b, replace=False)
    metric = "F2" if kernel == "rbf" else "l2"
    ref = oracle_outputs(orc.Spec(kernel, metric, LS, NUGGET), X, X, bi, ni, Y)
    t = TORCH[dtype]
    Xd, Yd = to_dev(X, t), to_dev(Y, t)
    got = posterior_mean_var(KernelSpec(kernel, metric, LS, NUGGET), Xd, Xd, to_dev(bi), to_dev(ni), Yd, want_ykinvy=True)
    assert _lib.last_kernel() == f"mgp::fused_large_kernel<{'float' if dtype == 'float32' else 'double'}>"
    check(got, ref, dtype, f"k = {k}")


# ---- 3. / 4. agreement with the LDS kernel -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("k, R, d, b", [(70, 1, 8, 16), (120, 3, 40, 16), (20, 1, 8, 5000)])
def test_agrees_with_the_generic_kernel(k, R, d, b, dtype):
    from muygpys_amd import _lib
    from muygpys_amd.fused import KernelSpec, posterior_mean_var

    rng = np.random.default_rng(k)
    n = 4000
    X, Y = make_table(rng, n, d, R)
    # (distinct neighbours per row: k of a window of 200 rows, the window placed at random)
    ni = np.argsort(rng.uniform(size=(b, 200)), axis=1)[:, :k] + rng.integers(0, n - 200, size=(b, 1))
    bi = rng.integers(0, n, size=b)
    t = TORCH[dtype]
    spec = KernelSpec("matern15", "l2", LS, NUGGET)
    args = (spec, to_dev(X, t), to_dev(X, t), to_dev(bi), to_dev(ni), to_dev(Y, t))
    large = posterior_mean_var(*args, want_ykinvy=True, path="large")
    assert _lib.last_kernel().startswith("mgp::fused_large_kernel<")
    generic = posterior_mean_var(*args, want_ykinvy=True, path="generic")
    assert _lib.last_kernel().startswith("mgp::fused_generic_kernel<")
    torch.cuda.synchronize()
    check(large, tuple(x.double().cpu().numpy() for x in generic), dtype, f"large vs generic, k = {k}, b = {b}")


# ---- 5. placement invariance, bitwise ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_placement_invariance_bitwise(dtype):
    from muygpys_amd import _lib
    from muygpys_amd.fused import KernelSpec, posterior_mean_var

    rng = np.random.default_rng(300)
    n, d, k, b = 1200, 8, 300, 9
    X, Y = make_table(rng, n, d)
    ni = neighbourhoods(rng, n, b, k)
    bi = rng.choice(n, size=b, replace=False)
    t = TORCH[dtype]
    Xd, Yd, spec = to_dev(X, t), to_dev(Y[:, 0], t), KernelSpec("matern15", "l2", LS, NUGGET)

    def fused(rows):
        out = posterior_mean_var(spec, Xd, Xd, to_dev(bi[rows]), to_dev(ni[rows]), Yd, want_ykinvy=True, path="large")
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in out]

    def direct(rows, slabs):
        """mgp_posterior_large_* itself on a workspace of `slabs` slabs (None: the recommended size)."""
        lib, es = _lib.load(), Xd.element_size()
        m = len(rows)
        size = lib.mgp_large_workspace_bytes(es, k, 1, m) if slabs is None else slabs * lib.mgp_large_workspace_bytes(es, k, 1, 1)
        ws = torch.empty(size, dtype=torch.uint8, device="cuda")
        ws.fill_(0xFF)  # (what the slab held before must not matter: NaN in every element, either width)
        bi_d, ni_d, ls = to_dev(bi[rows]), to_dev(ni[rows]), torch.tensor([LS], device="cuda", dtype=t)
        outs = [torch.empty(m, device="cuda", dtype=t) for _ in range(3)]
        P = _lib.ptr
        rc = _lib.fn("posterior_large", t)(P(Xd), P(Xd), d, P(bi_d), P(ni_d), m, k, P(Yd), 1, 0, 0, NUGGET, None, 2, 0, P(ls), 1,
                                           P(outs[0]), P(outs[1]), P(outs[2]), None, P(ws), size, _lib.stream_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in outs]

    alone = fused([0])
    first = fused([0, 1, 2, 3, 4, 5, 6, 7, 8])
    last = fused([1, 2, 3, 4, 5, 6, 7, 8, 0])
    one_slab = direct([3, 4, 0, 5, 6], 1)
    recommended = direct([3, 4, 0, 5, 6], None)
    for name, got, pos in (("first of 9", first, 0), ("last of 9", last, 8), ("grid of one", one_slab, 2), ("recommended", recommended, 2)):
        for a, g, what in zip(alone, got, ("mean", "var", "ykinvy")):
            assert a.reshape(-1)[0].tobytes() == g.reshape(-1)[pos].tobytes(), (name, what, a.reshape(-1)[0], g.reshape(-1)[pos])
    # ... and the whole batches agree where they share neighbourhoods
    assert first[0].reshape(-1)[1:].tobytes() == last[0].reshape(-1)[:8].tobytes()
    assert one_slab[1].tobytes() == recommended[1].tobytes()


# ---- 6. failure semantics ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_singular_neighbourhoods_are_nan_and_counted(dtype):
    from muygpys_amd.fused import KernelSpec, posterior_mean_var

    rng = np.random.default_rng(6)
    n, d, k, b = 1000, 8, 200, 8
    X, Y = make_table(rng, n, d)
    ni = neighbourhoods(rng, n, b, k)
    bi = rng.choice(n, size=b, replace=False)
    broken = np.array([2, 7])
    ni[broken, 1] = ni[broken, 0]  # a duplicated neighbour ...
    noise = np.full((b, k), NUGGET)
    noise[broken] = 0.0            # ... and no nugget: exactly singular
    good = np.setdiff1d(np.arange(b), broken)
    ref = oracle_outputs(orc.Spec("matern15", "l2", LS, 0.0), X, X, bi[good], ni[good], Y, noise_rows=noise[good])
    t = TORCH[dtype]
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    mean, var, yk = posterior_mean_var(KernelSpec("matern15", "l2", LS, to_dev(noise, t)), to_dev(X, t), to_dev(X, t), to_dev(bi),
                                       to_dev(ni), to_dev(Y[:, 0], t), want_ykinvy=True, info=info)
    torch.cuda.synchronize()
    assert int(info.item()) == 2
    for x in (mean, var, yk):
        assert torch.isnan(x[to_dev(broken)]).all() and torch.isfinite(x[to_dev(good)]).all()
    g = to_dev(good)
    check((mean[g], var[g], yk[g]), ref, dtype, "the six good neighbourhoods")


# ---- 7. materialised systems -------------------------------------------------------------------------------------------
def _spd_systems(rng, b, k, R):
    X = rng.uniform(size=(b, k + 1, 8))
    D = np.sqrt(((X[:, :, None, :] - X[:, None, :, :]) ** 2).sum(-1)) / LS
    K = (1.0 + np.sqrt(3.0) * D) * np.exp(-np.sqrt(3.0) * D)
    Kin = K[:, :k, :k] + NUGGET * np.eye(k)
    Kc = K[:, k, :k]
    Y = np.sin(3.0 * X[:, :k].sum(-1))[:, :, None] + 0.1 * rng.normal(size=(b, k, max(R, 1)))
    return Kin, Kc, Y[:, :, :R]


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("R", [0, 1, 3])
@pytest.mark.parametrize("k", ["k0+1", 520])
def test_materialised_systems(k, R, dtype):
    from muygpys_amd._src.gp.muygps import hip as M

    k = k0(dtype) + 1 if k == "k0+1" else k
    rng = np.random.default_rng(k + R)
    b = 5
    Kin, Kc, Y = _spd_systems(rng, b, k, R)
    t = TORCH[dtype]
    rtol = RTOL[dtype]
    Kin_d, Kc_d = to_dev(Kin, t), to_dev(Kc, t)
    a = np.linalg.solve(Kin, Kc[:, :, None])[:, :, 0]
    v_ref = 1.0 - np.einsum("bk,bk->b", Kc, a)
    if R == 0:
        _, var, _, _ = M._solve(Kin_d, Kc_d, None, want=("var",))
        torch.cuda.synchronize()
        assert_rel_close(var.cpu().numpy(), v_ref, rtol, "var")
        return
    mean, var, yk, co = M._solve(Kin_d, Kc_d, to_dev(Y, t), want=("mean", "var", "ykinvy", "coeffs"))
    torch.cuda.synchronize()
    c_ref = np.linalg.solve(Kin, Y)
    assert_close(mean.cpu().numpy(), np.einsum("bk,bkr->br", Kc, c_ref), rtol, "mean")
    assert_rel_close(var.cpu().numpy(), v_ref, rtol, "var")
    assert_rel_close(yk.cpu().numpy(), np.einsum("bkr,bkr->br", Y, c_ref), rtol, "ykinvy")
    assert_close(co.cpu().numpy(), c_ref, rtol, "coeffs")


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_fast_precompute_beyond_lds(dtype):
    from muygpys_amd._src.gp.muygps import hip as M

    k = k0(dtype) + 1
    rng = np.random.default_rng(k)
    Kin, _, Y = _spd_systems(rng, 4, k, 1)
    t = TORCH[dtype]
    co = M._muygps_fast_posterior_mean_precompute(to_dev(Kin, t), to_dev(Y[:, :, 0], t))
    torch.cuda.synchronize()
    assert_close(co.cpu().numpy(), np.linalg.solve(Kin, Y)[:, :, 0], RTOL[dtype], "coefficients")


# ---- 8. functor layer, end to end --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def functor_problem():
    rng = np.random.default_rng(8)
    n, d = 3000, 8
    X, Y = make_table(rng, n, d)
    return X, Y[:, 0]


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_functor_layer_end_to_end(functor_problem, dtype):
    from muygpys_amd import fused
    from muygpys_amd.gp import MuyGPS
    from muygpys_amd.gp.deformation import Isotropy, l2
    from muygpys_amd.gp.hyperparameter import AnalyticScale, Parameter
    from muygpys_amd.gp.kernels import Matern
    from muygpys_amd.gp.noise import HomoscedasticNoise
    from muygpys_amd.neighbors import NN_Wrapper
    from muygpys_amd.optimize import L_BFGS_B_optimize
    from muygpys_amd.optimize.loss import lool_fn

    X, y = functor_problem
    t = TORCH[dtype]
    rtol = RTOL[dtype]
    k = k0(dtype) + 10
    Xd, yd = to_dev(X, t), to_dev(y, t)
    nbrs = NN_Wrapper(Xd, nn_count=k, nn_method="exact")  # (k > 64: the dense path)
    rng = np.random.default_rng(88)
    bi = np.sort(rng.choice(len(X), size=64, replace=False))
    bi_d = to_dev(bi)
    ni_d, _ = nbrs.get_batch_nns(bi_d)
    ni = ni_d.cpu().numpy()
    assert ni.shape == (64, k)
    m = MuyGPS(kernel=Matern(smoothness=Parameter(1.5), deformation=Isotropy(l2, Parameter(LS, (0.05, 5.0)))),
               noise=HomoscedasticNoise(NUGGET), scale=AnalyticScale())
    ospec = orc.Spec("matern15", "l2", LS, NUGGET)
    m_ref, v_ref, yk_ref = oracle_outputs(ospec, X, X, bi, ni, y[:, None])
    # prediction: the batch rows as test points against the training table
    cross, pair, y_nn = m.make_predict_tensors(bi_d, ni_d, Xd, Xd, yd)
    Kin, Kc = m.kernel(pair), m.kernel(cross)
    mean = m.posterior_mean(Kin, Kc, y_nn)
    assert_close(mean.cpu().numpy().reshape(-1), m_ref[:, 0], rtol, "posterior_mean")
    assert_rel_close(m.get_opt_var_fn()(Kin, Kc).cpu().numpy(), v_ref, rtol, "unscaled variance")
    m = m.optimize_scale(pair, y_nn)
    s_ref = float(np.asarray(orc.sigma_sq(ospec, X, ni, y)).reshape(-1)[0])
    assert_rel_close([float(m.scale())], [s_ref], rtol, "sigma^2")
    assert_rel_close(m.posterior_variance(Kin, Kc).cpu().numpy().reshape(-1), v_ref * s_ref, rtol, "scaled variance")
    # training: the lool objective of make_loo_crossval_fn
    cross, pair, y_b, y_nn = m.make_train_tensors(bi_d, ni_d, Xd, yd)
    obj = L_BFGS_B_optimize.make_obj_fn(m, y_b, y_nn, cross, pair, loss_fn=lool_fn)
    val, ref = float(obj(length_scale=LS)), float(orc.loocv_objective(ospec, X, bi, ni, y, "lool"))
    print(f"lool objective: {val!r} against {ref!r}")
    assert_close([val], [ref], rtol, "lool objective")  # (the project's check of this scalar: test_gpu_distributed.py)
    # the six sums of one LOOCV evaluation
    partials, _, _ = fused.loocv_partials(fused.KernelSpec("matern15", "l2", LS, NUGGET), Xd, yd, bi_d, ni_d)
    torch.cuda.synchronize()
    r = m_ref[:, 0] - y[bi]
    sums = np.array([(r * r / v_ref).sum(), np.log(v_ref).sum(), (r * r).sum(), len(bi),
                     (1.5**2 * (np.sqrt(1.0 + (r / 1.5) ** 2) - 1.0)).sum(), yk_ref.sum()])
    got = partials.cpu().numpy()
    assert got[3] == len(bi)
    # (a sum of b terms each within rtol of its own size: bounded by rtol times the sum of the terms' magnitudes)
    mags = np.array([(r * r / v_ref).sum(), np.abs(np.log(v_ref)).sum(), (r * r).sum(), len(bi), sums[4], yk_ref.sum()])
    print(f"six sums: {got!r} against {sums!r}, magnitudes {mags!r}")
    assert np.all(np.abs(got - sums) <= rtol * mags), (got, sums)


def test_limits_are_errors_that_name_them():
    from muygpys_amd import fused

    rng = np.random.default_rng(1025)
    n, d, k = 1100, 4, 1023
    X = to_dev(rng.uniform(size=(n, d)), torch.float32)
    y = to_dev(rng.normal(size=n), torch.float32)
    ni = to_dev(neighbourhoods(rng, n, 2, k))
    with pytest.raises(ValueError, match="mgp_large_max_nn_count"):
        fused.posterior_mean_var(fused.KernelSpec("matern15", "l2", LS, NUGGET), X, X, to_dev(np.arange(2)), ni, y)
    # the one-launch prepared evaluation stays with the LDS kernels: refused, as before
    k = k0("float32") + 10
    ni = to_dev(neighbourhoods(rng, n, 4, k))
    plan = fused.LoocvPlan("matern15", "l2", X, y, to_dev(np.arange(4)), ni, packed=False)
    with pytest.raises(RuntimeError, match="MGP_EUNSUPPORTED"):
        plan.evaluate(LS, NUGGET)
