"""Classification on the GPU against the reference's fixtures (tests/golden/classify, make_golden_classify.py) and
the numpy oracle (tests/classify_oracle.py): the cross-entropy of the hip loss family, the sums and cotangent of
``mgp_class_sums_*``, the objective through the functor layer (one fused launch + one sums launch), the analytic
gradient (``fused.class_value_and_grad`` = ``oracle.posterior_vjp`` fed with the oracle's cotangent), L-BFGS-B with it,
the label partition (integer-exact), ``classify_any`` / ``classify_two_class_uq`` / ``train_two_class_interval`` /
``make_masks`` / ``do_uq``, and a two-rank sharded cross-entropy."""

import glob
import json
import os

import numpy as np
import pytest

from tests import classify_oracle as O
from tests.util import RTOL, assert_close, to_dev

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a ROCm device")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "classify")
NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
DTYPES = ["float64", "float32"]


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    g = {k: z[k] for k in z.files}
    g["meta"] = json.loads(str(g["meta"]))
    return g


def model(meta, noise_bounds=None, length_scale=None):
    from muygpys_amd.gp import MuyGPS
    from muygpys_amd.gp.deformation import Anisotropy, Isotropy, l2
    from muygpys_amd.gp.hyperparameter import FixedScale, Parameter, VectorParameter
    from muygpys_amd.gp.kernels import Matern
    from muygpys_amd.gp.noise import HomoscedasticNoise

    ls = meta["length_scale"] if length_scale is None else length_scale
    if meta["aniso"]:
        dfm = Anisotropy(l2, length_scale=VectorParameter(*[Parameter(float(v), (0.2, 20.0)) for v in ls]))
    else:
        dfm = Isotropy(l2, length_scale=Parameter(float(ls), (0.2, 20.0)))
    noise = HomoscedasticNoise(meta["noise"]) if noise_bounds is None else HomoscedasticNoise(meta["noise"], noise_bounds)
    return MuyGPS(kernel=Matern(smoothness=Parameter(1.5), deformation=dfm), noise=noise, scale=FixedScale())


def oracle_spec(meta):
    from oracle.muygps_oracle import Spec

    ls = np.asarray(meta["length_scale"], dtype=np.float64) if meta["aniso"] else float(meta["length_scale"])
    return Spec(kernel="matern15", metric="l2", length_scale=ls, noise=float(meta["noise"]))


def _scalar(x):
    return np.atleast_1d(np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float64))


# ---- the loss family -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_cross_entropy_matches_the_reference(name, dtype):
    """(On the parent commit this raises NotImplementedError.)"""
    from muygpys_amd._src.optimize import loss as L

    g = load(name)
    td = getattr(torch, dtype)
    mean, y = to_dev(g["mean"], td), to_dev(g["labels"][g["batch_indices"]], td)
    got = L._cross_entropy_fn(mean, y)
    assert got.ndim == 0 and got.dtype == td and got.is_cuda
    print(f"{name} {dtype}: cross-entropy {float(got):.10g} reference {float(g['cross_entropy']):.10g}")
    assert_close(_scalar(got), _scalar(g["cross_entropy"]), RTOL[dtype], "cross-entropy")
    again = L._cross_entropy_fn(mean, y)
    assert got.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()  # equal inputs, equal bits
    # the public catalogue entry is the same function
    from muygpys_amd.optimize.loss import cross_entropy_fn

    assert float(cross_entropy_fn(mean, y)) == float(got)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_entropy_clips_like_log_loss(dtype):
    from muygpys_amd._src.optimize import loss as L

    td, nd = getattr(torch, dtype), np.dtype(dtype)
    pred = np.array([[60.0, -60.0], [-60.0, 60.0], [0.3, -0.2], [60.0, -60.0]])
    target = np.array([[-1.0, 1.0], [-1.0, 1.0], [1.0, -1.0], [1.0, -1.0]])
    ref = O.cross_entropy(pred, target, nd)
    assert ref < 60.0  # (unclipped: 120.47)
    got = L._cross_entropy_fn(to_dev(pred, td), to_dev(target, td))
    assert_close(_scalar(got), _scalar(ref), RTOL[dtype], "clipped rows, two classes")
    pred3 = np.array([[60.0, 0.0, -60.0], [1.0, 2.0, 0.5], [-60.0, 0.0, 60.0], [0.0, 0.0, 0.0]])
    target3 = np.array([[0.0, 0, 1], [0, 1, 0], [0, 1, 0], [1, 0, 0]])
    got3 = L._cross_entropy_fn(to_dev(pred3, td), to_dev(target3, td))
    assert_close(_scalar(got3), _scalar(O.cross_entropy(pred3, target3, nd)), RTOL[dtype], "clipped rows, three classes")
    # the cotangent of a clipped entry is zero
    p = to_dev(pred, td).requires_grad_(True)
    L._cross_entropy_fn(p, to_dev(target, td)).backward()
    assert_close(p.grad.cpu().numpy(), O.cross_entropy_grad(pred, target, nd), 3 * RTOL[dtype], "cotangent with clipped rows")
    assert torch.all(p.grad[[0, 1, 3]] == 0)


def test_fewer_than_two_labels_still_raise():
    from muygpys_amd._src.optimize import loss as L

    for shape in ((7,), (7, 1)):
        x = torch.zeros(shape, device="cuda", dtype=torch.float64)
        with pytest.raises(NotImplementedError, match="two or more labels"):
            L._cross_entropy_fn(x, x)
        with pytest.raises(NotImplementedError, match="two or more labels"):
            L._cross_entropy_fn(x.clone().requires_grad_(True), x)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_class_sums_and_cotangent(name, dtype):
    from muygpys_amd import _lib
    from muygpys_amd._src.optimize import loss as L

    g = load(name)
    td, nd = getattr(torch, dtype), np.dtype(dtype)
    bi = g["batch_indices"]
    mean_h = g["mean"].astype(nd).astype(np.float64)  # the inputs as the kernel sees them
    y_h = g["labels"][bi]
    mean, y = to_dev(g["mean"], td), to_dev(y_h, td)
    R = mean.shape[1]
    sums, grad = _lib.class_sums(mean, y, R * mean.element_size(), None, "cross_entropy", 1.0, True)
    ref = O.class_sums(mean_h, y_h, nd)
    s = sums.cpu().numpy()
    assert s[2] == ref[2] and s[3] == ref[3] and s[4] == ref[4], (s, ref)  # counts and argmax agreements: exact
    for j, what in ((0, "cross-entropy"), (1, "sum r^2"), (5, "pseudo-Huber")):
        np.testing.assert_allclose(s[j], ref[j], rtol=1e-12, err_msg=what)  # fp64 sums of the same inputs
    assert_close(grad.cpu().numpy(), O.cross_entropy_grad(mean_h, y_h, nd), 3 * RTOL[dtype] if dtype == "float32" else RTOL[dtype],
                 "cotangent")
    # the label table + batch indices form (row stride in bytes) reads the same targets: equal bits
    table, bid = to_dev(g["labels"], td), to_dev(bi)
    sums_t, grad_t = _lib.class_sums(mean, table, R * table.element_size(), bid, "cross_entropy", 1.0, True)
    assert torch.equal(sums_t, sums) and torch.equal(grad_t, grad)
    # mse cotangent
    _, gm = _lib.class_sums(mean, y, R * mean.element_size(), None, "mse", 1.0 / mean.numel(), True)
    assert_close(gm.cpu().numpy(), O.mse_grad(mean_h, y_h), 3 * RTOL[dtype] if dtype == "float32" else RTOL[dtype], "mse cotangent")
    # torch.autograd of the same formula written in torch ops, against the Function's backward
    eps = float(np.finfo(nd).eps)
    a = mean.detach().double().requires_grad_(True)
    pr = torch.softmax(a, dim=1)
    (-(torch.where(y.double() > 0, 1.0, 0.0) * torch.log(torch.clamp(pr, eps, 1 - eps))).sum()).backward()
    h = mean.detach().clone().requires_grad_(True)
    L._cross_entropy_fn(h, y).backward()
    assert_close(h.grad.cpu().numpy(), a.grad.cpu().numpy(), 3 * RTOL[dtype] if dtype == "float32" else RTOL[dtype],
                 "autograd of the torch formula")


def test_class_sums_shape_limits():
    from muygpys_amd import _lib

    x = torch.zeros((4, 63), device="cuda", dtype=torch.float32)
    with pytest.raises(NotImplementedError):
        _lib.class_sums(x, x, 63 * 4, None)
    big = torch.randn((70001, 62), device="cuda", dtype=torch.float32)  # more rows than one pass of the grid
    t = torch.where(torch.randn_like(big) > 1.0, 1.0, -1.0)
    sums, _ = _lib.class_sums(big, t, 62 * 4, None)
    ref = O.class_sums(big.cpu().numpy(), t.cpu().numpy(), np.float32)
    np.testing.assert_allclose(sums.cpu().numpy(), ref, rtol=1e-10)
    empty = torch.zeros((0, 3), device="cuda", dtype=torch.float64)
    assert torch.all(_lib.class_sums(empty, empty, 24, None)[0] == 0)


# ---- the objective through the functor layer -------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_objective_probes_match_the_reference_in_two_launches(name, dtype, monkeypatch):
    from muygpys_amd import _lib
    from muygpys_amd import fused as F
    from muygpys_amd.optimize import Bayes_optimize, L_BFGS_B_optimize
    from muygpys_amd.optimize.loss import cross_entropy_fn, mse_fn

    g = load(name)
    meta, td = g["meta"], getattr(torch, dtype)
    m = model(meta)
    X, Y = to_dev(g["features"], td), to_dev(g["labels"], td)
    cross, pair, y_b, y_nn = m.make_train_tensors(to_dev(g["batch_indices"]), to_dev(g["batch_nn_indices"]), X, Y)
    calls = {"fused": 0, "sums": 0}
    real_post, real_sums = F.posterior_mean_var, _lib.class_sums
    monkeypatch.setattr(F, "posterior_mean_var", lambda *a, **kw: (calls.__setitem__("fused", calls["fused"] + 1), real_post(*a, **kw))[1])
    monkeypatch.setattr(_lib, "class_sums", lambda *a, **kw: (calls.__setitem__("sums", calls["sums"] + 1), real_sums(*a, **kw))[1])
    for driver in (L_BFGS_B_optimize, Bayes_optimize):  # the two drivers build the same objective
        obj = driver.make_obj_fn(m, y_b, y_nn, cross, pair, loss_fn=cross_entropy_fn)
        for probe, ref in zip(meta["probes"], g["probe_cross_entropy"]):
            calls.update(fused=0, sums=0)
            got = obj(**probe)
            assert calls == {"fused": 1, "sums": 1}, calls  # one fused posterior launch, one mgp_class_sums launch
            print(f"{name} {dtype}: objective {float(got):.10g} reference {float(ref):.10g}")
            assert_close(_scalar(got), _scalar(ref), RTOL[dtype], f"cross-entropy objective at {probe}")
    obj = L_BFGS_B_optimize.make_obj_fn(m, y_b, y_nn, cross, pair, loss_fn=mse_fn)
    for probe, ref in zip(meta["probes"], g["probe_mse"]):
        assert_close(_scalar(obj(**probe)), _scalar(ref), RTOL[dtype], f"mse objective at {probe}")


# ---- analytic gradients ----------------------------------------------------------------------------------------------


def _oracle_value_and_grad(g, loss, nd):
    import oracle.muygps_oracle as orc

    spec = oracle_spec(g["meta"])
    X, Y, bi, ni = g["features"], g["labels"], g["batch_indices"], g["batch_nn_indices"]
    mean, _ = orc.posterior_mean_var(spec, X, X, bi, ni, Y)
    t = Y[bi]
    if loss == "cross_entropy":
        value, gm = O.cross_entropy(mean, t, nd), O.cross_entropy_grad(mean, t, nd)
    else:
        value, gm = O.mse(mean, t), O.mse_grad(mean, t)
    vjp = orc.posterior_vjp(spec, X, X, bi, ni, Y, gm, np.zeros(len(bi)))
    return value, np.atleast_1d(vjp["length_scale"]), float(vjp["noise"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("loss", ["cross_entropy", "mse"])
@pytest.mark.parametrize("name", ["c2_pm1_iso_k12", "c2_01_iso_k30", "c3_pm1_aniso_k12", "c10_pm1_iso_k30", "c10_pm1_aniso_k12"])
def test_class_value_and_grad_is_the_oracle_vjp(name, loss, dtype):
    """Isotropy and Anisotropy; the noise derivative is that of a free homoscedastic noise."""
    from muygpys_amd import fused as F

    g = load(name)
    meta, td, nd = g["meta"], getattr(torch, dtype), np.dtype(dtype)
    ls = torch.tensor(meta["length_scale"], dtype=td, device="cuda") if meta["aniso"] else float(meta["length_scale"])
    spec = F.KernelSpec("matern15", "l2", ls, float(meta["noise"]))
    value, g_ls, g_noise = F.class_value_and_grad(spec, to_dev(g["features"], td), to_dev(g["labels"], td),
                                                  to_dev(g["batch_indices"]), to_dev(g["batch_nn_indices"]), loss=loss)
    ref_value, ref_ls, ref_noise = _oracle_value_and_grad(g, loss, nd)
    rtol = RTOL[dtype] if dtype == "float64" else 3 * RTOL[dtype]
    print(f"{name} {loss} {dtype}: value {value:.10g} / {ref_value:.10g}; d/dls {g_ls} / {ref_ls}; d/dnoise {g_noise:.8g} / {ref_noise:.8g}")
    assert_close(_scalar(value), _scalar(ref_value), rtol, "value")
    assert_close(g_ls, ref_ls, rtol, "d / d length_scale")
    assert_close(_scalar(g_noise), _scalar(ref_noise), rtol, "d / d noise")


@pytest.mark.parametrize("loss", ["cross_entropy", "mse"])
@pytest.mark.parametrize("name", ["c2_pm1_iso_k12", "c10_pm1_aniso_k12"])
def test_chassis_differentiates_classification_objectives(name, loss):
    """``_analytic_value_and_grad`` accepts cross_entropy_fn and routes mse_fn on several columns to the same path:
    the value is the objective's own, the gradient the oracle's -- with the noise among the free parameters."""
    from muygpys_amd._src.optimize.chassis.hip import _analytic_value_and_grad
    from muygpys_amd.optimize import L_BFGS_B_optimize
    from muygpys_amd.optimize import loss as L

    g = load(name)
    m = model(g["meta"], noise_bounds=(1e-5, 1e-1))
    td = torch.float64
    X, Y = to_dev(g["features"], td), to_dev(g["labels"], td)
    cross, pair, y_b, y_nn = m.make_train_tensors(to_dev(g["batch_indices"]), to_dev(g["batch_nn_indices"]), X, Y)
    obj = L_BFGS_B_optimize.make_obj_fn(m, y_b, y_nn, cross, pair, loss_fn=getattr(L, loss + "_fn"))
    names, x0, _ = m.get_opt_params()
    assert "noise" in names
    value, grad = _analytic_value_and_grad(m, obj, names)(np.asarray(x0, dtype=np.float64))
    np.testing.assert_allclose(value, -float(obj(**{n: float(v) for n, v in zip(names, x0)})), rtol=1e-10)
    ref_value, ref_ls, ref_noise = _oracle_value_and_grad(g, loss, np.float64)
    assert_close(_scalar(value), _scalar(ref_value), RTOL["float64"], "value")
    assert_close(grad, np.concatenate([ref_ls, [ref_noise]]), RTOL["float64"], "gradient")


def test_analytic_route_still_refuses_what_it_refused():
    from muygpys_amd.optimize import L_BFGS_B_optimize
    from muygpys_amd.optimize.loss import cross_entropy_fn

    g = load("c2_pm1_iso_k12")
    m = model(g["meta"])
    X, Y = to_dev(g["features"], torch.float64), to_dev(g["labels"], torch.float64)
    bi, ni = to_dev(g["batch_indices"]), to_dev(g["batch_nn_indices"])
    cross, pair, y_b, y_nn = m.make_train_tensors(bi, ni, X, Y)
    with pytest.raises(ValueError, match="no target mask"):
        L_BFGS_B_optimize(m, y_b, y_nn, cross, pair, loss_fn=cross_entropy_fn, target_mask=[0], analytic_gradient=True)
    with pytest.raises(ValueError, match="loss_kwargs"):
        L_BFGS_B_optimize(m, y_b, y_nn, cross, pair, loss_fn=cross_entropy_fn, loss_kwargs={"boundary_scale": 2.0},
                          analytic_gradient=True)
    cross, pair, y_b, y_nn = m.make_train_tensors(bi, ni, X, Y, materialize=True)
    with pytest.raises(ValueError, match="lazy training tensors"):
        L_BFGS_B_optimize(model(g["meta"]), y_b, y_nn, cross, pair, loss_fn=cross_entropy_fn, analytic_gradient=True)


@pytest.mark.parametrize("name", ["c10_pm1_iso_k30", "c3_pm1_aniso_k12"])
def test_lbfgsb_on_cross_entropy_reaches_the_finite_difference_optimum_in_fewer_evaluations(name, monkeypatch):
    """Same comparison and tolerance as tests/test_gpu_analytic_gradient.py: both drivers to the same optimum (1e-4
    relative on every length scale), the analytic one in fewer objective evaluations (fused forward launches)."""
    from muygpys_amd import fused as F
    from muygpys_amd.optimize import L_BFGS_B_optimize
    from muygpys_amd.optimize.loss import cross_entropy_fn

    g = load(name)
    meta, td = g["meta"], torch.float64
    X, Y = to_dev(g["features"], td), to_dev(g["labels"], td)
    bi, ni = to_dev(g["batch_indices"]), to_dev(g["batch_nn_indices"])
    launches = {"fwd": 0}
    real_post = F.posterior_mean_var
    monkeypatch.setattr(F, "posterior_mean_var", lambda *a, **kw: (launches.__setitem__("fwd", launches["fwd"] + 1), real_post(*a, **kw))[1])
    results = {}
    for analytic in (False, True):
        m = model(meta)
        cross, pair, y_b, y_nn = m.make_train_tensors(bi, ni, X, Y)
        launches["fwd"] = 0
        new = L_BFGS_B_optimize(m, y_b, y_nn, cross, pair, loss_fn=cross_entropy_fn, analytic_gradient=analytic,
                                options={"ftol": 1e-14, "gtol": 1e-9})
        ls = new.kernel.deformation.length_scale()
        results[analytic] = (np.array([float(v) for v in ls] if meta["aniso"] else [float(ls)]), launches["fwd"])
    ls_fd, n_fd = results[False]
    ls_an, n_an = results[True]
    print(f"{name}: finite differences {ls_fd} in {n_fd} evaluations, analytic {ls_an} in {n_an}")
    np.testing.assert_allclose(ls_an, ls_fd, rtol=1e-4)
    assert 0 < n_an < n_fd, (n_an, n_fd)


# ---- the partition ---------------------------------------------------------------------------------------------------


def _check_partition(labels_h, nn_h, td):
    from muygpys_amd import _lib

    labels, nn = to_dev(labels_h, td), to_dev(nn_h)
    pred, flags, count, sel, nn_sel = _lib.class_partition(labels, nn)
    first, nonconstant, sel_ref, nn_sel_ref = O.partition(labels_h, nn_h)
    m = int(count.item())
    assert m == len(sel_ref)
    assert np.array_equal(flags.cpu().numpy(), nonconstant)
    assert np.array_equal(sel[:m].cpu().numpy(), sel_ref) and np.array_equal(nn_sel[:m].cpu().numpy(), nn_sel_ref)
    assert np.array_equal(pred.cpu().numpy(), first.astype(pred.cpu().numpy().dtype))
    return m


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_partition_matches_the_oracle_on_the_fixtures(name, dtype):
    g = load(name)
    m = _check_partition(g["labels"], g["test_nn_indices"], getattr(torch, dtype))
    assert m == int(g["nonconstant"].sum())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b,k,R", [(1, 3, 2), (255, 12, 3), (1000, 30, 10), (262145, 5, 2), (300007, 7, 3)])
def test_partition_on_ragged_sizes(b, k, R, dtype):
    """b not a multiple of the workgroup size, fewer rows than one workgroup, and more than 1024 workgroups' worth
    (chunks of several tiles)."""
    rng = np.random.default_rng(b)
    n = 5000
    ids = rng.integers(0, R, size=n)
    labels = -np.ones((n, R))
    labels[np.arange(n), ids] = 1.0
    # neighbourhoods drawn from one class with probability 1/2: both kinds of rows everywhere
    nn = rng.integers(0, n, size=(b, k))
    same = np.where(ids == 0)[0]
    rows = rng.random(b) < 0.5
    nn[rows] = same[rng.integers(0, len(same), size=(int(rows.sum()), k))]
    _check_partition(labels, nn, getattr(torch, dtype))


def test_partition_with_no_and_with_only_nonconstant_rows():
    n, b, k = 600, 777, 9
    rng = np.random.default_rng(3)
    nn = rng.integers(0, n, size=(b, k))
    labels = np.tile(np.array([[1.0, -1.0]]), (n, 1))
    assert _check_partition(labels, nn, torch.float64) == 0  # m = 0
    nn[:, 0], nn[:, 1] = 0, 1
    labels[1] = [-1.0, 1.0]
    assert _check_partition(labels, nn, torch.float32) == b  # m = b


def test_empty_batches_are_served():
    from muygpys_amd import _lib

    labels = torch.tensor([[1.0, -1.0], [-1.0, 1.0]], device="cuda", dtype=torch.float64)
    pred, flags, count, sel, nn_sel = _lib.class_partition(labels, torch.zeros((0, 4), device="cuda", dtype=torch.int64))
    assert int(count.item()) == 0 and pred.shape == (0, 2) and flags.shape == (0,) and nn_sel.shape == (0, 4)
    dst, var = torch.ones((3, 2), device="cuda", dtype=torch.float64), torch.ones(3, device="cuda", dtype=torch.float64)
    _lib.class_scatter(pred, var[:0], sel, dst, var)  # m = 0: nothing moves
    assert torch.all(dst == 1) and torch.all(var == 1)


# ---- prediction ------------------------------------------------------------------------------------------------------


class FixtureLookup:
    """The neighbour lists the reference's own lookup returned (stored in the fixture), behind NN_Wrapper's query."""

    def __init__(self, indices):
        self.indices = indices

    def get_nns(self, test):
        return self.indices, None


def _count_fused_rows(monkeypatch):
    from muygpys_amd import fused as F

    rows = []
    real = F.posterior_mean_var

    def spy(spec, fq, fn, bi, ni, *a, **kw):
        rows.append(int(ni.shape[0]))
        return real(spec, fq, fn, bi, ni, *a, **kw)

    monkeypatch.setattr(F, "posterior_mean_var", spy)
    return rows


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_classify_any_matches_the_reference(name, dtype, monkeypatch):
    from muygpys_amd.examples.classify import classify_any

    g = load(name)
    meta, td = g["meta"], getattr(torch, dtype)
    rows = _count_fused_rows(monkeypatch)
    X, Y, Xt = to_dev(g["features"], td), to_dev(g["labels"], td), to_dev(g["test_features"], td)
    pred, timing = classify_any(model(meta), Xt, X, FixtureLookup(to_dev(g["test_nn_indices"])), Y)
    assert set(timing) == {"nn", "agree", "pred"}
    nc = g["nonconstant"]
    assert rows == [int(nc.sum())], (rows, int(nc.sum()), len(nc))  # the fused kernel ran on m rows, not b
    got = pred.cpu().numpy()
    assert np.array_equal(got[~nc], g["predictions"][~nc])  # constant rows: exact
    assert_close(got[nc], g["predictions"][nc], RTOL[dtype], "solved rows")
    ties = O.near_ties(g["predictions"], RTOL[dtype])
    assert ties.mean() <= 0.01
    assert np.array_equal(got.argmax(1)[~ties], g["predictions"].argmax(1)[~ties])  # predicted labels


@pytest.mark.parametrize("dtype", DTYPES)
def test_classify_two_class_uq_matches_the_reference(dtype, monkeypatch):
    from muygpys_amd.examples.classify import classify_two_class_uq

    g = load("c2_pm1_iso_k12")
    meta, td = g["meta"], getattr(torch, dtype)
    rows = _count_fused_rows(monkeypatch)
    X, Y, Xt = to_dev(g["features"], td), to_dev(g["labels"], td), to_dev(g["test_features"], td)
    means, variances, _ = classify_two_class_uq(model(meta), Xt, X, FixtureLookup(to_dev(g["test_nn_indices"])), Y)
    nc = g["nonconstant"]
    assert rows == [int(nc.sum())]
    mh, vh = means.cpu().numpy(), variances.cpu().numpy()
    assert np.array_equal(mh[~nc], g["uq_means"][~nc]) and np.all(vh[~nc] == 0.0)  # constant rows: exact, variance 0
    assert_close(mh[nc], g["uq_means"][nc], RTOL[dtype], "solved means")
    assert_close(vh[nc], g["uq_variances"][nc], RTOL[dtype], "solved variances")


def test_classify_any_with_the_device_lookup():
    """End to end with the package's own NN_Wrapper: whatever neighbours it returns, constant rows carry their nearest
    neighbour's label exactly and the others are the fused posterior of exactly those neighbourhoods."""
    from muygpys_amd import fused as F
    from muygpys_amd.examples.classify import classify_any
    from muygpys_amd.neighbors import NN_Wrapper

    g = load("c10_pm1_iso_k30")
    meta, td = g["meta"], torch.float32
    X, Y, Xt = to_dev(g["features"], td), to_dev(g["labels"], td), to_dev(g["test_features"], td)
    nbrs = NN_Wrapper(X, meta["k"])
    pred, _ = classify_any(model(meta), Xt, X, nbrs, Y)
    nn = nbrs.get_nns(Xt)[0]
    first, nc, sel, nn_sel = O.partition(g["labels"], nn.cpu().numpy())
    got = pred.cpu().numpy()
    assert np.array_equal(got[~nc], first[~nc].astype(np.float32)) and 0 < nc.sum() < len(nc)
    spec = F.KernelSpec("matern15", "l2", float(meta["length_scale"]), float(meta["noise"]))
    mean, _ = F.posterior_mean_var(spec, Xt, X, to_dev(sel), to_dev(nn_sel), Y)
    assert_close(got[nc], mean.cpu().numpy(), RTOL["float32"], "solved rows")


def test_two_class_interval_masks_and_uq():
    from muygpys_amd.examples import classify as Cl

    g = load("c2_pm1_iso_k12")
    td = torch.float64
    m = model(g["meta"])
    X, Y = to_dev(g["features"], td), to_dev(g["labels"], td)
    bi, bni = to_dev(g["batch_indices"]), to_dev(g["batch_nn_indices"])
    signed = to_dev(2 * g["class_ids"] - 1)
    cutoffs = Cl.train_two_class_interval(m, bi, bni, X, Y, signed, Cl.example_lambdas)
    step = float(g["cutv"][1] - g["cutv"][0])
    print("cutoffs", cutoffs.cpu().numpy(), "reference", g["cutoffs"])
    assert np.all(np.abs(cutoffs.cpu().numpy() - g["cutoffs"]) <= step * (1 + 1e-9))
    mean, var = Cl._regress_from_indices(m, bi, bni, X, X, Y, True)
    assert_close(mean.cpu().numpy(), g["mean"], RTOL["float64"], "batch means")
    assert_close(var.cpu().numpy(), g["batch_variance"], RTOL["float64"], "batch variances")
    correct = (2 * torch.argmax(mean, dim=1) - 1) == signed[bi]
    assert np.array_equal(correct.cpu().numpy(), g["correct_mask"])
    alpha, beta = Cl.interval_curves(mean, var, correct, to_dev(g["cutv"], td))
    n_wrong, n_right = int((~g["correct_mask"]).sum()), int(g["correct_mask"].sum())
    assert np.abs(alpha.cpu().numpy() - g["alpha"]).max() <= 1.0 / n_wrong + 1e-12
    assert np.abs(beta.cpu().numpy() - g["beta"]).max() <= 1.0 / n_right + 1e-12
    # make_masks / do_uq: exact given the fixture's means
    masks = Cl.make_masks(to_dev(g["uq_means"], td), to_dev(g["cutoffs"], td), to_dev(g["uq_variances"], td), 0.0)
    assert np.array_equal(masks.cpu().numpy(), g["masks"])
    accuracy, uq = Cl.do_uq(to_dev(g["uq_means"], td), to_dev(g["test_labels"], td), masks)
    np.testing.assert_allclose(accuracy, float(g["uq_accuracy"]), rtol=1e-14)
    np.testing.assert_allclose(uq.cpu().numpy(), g["uq"], rtol=1e-14, atol=0)


# ---- sharded ---------------------------------------------------------------------------------------------------------


def _shard_rank(rank, world, port, q):
    """One of two processes sharing cuda:0: its half of the batch, the cross-entropy all-reduced."""
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from muygpys_amd import distributed as D
        from muygpys_amd._src.optimize import loss as L

        g = load("c10_pm1_iso_k30")
        rows = np.array_split(np.arange(len(g["batch_indices"])), world)[rank]
        mean = to_dev(g["mean"][rows], torch.float64)
        y = to_dev(g["labels"][g["batch_indices"]][rows], torch.float64)
        with D.sharded_reductions():
            total = float(L._cross_entropy_fn(mean, y))
        q.put((rank, total, float(L._cross_entropy_fn(mean, y))))
    finally:
        dist.destroy_process_group()


def test_two_shards_all_reduce_to_the_single_rank_cross_entropy():
    import socket

    import torch.multiprocessing as mp

    from muygpys_amd._src.optimize import loss as L

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_shard_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=600) for _ in procs)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    g = load("c10_pm1_iso_k30")
    single = float(L._cross_entropy_fn(to_dev(g["mean"], torch.float64), to_dev(g["labels"][g["batch_indices"]], torch.float64)))
    assert got[0][1] == got[1][1], "every rank must hold the same global sum"
    np.testing.assert_allclose(got[0][1], single, rtol=1e-12)
    np.testing.assert_allclose(got[0][2] + got[1][2], single, rtol=1e-12)  # (the local sums are the shards' own)
    np.testing.assert_allclose(single, g["cross_entropy"], rtol=1e-8)


# ---- resources -------------------------------------------------------------------------------------------------------


def test_new_kernels_spill_nothing():
    from muygpys_amd import build

    res = json.load(open(os.path.join(build.LIBDIR, "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if "3mgp" in k and "class_" in k}
    assert len(mine) >= 9, sorted(mine)
    for name, r in mine.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (name, r)
