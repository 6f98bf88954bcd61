"""GPU: the fast-posterior-mean workflow of the general-smoothness Matern on the fused kernels (``fused.gen_fast("fused")``):
``mgp_fast_coefficients_gen_*`` (the GEN x COEFFS instantiations of the LDS and slab workgroup kernels) and
``mgp_fast_posterior_mean_gen_*`` (fast_mean_gen_kernel / fast_mean_wide_gen_kernel, csrc/mgp_fast_mean.hip) and the
Python layers above them, against numpy fp64: ``oracle.muygps_oracle`` with ``matern_gen_fn`` (scipy ``kv``),
``np.linalg.solve`` and ``np.einsum``.

Case lists and problems: tests/fast_gen_cases.py.  tests/test_fast_gen_cpu.py proves their coverage, and that the fp32
evaluator's own error moves none of the fp32 cases by more than a quarter of the band asserted here."""

import numpy as np
import pytest

from oracle import muygps_oracle as orc
from tests import fast_gen_cases as G
from tests.util import RTOL, assert_close, to_dev

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def TD(dtype):
    return getattr(torch, dtype)


def ES(dtype):
    return 4 if dtype == "float32" else 8


def lds_limit(dtype, R):
    from muygpys_amd import _lib

    return _lib.load().mgp_max_nn_count_gen(ES(dtype), R)


def gen_kernel_spec(nu, ls, noise=0.0):
    from muygpys_amd.fused import KernelSpec

    return KernelSpec("matern_gen", "l2", ls, noise, smoothness=nu)


def predict(c, problem, nu=None):
    from muygpys_amd import fused

    X, Q, ni, bi, co, crow, ls = problem
    t = TD(c["dtype"])
    with fused.gen_fast("fused"):
        got = fused.fast_posterior_mean(gen_kernel_spec(c["nu"] if nu is None else nu, ls), to_dev(Q, t), to_dev(X, t),
                                        None if bi is None else to_dev(bi), to_dev(ni),
                                        to_dev(co if c["R"] > 1 else co[:, :, 0], t), to_dev(crow))
    torch.cuda.synchronize()
    return got.cpu().numpy().reshape(ni.shape[0], c["R"])


# ---- 1. prediction edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.prediction_cases(), ids=G.prediction_id)
def test_prediction_kernel_edges(c):
    from muygpys_amd import _lib

    problem = G.prediction_problem(c)
    ref = G.prediction_reference(c, problem)
    got = predict(c, problem)
    want = "fast_mean_wide_gen_kernel" if c["k"] + 1 > 64 else "fast_mean_gen_kernel"
    assert want in _lib.last_kernel(), _lib.last_kernel()
    print(f"max abs err {np.abs(got - ref).max():.3e}, rms(ref) {np.sqrt((ref ** 2).mean()):.3e}")
    assert np.isfinite(got).all()
    assert_close(got, ref, G.BAND[c["dtype"]], "fast posterior mean")


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_beyond_nu_30_is_refused_and_the_lazy_layer_steps_aside(dtype):
    from muygpys_amd import fused, lazy, lazy_eval

    c = dict(k=40, d=8, dtype=dtype, nu=30.5, aniso=False, R=3, batch_idx=True, zero=False)
    problem = G.prediction_problem(c)
    with pytest.raises(fused.FusedUnsupported):
        predict(c, problem)
    X, Q, ni, bi, co, crow, ls = problem
    t = TD(dtype)
    Xd, Qd, nid, bid, cod, crowd = to_dev(X, t), to_dev(Q, t), to_dev(ni), to_dev(bi), to_dev(co, t), to_dev(crow)

    def handle(nu):
        m = model(nu, ls, 0.0)
        Kcross = m.kernel(m.kernel.deformation.crosswise_tensor(Qd, Xd, bid, nid, lazy=True))
        assert isinstance(Kcross, lazy.LazyCov) and Kcross.kernel == "matern_gen" and Kcross.smoothness == nu
        return Kcross

    with fused.gen_fast("fused"):
        assert lazy_eval.fast_mean(handle(30.5), cod, rows=crowd) is None
        out = lazy_eval.fast_mean(handle(2.2), cod, rows=crowd)  # (the same handle below the limit is served)
    assert out is not None and tuple(out.shape) == (37, 3)
    assert lazy_eval.fast_mean(handle(2.2), cod, rows=crowd) is None  # (outside the block: as before)


# ---- 2. a test point's bits do not depend on its wave-mates ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("k", [30, 12, 100])
def test_bits_do_not_depend_on_the_batch_around_a_point(k, dtype):
    """Every other test point is pulled to within 1e-4 of its nearest neighbour: partners in a wave (k = 30, 12: two
    points per wave) need very different node counts.  Alone, in the batch and in the reversed batch: equal bits."""
    from muygpys_amd import fused

    rng = np.random.default_rng(31 * k)
    n, b, d, R, nu = 500, 37, 8, 3, 1.3
    X, Q = rng.uniform(size=(n, d)), rng.uniform(size=(b, d))
    ni = G.neighbourhoods(rng, n, b, k)
    for t in range(0, b, 2):
        near = ni[t, np.argmin(((X[ni[t]] - Q[t]) ** 2).sum(1))]
        step = rng.normal(size=d)
        Q[t] = X[near] + 1e-4 * rng.uniform() * step / np.linalg.norm(step)
    co, crow = rng.normal(size=(41, k, R)), rng.permutation(41)[:b]
    t_ = TD(dtype)
    Xd, Qd, nid, cod, crowd = to_dev(X, t_), to_dev(Q, t_), to_dev(ni), to_dev(co, t_), to_dev(crow)
    spec = gen_kernel_spec(nu, G.length_scale(d))
    order = torch.arange(b, device="cuda")
    with fused.gen_fast("fused"):
        batch = fused.fast_posterior_mean(spec, Qd, Xd, order, nid, cod, crowd)
        rev = order.flip(0)
        reversed_ = fused.fast_posterior_mean(spec, Qd, Xd, rev.contiguous(), nid[rev].contiguous(), cod, crowd[rev].contiguous())
        alone = torch.cat([fused.fast_posterior_mean(spec, Qd, Xd, order[i:i + 1], nid[i:i + 1], cod, crowd[i:i + 1]) for i in range(b)])
    torch.cuda.synchronize()
    assert torch.isfinite(batch).all()
    assert torch.equal(alone, batch), "alone against in the batch"
    assert torch.equal(reversed_.flip(0), batch), "the reversed batch"


# ---- 3. coefficient edges -----------------------------------------------------------------------------------------------
def coefficients(c, problem, **kw):
    from muygpys_amd import fused

    X, Y, ni, ls, noise, rows = problem
    t = TD(c["dtype"])
    nz = to_dev(noise, t) if isinstance(noise, np.ndarray) else noise
    spec = gen_kernel_spec(c["nu"], ls, nz)
    Xd = to_dev(X, t)
    with fused.gen_fast("fused"):
        inp = fused._normalize(spec, Xd, Xd, None, to_dev(ni), to_dev(Y, t))
        out = fused._fused_coefficients(spec, inp)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("c", G.coefficient_cases(), ids=G.coefficient_id)
def test_coefficient_edges(c):
    from muygpys_amd import _lib

    k = G.resolve_k(c, lds_limit)
    problem = G.coefficient_problem(c, k)
    ref = G.coefficient_reference(c, problem)
    got = coefficients(c, problem)
    assert got is not None
    family = "fused_generic_gen_coeffs_kernel" if k <= lds_limit(c["dtype"], c["R"]) else "fused_large_gen_coeffs_kernel"
    assert family in _lib.last_kernel(), (_lib.last_kernel(), family)
    got = got.cpu().numpy()
    print(f"k = {k}: max abs err {np.abs(got - ref).max():.3e}, rms(ref) {np.sqrt((ref ** 2).mean()):.3e}")
    assert_close(got, ref, G.BAND[c["dtype"]], "coefficients")


def test_through_fast_coefficients_with_the_self_including_lists():
    """``fused.fast_coefficients`` itself (fast_nn_update in front), one response, squeezed."""
    from muygpys_amd import fused

    rng = np.random.default_rng(12)
    n, d, k, nu = 300, 8, 70, 2.2
    X, Y = G.make_table(rng, n, d)
    nn = np.stack([rng.choice(np.delete(np.arange(n), i), size=k, replace=False) for i in range(n)])
    nn_fast = orc.fast_nn_update(nn)
    c = dict(nu=nu, aniso=False)
    ref = G.coefficient_reference(c, (X, Y, nn_fast, G.length_scale(d), G.NUGGET, np.full(nn_fast.shape, G.NUGGET)))[:, :, 0]
    for dtype in ("float32", "float64"):
        t = TD(dtype)
        with fused.gen_fast("fused"):
            co, nn_d = fused.fast_coefficients(gen_kernel_spec(nu, G.length_scale(d), G.NUGGET), to_dev(X, t), to_dev(Y[:, 0], t), to_dev(nn))
        torch.cuda.synchronize()
        assert np.array_equal(nn_d.cpu().numpy(), nn_fast) and tuple(co.shape) == (n, k)
        assert_close(co.cpu().numpy(), ref, G.BAND[dtype], "coefficients")


# ---- 4. placement ---------------------------------------------------------------------------------------------------------
def call_gen(dtype, X, Y, ni, ls, nu, workspace="recommended"):
    """One ``mgp_fast_coefficients_gen_*`` call through ``_lib`` directly -> (coeffs (b, k, R), workspace bytes)."""
    from muygpys_amd import _lib, fused

    t = TD(dtype)
    spec = gen_kernel_spec(nu, ls, G.NUGGET)
    Xd = to_dev(X, t)
    inp = fused._normalize(spec, Xd, Xd, None, to_dev(ni), to_dev(Y, t))
    size = _lib.load().mgp_fast_coefficients_gen_workspace_bytes(ES(dtype), inp.k, inp.R, 1 if workspace == "one slab" else inp.b)
    ws = torch.empty(size, dtype=torch.uint8, device="cuda") if size else None
    out = torch.full((inp.b, inp.k, inp.R), float("nan"), device="cuda", dtype=t)
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    P = _lib.ptr
    rc = _lib.fn("fast_coefficients_gen", t)(P(inp.fn), inp.d, P(inp.ni), inp.b, inp.k, P(inp.tg), inp.R, inp.mode, inp.eps, P(inp.nz),
                                             float(nu), spec.metric_id(), P(inp.ls), inp.ls.numel(), P(out), P(info), P(ws), size,
                                             _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert int(info.item()) == 0
    return out, size


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("k", [40, 100, 300])
def test_coefficients_do_not_depend_on_workspace_or_place(dtype, k):
    rng = np.random.default_rng(77 + k)
    n, d, R, b, nu = 400, 8, 3, 24, 1.3
    X, Y = G.make_table(rng, n, d, R)
    ni = G.neighbourhoods(rng, n, b, k)
    ls = G.length_scale(d)
    full, size = call_gen(dtype, X, Y, ni, ls, nu)
    assert (size > 0) == (k > lds_limit(dtype, R))
    if size:
        one, slab = call_gen(dtype, X, Y, ni, ls, nu, workspace="one slab")
        assert 0 < slab < size and torch.equal(one, full), "a workspace of exactly one slab"
    perm = np.random.default_rng(1).permutation(b)
    moved, _ = call_gen(dtype, X, Y, ni[perm], ls, nu)
    assert torch.equal(moved, full[to_dev(perm)]), "a neighbourhood at another place in the batch"
    alone, _ = call_gen(dtype, X, Y, ni[3:4], ls, nu)
    assert torch.equal(alone[0], full[3]), "a neighbourhood in a batch of its own"


# ---- 5. which kernels ran: asserted by name in tests 1 and 3 above; the exact names once more here ----------------------------
def test_kernel_names():
    from muygpys_amd import _lib

    seen = {}
    for dtype, T in (("float32", "float"), ("float64", "double")):
        for k in (30, 60, 100):
            c = dict(k=k, d=8, dtype=dtype, nu=1.0, aniso=False, R=1, batch_idx=True, zero=False)
            predict(c, G.prediction_problem(c))
            seen[(dtype, k)] = _lib.last_kernel()
        assert seen[(dtype, 30)] == f"mgp::fast_mean_gen_kernel<{T}, 32>"
        assert seen[(dtype, 60)] == f"mgp::fast_mean_gen_kernel<{T}, 64>"
        assert seen[(dtype, 100)] == f"mgp::fast_mean_wide_gen_kernel<{T}>"
        L = lds_limit(dtype, 1)
        for k, name in ((L, f"mgp::fused_generic_gen_coeffs_kernel<{T}>"), (L + 1, f"mgp::fused_large_gen_coeffs_kernel<{T}>")):
            c = dict(k=k, d=8, dtype=dtype, nu=1.0, R=1, aniso=False, noise="scalar", b=4, n=400)
            assert coefficients(c, G.coefficient_problem(c, k)) is not None
            assert _lib.last_kernel() == name


# ---- 6. agreement with the closed form at nu = 3/2 ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("k", [30, 100])
def test_agrees_with_the_closed_form_at_three_halves(k, dtype):
    """The new entries and the ``matern15`` entries on the same inputs, within the project's band of the dtype: RTOL in
    fp64 (the evaluator's error is 6e-13), 3e-3 in fp32 (the same fp32 solve on the same inputs; the fp32 evaluator moves
    such results by at most a quarter of that band, tests/test_fast_gen_cpu.py)."""
    from muygpys_amd import fused

    c = dict(k=k, d=8, dtype=dtype, nu=1.5, R=3, aniso=False, noise="scalar", b=24, n=400, batch_idx=True, zero=False)
    tol = G.BAND[dtype]
    assert G.BAND["float64"] == RTOL["float64"]
    t = TD(dtype)
    X, Y, ni, ls, noise, _ = G.coefficient_problem(c, k)
    gen = coefficients(c, (X, Y, ni, ls, noise, None))
    Xd = to_dev(X, t)
    closed_spec = fused.KernelSpec("matern15", "l2", ls, noise)
    closed = fused._fused_coefficients(closed_spec, fused._normalize(closed_spec, Xd, Xd, None, to_dev(ni), to_dev(Y, t)))
    torch.cuda.synchronize()
    assert_close(gen.cpu().numpy(), closed.cpu().numpy(), tol, "coefficients")
    X, Q, ni, bi, co, crow, ls = problem = G.prediction_problem(c)
    got = predict(c, problem)
    ref = fused.fast_posterior_mean(fused.KernelSpec("matern15", "l2", ls, 0.0), to_dev(Q, t), to_dev(X, t), to_dev(bi), to_dev(ni),
                                    to_dev(co, t), to_dev(crow))
    torch.cuda.synchronize()
    assert_close(got, ref.cpu().numpy(), tol, "fast posterior mean")


# ---- 7. the workflow --------------------------------------------------------------------------------------------------------
def oracle_fast(X, y, Q, k, specs):
    """fast_nn_update, solve, closest neighbour's coefficients x Kcross -- one oracle spec per response column (or one
    for all of them)."""
    from sklearn.neighbors import NearestNeighbors

    nbrs = NearestNeighbors(n_neighbors=k + 1, algorithm="brute").fit(X)
    nn = nbrs.kneighbors(X, return_distance=False)[:, 1:]
    nn_fast = orc.fast_nn_update(nn)
    pd = orc.pairwise_tensor(X, nn_fast)
    test_nn = nbrs.kneighbors(Q, n_neighbors=k, return_distance=False)
    closest = test_nn[:, 0]
    cd = orc.crosswise_tensor(Q, X, np.arange(len(Q)), nn_fast[closest])
    coeffs, means = [], []
    for spec, cols in specs:
        _, Kin = orc.kernel_tensors(spec, pd[:, 0], pd)
        co = orc.fast_posterior_mean_precompute(orc.perturb(spec, Kin, nn_fast), y[nn_fast][..., cols])
        Kc, _ = orc.kernel_tensors(spec, cd, pd[:1])
        coeffs.append(co.reshape(co.shape[0], k, -1))
        means.append(orc.fast_posterior_mean(Kc, co[closest]).reshape(len(Q), -1))
    return (nn, test_nn), np.concatenate(coeffs, -1), np.concatenate(means, -1)


def make_problem(k, seed=17, n=1500, nq=300, d=8, R=3):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d))
    W = rng.normal(size=(d, R)) / np.sqrt(d)
    Y = np.sin(X @ W) + 0.05 * rng.normal(size=(n, R))
    return X, Y, rng.normal(size=(nq, d))


@pytest.fixture(scope="module", params=[30, 100])
def workflow_problem(request):
    k = request.param
    X, Y, Q = make_problem(k)
    return X, Y, Q, k, oracle_fast(X, Y, Q, k, [(G.gen_spec(1.37, 2.5, 1e-2), slice(None))])


def spy_on_library(monkeypatch):
    from muygpys_amd import _lib

    calls, real = [], _lib.fn
    monkeypatch.setattr(_lib, "fn", lambda base, dtype: (calls.append(base), real(base, dtype))[1])
    return calls


def model(nu=1.37, ls=2.5, noise=1e-2):
    from muygpys_amd.gp import MuyGPS
    from muygpys_amd.gp.deformation import Isotropy, l2
    from muygpys_amd.gp.hyperparameter import Parameter
    from muygpys_amd.gp.kernels import Matern
    from muygpys_amd.gp.noise import HomoscedasticNoise

    return MuyGPS(kernel=Matern(smoothness=Parameter(nu), deformation=Isotropy(l2, Parameter(ls))), noise=HomoscedasticNoise(noise))


MATERIALISING = {"solve", "solve_large", "matern_gen", "pairwise_dists", "crosswise_dists"}


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_workflow_is_two_fused_launches(workflow_problem, dtype, monkeypatch):
    from muygpys_amd import fused
    from muygpys_amd.examples.fast_posterior_mean import fast_posterior_mean_any
    from muygpys_amd.neighbors import NN_Wrapper

    X, Y, Q, k, ((nn, test_nn), coeffs_ref, mean_ref) = workflow_problem
    t = TD(dtype)
    Xd, Yd, Qd = to_dev(X, t), to_dev(Y, t), to_dev(Q, t)
    nbrs = NN_Wrapper(Xd, k)
    calls = spy_on_library(monkeypatch)
    with fused.gen_fast("fused"):
        mean, coeffs, timing = fast_posterior_mean_any(model(), Qd, Xd, nbrs, Yd)
    torch.cuda.synchronize()
    assert sorted(timing) == ["agree", "nn", "precompute", "pred"]
    assert calls.count("fast_coefficients_gen") == 1 and calls.count("fast_posterior_mean_gen") == 1, calls
    assert not MATERIALISING & set(calls), calls
    assert coeffs.shape == coeffs_ref.shape and mean.shape == mean_ref.shape
    # (the k-NN front end is the real one: in fp32 it may order two nearly equidistant neighbours the other way round
    # than the fp64 oracle -- compared where both sides solved the same list, as tests/test_gpu_fast_any.py does)
    nn_d = nbrs.get_batch_nns(torch.arange(X.shape[0], device="cuda"))[0].cpu().numpy()
    closest_d = nbrs.get_nns(Qd)[0][:, 0].cpu().numpy()
    same_rows = (nn_d == nn).all(axis=1)
    same_points = (closest_d == test_nn[:, 0]) & same_rows[test_nn[:, 0]]
    if dtype == "float64":
        assert same_rows.all() and same_points.all()
    assert same_rows.mean() >= 0.99 and same_points.mean() >= 0.98
    assert_close(coeffs.cpu().numpy()[same_rows], coeffs_ref[same_rows], G.BAND[dtype], "coefficients")
    assert_close(mean.cpu().numpy()[same_points], mean_ref[same_points], G.BAND[dtype], "fast posterior mean")
    # outside the block: the calls of the materialising route, as before
    calls.clear()
    mean2, coeffs2, _ = fast_posterior_mean_any(model(), Qd, Xd, nbrs, Yd)
    torch.cuda.synchronize()
    assert {"solve", "matern_gen"} <= set(calls), calls
    assert not {"fast_coefficients_gen", "fast_posterior_mean_gen", "fast_coefficients_any", "fast_posterior_mean"} & set(calls), calls
    assert_close(mean2.cpu().numpy()[same_points], mean_ref[same_points], G.BAND[dtype], "fast posterior mean (materialised)")


def test_multivariate_workflow_with_a_smoothness_per_model(monkeypatch):
    from muygpys_amd import fused
    from muygpys_amd.examples.fast_posterior_mean import fast_posterior_mean_any
    from muygpys_amd.neighbors import NN_Wrapper

    k = 40
    X, Y, Q = make_problem(k, seed=23, n=800, nq=100, R=2)
    _, coeffs_ref, mean_ref = oracle_fast(X, Y, Q, k, [(G.gen_spec(0.8, 2.5, 1e-2), slice(0, 1)), (G.gen_spec(2.6, 2.0, 1e-2), slice(1, 2))])

    class Multi:
        models = [model(0.8, 2.5), model(2.6, 2.0)]

    Xd, Yd, Qd = to_dev(X, torch.float64), to_dev(Y, torch.float64), to_dev(Q, torch.float64)
    calls = spy_on_library(monkeypatch)
    with fused.gen_fast("fused"):
        mean, coeffs, _ = fast_posterior_mean_any(Multi(), Qd, Xd, NN_Wrapper(Xd, k), Yd)
    torch.cuda.synchronize()
    assert calls.count("fast_coefficients_gen") == 2 and calls.count("fast_posterior_mean_gen") == 2, calls
    assert not MATERIALISING & set(calls), calls
    assert_close(coeffs.cpu().numpy(), coeffs_ref, G.BAND["float64"], "coefficients")
    assert_close(mean.cpu().numpy(), mean_ref, G.BAND["float64"], "fast posterior mean")
