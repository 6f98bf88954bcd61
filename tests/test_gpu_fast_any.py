"""GPU: the fast-posterior-mean workflow for any nn_count and response count -- the prediction kernel beyond 64 slots
(csrc/mgp_fast_mean.hip), ``mgp_fast_coefficients_any_*`` on the LDS and slab kernels, the Python layers above them --
against numpy fp64 (``np.linalg.solve``, the oracle's closed-form kernels), and the outputs of the entries this work
must not change against recordings of the parent commit's build (tests/golden/parent_bits/fast_any.npz, data only).

Inputs are of the family tests/test_gpu_large.py uses: points uniform in the unit cube with LS = 0.5 and a nugget of
1e-2 (or, for the workflow test, the Gaussian points of tests/test_gpu_fast_mean.py with noise 1e-2).
tests/test_fast_any_cpu.py::test_fp32_numpy_solve_stays_inside_the_band checks on the CPU that ``np.linalg.solve`` in
fp32 itself stays inside RTOL on the coefficient cases below."""

import ctypes as C
import os

import numpy as np
import pytest

from oracle import muygps_oracle as orc
from tests.util import RTOL, assert_close, to_dev

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LS, NUGGET = 0.5, 1e-2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parent_bits", "fast_any.npz")
ANISO8 = [0.4, 0.6, 0.5, 0.7, 0.45, 0.55, 0.65, 0.5]


def TD(dtype):
    return getattr(torch, dtype)


def make_table(rng, n, d, R=1):
    X = rng.uniform(size=(n, d))
    Y = np.stack([np.sin(3.0 * X.sum(1) + r) + 0.1 * rng.normal(size=n) for r in range(R)], axis=1)
    return X, Y


def neighbourhoods(rng, n, b, k):
    return np.stack([rng.choice(n, size=k, replace=False) for _ in range(b)])


def k_lds(dtype, R):
    from muygpys_amd import _lib

    return _lib.load().mgp_max_nn_count(4 if dtype == "float32" else 8, R)


# ---- 1. the prediction kernel: edges ----------------------------------------------------------------------------------
# Every k of {63, 64, 65, 127, 128, 129, 300, 1023} with every d of {1, 3, 8, 70} (scalar gather, vector gather in fp32
# only at d = 8 -- fp64 vectors need d % 2 == 0: d = 8 and 70 --, a second feature chunk with a ragged tail); the other
# factors -- dtype, (kernel, metric), Isotropy / Anisotropy, R in {1, 3}, batch_idx or None -- cycle with co-prime
# periods over the 32 (k, d) pairs so that each value of each meets several k and several d.  The query table is
# always a table of its own; coeff_row is a random draw without repetition from a coefficient table of 41 rows.
PRED_K = (63, 64, 65, 127, 128, 129, 300, 1023)
PRED_D = (1, 3, 8, 70)
MODELS = (("matern15", "l2"), ("rbf", "F2"), ("matern25", "l2"))


def _prediction_cases():
    cases = []
    for i, (k, d) in enumerate((k, d) for k in PRED_K for d in PRED_D):
        kernel, metric = MODELS[i % 3]
        cases.append(dict(k=k, d=d, dtype=("float32", "float64")[(i + i // 4) % 2], kernel=kernel, metric=metric,
                          aniso=(i % 5) in (1, 3), R=(1, 3)[(i // 2 + i // 8) % 2], batch_idx=(i % 7) not in (2, 5)))
    return cases


PRED_CASES = _prediction_cases()
# ... and the fp32 vector gather in a second feature chunk (d a multiple of 4 above 64; d = 70 reaches it in fp64 only):
# one pass and five passes of neighbours, ragged last pass
PRED_CASES += [dict(k=k, d=68, dtype="float32", kernel="matern15", metric="l2", aniso=a, R=3, batch_idx=True)
               for k, a in ((65, False), (300, True))]


def test_prediction_sample_covers_every_factor():
    for key, values in (("dtype", ("float32", "float64")), ("aniso", (False, True)), ("R", (1, 3)), ("batch_idx", (False, True)),
                        ("metric", ("l2", "F2"))):
        for v in values:
            mine = [c for c in PRED_CASES if c[key] == v and c["d"] != 68]
            assert len({c["d"] for c in mine}) == len(PRED_D), (key, v)
            assert len({c["k"] for c in mine}) >= 4, (key, v)
    assert {(c["k"], c["d"]) for c in PRED_CASES if c["d"] != 68} == {(k, d) for k in PRED_K for d in PRED_D}


def prediction_problem(c):
    rng = np.random.default_rng(1000 * c["k"] + c["d"])
    n, b, nq, nco = 1100, 37, 50, 41
    k, d, R = c["k"], c["d"], c["R"]
    X, Q = rng.uniform(size=(n, d)), rng.uniform(size=(nq, d))
    ni = neighbourhoods(rng, n, b, k)
    bi = rng.choice(nq, size=b, replace=False) if c["batch_idx"] else None
    co = rng.normal(size=(nco, k, R))
    crow = rng.permutation(nco)[:b]
    # (length scales that keep the covariances of order 0.1 - 1 in d dimensions)
    ell = LS * np.sqrt(d / 8.0) if d > 1 else LS
    ls = (ell * (0.75 + 0.5 * rng.uniform(size=d))).tolist() if c["aniso"] else ell
    return X, Q, ni, bi, co, crow, ls


@pytest.mark.parametrize("c", PRED_CASES, ids=lambda c: "k{k}-d{d}-{dtype}-{kernel}-{metric}-aniso{aniso:d}-R{R}-bi{batch_idx:d}".format(**c))
def test_prediction_kernel_edges(c):
    from muygpys_amd.fused import KernelSpec, fast_posterior_mean

    X, Q, ni, bi, co, crow, ls = prediction_problem(c)
    b = ni.shape[0]
    ospec = orc.Spec(c["kernel"], c["metric"], np.asarray(ls) if c["aniso"] else ls, 0.0)
    cd = orc.crosswise_tensor(Q, X, bi if bi is not None else np.arange(b), ni)
    Kc, _ = orc.kernel_tensors(ospec, cd, orc.pairwise_tensor(X, ni[:1, :2]))
    ref = np.einsum("bk,bkr->br", Kc, co[crow])
    t = TD(c["dtype"])
    spec = KernelSpec(c["kernel"], c["metric"], ls, 0.0)
    got = fast_posterior_mean(spec, to_dev(Q, t), to_dev(X, t), None if bi is None else to_dev(bi), to_dev(ni),
                              to_dev(co if c["R"] > 1 else co[:, :, 0], t), to_dev(crow))
    torch.cuda.synchronize()
    got = got.cpu().numpy().reshape(b, c["R"])
    print(f"max abs err {np.abs(got - ref).max():.3e}, rms(ref) {np.sqrt((ref ** 2).mean()):.3e}")
    assert_close(got, ref, 3 * RTOL[c["dtype"]], "fast posterior mean")


# ---- 2. / 4. unchanged bits: recordings of the parent commit's build ---------------------------------------------------
def parent_cases(lib):
    """{name: ndarray} of the entries whose outputs must not change, by direct calls of the C ABI on ``lib`` (functions
    bound from the header): the prediction kernel at k = 63 and k = 30 (the 64- and 32-slot instantiations),
    ``mgp_posterior_generic_*`` on an LDS shape (k = 100) and ``mgp_posterior_large_*`` on a slab shape (k = 200)."""
    out = {}
    P = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    for dtype, suf, es in (("float32", "f32", 4), ("float64", "f64", 8)):
        t = TD(dtype)
        for k in (63, 30):
            rng = np.random.default_rng(k)
            n, b, d, R = 1100, 37, 8, 3
            X, Q = to_dev(rng.uniform(size=(n, d)), t), to_dev(rng.uniform(size=(50, d)), t)
            ni, bi = to_dev(neighbourhoods(rng, n, b, k)), to_dev(rng.choice(50, size=b, replace=False))
            co, crow = to_dev(rng.normal(size=(41, k, R)), t), to_dev(rng.permutation(41)[:b])
            ls = to_dev(np.array([LS]), t)
            mean = torch.full((b, R), float("nan"), device="cuda", dtype=t)
            rc = getattr(lib, f"mgp_fast_posterior_mean_{suf}")(P(Q), P(X), d, P(bi), P(ni), b, k, P(co), P(crow), R, 2, 0, P(ls), 1,
                                                                P(mean), None)
            assert rc == 0
            torch.cuda.synchronize()
            out[f"fast_mean_k{k}_{suf}"] = mean.cpu().numpy()
        for name, k, b in (("posterior_generic", 100, 6), ("posterior_large", 200, 3)):
            rng = np.random.default_rng(k)
            n, d, R = 600, 8, 1
            Xn, Yn = make_table(rng, n, d, R)
            X, Y = to_dev(Xn, t), to_dev(Yn, t)
            ni, bi = to_dev(neighbourhoods(rng, n, b, k)), to_dev(rng.choice(n, size=b, replace=False))
            ls = to_dev(np.array([LS]), t)
            mean, var, yk = (torch.full(s, float("nan"), device="cuda", dtype=t) for s in ((b, R), (b,), (b, R)))
            info = torch.zeros(1, dtype=torch.int32, device="cuda")
            head = (P(X), P(X), d, P(bi), P(ni), b, k, P(Y), R)
            model = (0, NUGGET, None, 2, 0, P(ls), 1, P(mean), P(var), P(yk), P(info))
            if name == "posterior_generic":
                rc = getattr(lib, f"mgp_posterior_generic_{suf}")(*head, *model, None)
            else:
                size = lib.mgp_large_workspace_bytes(es, k, R, b)
                ws = torch.empty(size, dtype=torch.uint8, device="cuda")
                rc = getattr(lib, f"mgp_posterior_large_{suf}")(*head, 0, *model, P(ws), size, None)
            assert rc == 0
            torch.cuda.synchronize()
            assert int(info.item()) == 0
            for o, x in (("mean", mean), ("var", var), ("yk", yk)):
                out[f"{name}_{o}_{suf}"] = x.cpu().numpy()
    return out


def test_untouched_entries_return_the_parent_commits_bits():
    from muygpys_amd import _lib

    now = parent_cases(_lib.load())
    then = np.load(GOLDEN)
    assert sorted(now) == sorted(then.files)
    for name in then.files:
        assert np.isfinite(then[name]).all(), name
        assert torch.equal(torch.from_numpy(now[name]), torch.from_numpy(then[name])), name


# ---- 3. the coefficient entry -----------------------------------------------------------------------------------------
def coefficient_problem(k, R, noise_mode, aniso, seed, b=6, n=1100, d=8):
    """Tables, ``b`` neighbourhoods, the noise in the given mode and the fp64 system matrices / right-hand sides."""
    rng = np.random.default_rng(seed)
    X, Y = make_table(rng, n, d, R)
    ni = neighbourhoods(rng, n, b, k)
    ls = ANISO8 if aniso else LS
    if noise_mode == "scalar":
        noise, rows = NUGGET, np.full((b, k), NUGGET)
    elif noise_mode == "table":
        noise = 10.0 ** (-2.5 + rng.uniform(size=n))
        rows = noise[ni]
    else:
        noise = 10.0 ** (-2.5 + rng.uniform(size=(b, k)))
        rows = noise
    ospec = orc.Spec("matern15", "l2", np.asarray(ls) if aniso else ls, 0.0)
    pd = orc.pairwise_tensor(X, ni)
    _, Kin = orc.kernel_tensors(ospec, pd[:, 0], pd)
    Kin = Kin + np.stack([np.diag(r) for r in rows])
    return X, Y, ni, ls, noise, Kin, Y[ni]


def call_any(dtype, X, Y, ni, ls, noise, workspace="recommended", info=None):
    """One ``mgp_fast_coefficients_any_*`` call through ``_lib`` directly -> (coeffs (b, k, R), info)."""
    from muygpys_amd import _lib
    from muygpys_amd.fused import KernelSpec, _normalize

    t = TD(dtype)
    nz = to_dev(noise, t) if isinstance(noise, np.ndarray) else noise
    spec = KernelSpec("matern15", "l2", ls, nz)
    Xd = to_dev(X, t)
    inp = _normalize(spec, Xd, Xd, None, to_dev(ni), to_dev(Y, t))
    es = 4 if dtype == "float32" else 8
    lib = _lib.load()
    size = lib.mgp_fast_coefficients_workspace_bytes(es, inp.k, inp.R, 1 if workspace == "one slab" else inp.b)
    ws = torch.empty(size, dtype=torch.uint8, device="cuda") if size else None
    out = torch.full((inp.b, inp.k, inp.R), float("nan"), device="cuda", dtype=t)
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    P = _lib.ptr
    rc = _lib.fn("fast_coefficients_any", t)(P(inp.fn), inp.d, P(inp.ni), inp.b, inp.k, P(inp.tg), inp.R, inp.mode, inp.eps, P(inp.nz),
                                             spec.kernel_id(), spec.metric_id(), P(inp.ls), inp.ls.numel(), P(out), P(info), P(ws),
                                             size, _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out, int(info.item()), size


def coefficient_cases():
    """k in {62, 63, 64, mgp_max_nn_count, that + 1, 300} x R in {1, 3} x dtype; the three noise modes in turn, per-feature
    length scales once per dtype."""
    cases = []
    for dtype in ("float32", "float64"):
        for j, (k, R) in enumerate((k, R) for k in (62, 63, 64, "kmax", "kmax+1", 300) for R in (1, 3)):
            cases.append(dict(dtype=dtype, k=k, R=R, noise_mode=("scalar", "table", "batch")[j % 3], aniso=j == 7))
    return cases


def resolve_k(c):
    k = c["k"]
    return k if isinstance(k, int) else k_lds(c["dtype"], c["R"]) + (1 if k == "kmax+1" else 0)


@pytest.mark.parametrize("c", coefficient_cases(), ids=lambda c: "{dtype}-k{k}-R{R}-{noise_mode}-aniso{aniso:d}".format(**c))
def test_coefficient_entry(c):
    k = resolve_k(c)
    X, Y, ni, ls, noise, Kin, Yn = coefficient_problem(k, c["R"], c["noise_mode"], c["aniso"], seed=k + c["R"])
    got, bad, size = call_any(c["dtype"], X, Y, ni, ls, noise)
    assert bad == 0 and (size > 0) == (k > k_lds(c["dtype"], c["R"]))
    ref = np.linalg.solve(Kin, Yn)
    print(f"max abs err {np.abs(got.cpu().numpy() - ref).max():.3e}, rms(ref) {np.sqrt((ref ** 2).mean()):.3e}")
    assert_close(got.cpu().numpy(), ref, RTOL[c["dtype"]], "coefficients")


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("R", [1, 3])
def test_coefficient_entry_at_the_row_limit(dtype, R):
    k = 1023 - R
    X, Y, ni, ls, noise, Kin, Yn = coefficient_problem(k, R, "scalar", False, seed=k, b=3)
    got, bad, size = call_any(dtype, X, Y, ni, ls, noise)
    assert bad == 0 and size > 0
    ref = np.linalg.solve(Kin, Yn)
    print(f"max abs err {np.abs(got.cpu().numpy() - ref).max():.3e}, rms(ref) {np.sqrt((ref ** 2).mean()):.3e}")
    assert_close(got.cpu().numpy(), ref, RTOL[dtype], "coefficients")


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("k", [64, 300])
def test_coefficients_do_not_depend_on_workspace_or_place(dtype, k):
    X, Y, ni, ls, noise, _, _ = coefficient_problem(k, 3, "table", False, seed=77 + k)
    full, _, size = call_any(dtype, X, Y, ni, ls, noise)
    if size:
        one, _, slab = call_any(dtype, X, Y, ni, ls, noise, workspace="one slab")
        assert 0 < slab < size and torch.equal(one, full), "a workspace of exactly one slab"
    perm = np.array([4, 0, 5, 2, 1, 3])
    moved, _, _ = call_any(dtype, X, Y, ni[perm], ls, noise)
    assert torch.equal(moved, full[to_dev(perm)]), "a neighbourhood at another place in the batch"
    alone, _, _ = call_any(dtype, X, Y, ni[3:4], ls, noise)
    assert torch.equal(alone[0], full[3]), "a neighbourhood in a batch of its own"


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("k", [64, 300])
def test_a_singular_neighbourhood_is_nan_and_counted(dtype, k):
    """A duplicated index with zero noise: NaN in that (k, R) block, one count, the neighbours untouched (the numerical
    flag path of the factorisation, as for mgp_solve_*)."""
    X, Y, ni, ls, noise, Kin, Yn = coefficient_problem(k, 3, "batch", False, seed=5 + k)
    broken, good = 2, np.array([0, 1, 3, 4, 5])
    ni = ni.copy()
    ni[broken, 1] = ni[broken, 0]
    noise = noise.copy()
    noise[broken] = 0.0
    got, bad, _ = call_any(dtype, X, Y, ni, ls, noise)
    assert bad == 1
    assert torch.isnan(got[broken]).all() and torch.isfinite(got[to_dev(good)]).all()
    assert_close(got[to_dev(good)].cpu().numpy(), np.linalg.solve(Kin[good], Yn[good]), RTOL[dtype], "the five good neighbourhoods")


# ---- 5. the workflow --------------------------------------------------------------------------------------------------
def oracle_fast(X, y, Q, k, spec):
    """tests/test_gpu_fast_mean.py::oracle_fast: fast_nn_update applied once."""
    from sklearn.neighbors import NearestNeighbors

    nbrs = NearestNeighbors(n_neighbors=k + 1, algorithm="brute").fit(X)
    nn = nbrs.kneighbors(X, return_distance=False)[:, 1:]
    nn_fast = orc.fast_nn_update(nn)
    pd = orc.pairwise_tensor(X, nn_fast)
    _, Kin = orc.kernel_tensors(spec, pd[:, 0], pd)
    coeffs = orc.fast_posterior_mean_precompute(orc.perturb(spec, Kin, nn_fast), y[nn_fast])
    test_nn = nbrs.kneighbors(Q, n_neighbors=k, return_distance=False)
    closest = test_nn[:, 0]
    cd = orc.crosswise_tensor(Q, X, np.arange(len(Q)), nn_fast[closest])
    Kc, _ = orc.kernel_tensors(spec, cd, pd[:1])
    return (nn, test_nn), coeffs, orc.fast_posterior_mean(Kc, coeffs[closest])


@pytest.fixture(scope="module")
def workflow_problem():
    rng = np.random.default_rng(17)
    n, d, k, R = 1500, 8, 100, 3
    X = rng.normal(size=(n, d))
    W = rng.normal(size=(d, R)) / np.sqrt(d)
    Y = np.sin(X @ W) + 0.05 * rng.normal(size=(n, R))
    Q = rng.normal(size=(300, d))
    return X, Y, Q, k, oracle_fast(X, Y, Q, k, orc.Spec("matern15", "l2", 2.5, 1e-2))


def spy_on_library(monkeypatch):
    from muygpys_amd import _lib

    calls, real = [], _lib.fn
    monkeypatch.setattr(_lib, "fn", lambda base, dtype: (calls.append(base), real(base, dtype))[1])
    return calls


def model(ls=2.5, noise=1e-2):
    from muygpys_amd.gp import MuyGPS
    from muygpys_amd.gp.deformation import Isotropy, l2
    from muygpys_amd.gp.hyperparameter import Parameter
    from muygpys_amd.gp.kernels import Matern
    from muygpys_amd.gp.noise import HomoscedasticNoise

    return MuyGPS(kernel=Matern(smoothness=Parameter(1.5), deformation=Isotropy(l2, Parameter(ls))), noise=HomoscedasticNoise(noise))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_workflow_is_two_fused_launches(workflow_problem, dtype, monkeypatch):
    from muygpys_amd.examples.fast_posterior_mean import fast_posterior_mean_any
    from muygpys_amd.neighbors import NN_Wrapper

    X, Y, Q, k, ((nn, test_nn), coeffs_ref, mean_ref) = workflow_problem
    t = TD(dtype)
    Xd, Yd, Qd = to_dev(X, t), to_dev(Y, t), to_dev(Q, t)
    nbrs = NN_Wrapper(Xd, k)
    calls = spy_on_library(monkeypatch)
    mean, coeffs, timing = fast_posterior_mean_any(model(), Qd, Xd, nbrs, Yd)
    torch.cuda.synchronize()
    assert sorted(timing) == ["agree", "nn", "precompute", "pred"]
    assert calls.count("fast_coefficients_any") == 1 and calls.count("fast_posterior_mean") == 1, calls
    assert not {"pairwise_dists", "pairwise_diffs", "crosswise_dists", "solve", "solve_large", "kernel_apply"} & set(calls), calls
    assert coeffs.shape == coeffs_ref.shape and mean.shape == mean_ref.shape
    # The k-NN front end is the real one in both dtypes.  On the features ROUNDED to fp32 the exact search may order two
    # nearly equidistant neighbours the other way round than the fp64 oracle (one row of 1500 at k = 100 on this seed):
    # a legitimate answer that permutes that row's coefficients.  The order of the k-NN is not what this test is about,
    # so the values are compared where both sides solved the same list -- which must be all rows in fp64 and nearly all
    # (99 % of the training rows, 98 % of the test points: the comparison may not become vacuous) in fp32.
    nn_d = nbrs.get_batch_nns(torch.arange(X.shape[0], device="cuda"))[0].cpu().numpy()
    closest_d = nbrs.get_nns(Qd)[0][:, 0].cpu().numpy()
    same_rows = (nn_d == nn).all(axis=1)
    same_points = (closest_d == test_nn[:, 0]) & same_rows[test_nn[:, 0]]
    print(f"{dtype}: {same_rows.sum()} of {same_rows.size} training rows and {same_points.sum()} of {same_points.size} "
          "test points with the oracle's lists")
    if dtype == "float64":
        assert same_rows.all() and same_points.all()
    assert same_rows.mean() >= 0.99 and same_points.mean() >= 0.98
    assert_close(coeffs.cpu().numpy()[same_rows], coeffs_ref[same_rows], RTOL[dtype], "coefficients")
    assert_close(mean.cpu().numpy()[same_points], mean_ref[same_points], 3 * RTOL[dtype], "fast posterior mean")


def test_multivariate_workflow_is_one_launch_pair_per_model(workflow_problem, monkeypatch):
    from muygpys_amd.examples.fast_posterior_mean import fast_posterior_mean_any
    from muygpys_amd.neighbors import NN_Wrapper

    X, Y, Q, k, (_, coeffs_ref, mean_ref) = workflow_problem

    class Multi:
        models = [model(), model(), model()]

    Xd, Yd, Qd = to_dev(X, torch.float64), to_dev(Y, torch.float64), to_dev(Q, torch.float64)
    calls = spy_on_library(monkeypatch)
    mean, coeffs, _ = fast_posterior_mean_any(Multi(), Qd, Xd, NN_Wrapper(Xd, k), Yd)
    torch.cuda.synchronize()
    assert calls.count("fast_coefficients_any") == 3 and calls.count("fast_posterior_mean") == 3, calls
    assert_close(coeffs.cpu().numpy(), coeffs_ref, RTOL["float64"], "coefficients")
    assert_close(mean.cpu().numpy(), mean_ref, 3 * RTOL["float64"], "fast posterior mean")


# ---- 6. the functor layer ---------------------------------------------------------------------------------------------
def test_functor_layer_precompute_is_the_fused_launch_and_stays_small(monkeypatch):
    """Lazy pairwise_tensor -> m.kernel -> m.fast_coefficients at k = 100, n = 20 000, fp32: one fused launch whose
    peak allocation stays below 4 n k R s + the workspace -- the materialising route needs n k k s = 800 MB for Kin
    alone."""
    from muygpys_amd import _lib, lazy

    rng = np.random.default_rng(3)
    n, d, k, R, s = 20_000, 8, 100, 1, 4
    X, Y = make_table(rng, n, d, R)
    Xd, yd = to_dev(X, torch.float32), to_dev(Y[:, 0], torch.float32)
    # (self-including lists of k distinct rows: row i, then k - 1 distinct non-zero offsets from it)
    offsets = np.concatenate([[0], rng.choice(np.arange(1, n), size=k - 1, replace=False)])
    ni = to_dev((np.arange(n)[:, None] + offsets[None, :]) % n)
    m = model(LS, NUGGET)
    ws = _lib.workspace("mgp_fast_coefficients_workspace_bytes", torch.float32, k, R, n, device="cuda")
    ws_bytes = 0 if ws is None else ws.numel()
    del ws
    calls = spy_on_library(monkeypatch)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    Kin = m.kernel(m.kernel.deformation.pairwise_tensor(Xd, ni, lazy=True))
    co = m.fast_coefficients(Kin, lazy.LazyTargets(yd, ni))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    assert calls.count("fast_coefficients_any") == 1 and "solve" not in calls and "pairwise_dists" not in calls, calls
    assert co.shape == (n, k)
    print(f"peak {peak / 1e6:.1f} MB; bound {(4 * n * k * R * s + ws_bytes) / 1e6:.1f} MB")
    assert peak < 4 * n * k * R * s + ws_bytes
    # the materialised Kin still takes the solve, and agrees (the first 64 neighbourhoods)
    sub = ni[:64].contiguous()
    calls.clear()
    Kin_m = m.kernel(m.kernel.deformation.pairwise_tensor(Xd, sub))
    dense = m.fast_coefficients(Kin_m, yd[sub])
    torch.cuda.synchronize()
    assert "solve" in calls and "fast_coefficients_any" not in calls, calls
    # (two fp32 results, each held to RTOL against fp64 below: at most 2 RTOL apart)
    assert_close(co[:64].cpu().numpy(), dense.cpu().numpy(), 2 * RTOL["float32"], "fused against materialised")
    Xn, idx = X, sub.cpu().numpy()
    pd = orc.pairwise_tensor(Xn, idx)
    _, K64 = orc.kernel_tensors(orc.Spec("matern15", "l2", LS, NUGGET), pd[:, 0], pd)
    ref = np.linalg.solve(K64 + NUGGET * np.eye(k), Y[idx])[:, :, 0]
    assert_close(co[:64].cpu().numpy(), ref, RTOL["float32"], "coefficients")
    assert_close(dense.cpu().numpy(), ref, RTOL["float32"], "coefficients (materialised)")


# ---- 7. the general nu: no fused coefficient kernel, the forced solve ---------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("k", [30, 62, 70])
def test_general_nu_precompute_takes_the_forced_solve(k, dtype, monkeypatch):
    """A free Matern smoothness (``Matern(smoothness=2.0)``: the general Bessel form) on lazy handles, one response, at
    k <= 62 (the wave entry's shapes, which does not know the kernel id) and beyond: the functor layer forces the handle
    and solves, as before the fused coefficient launch existed, and ``fused.fast_coefficients`` takes its chunked
    route through ``mgp_matern_gen_*``; both agree with the oracle."""
    from muygpys_amd import fused, lazy
    from muygpys_amd.gp import MuyGPS
    from muygpys_amd.gp.deformation import Isotropy, l2
    from muygpys_amd.gp.hyperparameter import Parameter
    from muygpys_amd.gp.kernels import Matern
    from muygpys_amd.gp.noise import HomoscedasticNoise

    nu = 2.0
    rng = np.random.default_rng(900 + k)
    n, d = 300, 8
    X, Y = make_table(rng, n, d)
    nn = np.stack([rng.choice(np.delete(np.arange(n), i), size=k, replace=False) for i in range(n)])  # (never i itself)
    nn_fast = orc.fast_nn_update(nn)
    pd = orc.pairwise_tensor(X, nn_fast)
    ospec = orc.Spec(lambda r: orc.matern_gen_fn(r, nu), "l2", LS, NUGGET)
    _, Kin = orc.kernel_tensors(ospec, pd[:, 0], pd)
    ref = np.linalg.solve(Kin + NUGGET * np.eye(k), Y[nn_fast])[:, :, 0]
    t = TD(dtype)
    Xd, yd, nnd = to_dev(X, t), to_dev(Y[:, 0], t), to_dev(nn_fast)
    m = MuyGPS(kernel=Matern(smoothness=Parameter(nu), deformation=Isotropy(l2, Parameter(LS))), noise=HomoscedasticNoise(NUGGET))
    calls = spy_on_library(monkeypatch)
    Kin_lazy = m.kernel(m.kernel.deformation.pairwise_tensor(Xd, nnd, lazy=True))
    assert isinstance(Kin_lazy, lazy.LazyCov) and Kin_lazy.kernel == "matern_gen"
    co = m.fast_coefficients(Kin_lazy, lazy.LazyTargets(yd, nnd))
    torch.cuda.synchronize()
    assert "solve" in calls and not {"fast_coefficients", "fast_coefficients_any"} & set(calls), calls
    assert_close(co.cpu().numpy(), ref, RTOL[dtype], "coefficients (functor layer)")
    calls.clear()
    co2, nn_fast_d = fused.fast_coefficients(fused.KernelSpec("matern_gen", "l2", LS, NUGGET, smoothness=nu), Xd, yd, to_dev(nn))
    torch.cuda.synchronize()
    assert np.array_equal(nn_fast_d.cpu().numpy(), nn_fast)
    assert "solve" in calls and "matern_gen" in calls and not {"fast_coefficients", "fast_coefficients_any"} & set(calls), calls
    assert_close(co2.cpu().numpy(), ref, RTOL[dtype], "coefficients (fused.fast_coefficients)")
