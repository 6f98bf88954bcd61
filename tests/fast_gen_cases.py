"""The case lists and numpy problems of the general-smoothness fast-posterior-mean tests (tests/test_gpu_fast_gen.py on
the device, tests/test_fast_gen_cpu.py for what is decided about the lists without one).  numpy and the oracle only.

Inputs follow tests/test_gpu_gen_beyond64.py and tests/test_gpu_fast_any.py: points uniform in the unit cube, length
scale 0.5 sqrt(d / 8) (0.5 at d = 1), nugget 1e-2, responses sin(3 sum x + r) + 0.1 noise; the l2 metric throughout."""

import numpy as np

from oracle import muygps_oracle as orc

LS, NUGGET = 0.5, 1e-2
NUS = (0.42, 1.0, 2.2, 3.7, 8.0)
# fp32: 3 x 1e-3 for coefficients and predictions; fp64: tests.util.RTOL
BAND = {"float32": 3e-3, "float64": 1e-5}


def gen_spec(nu, ls, noise=0.0, fn=None):
    fn = orc.matern_gen_fn if fn is None else fn
    return orc.Spec(lambda r: fn(r, nu), "l2", ls, noise)


def length_scale(d):
    return LS * np.sqrt(d / 8.0) if d > 1 else LS


def make_table(rng, n, d, R=1):
    X = rng.uniform(size=(n, d))
    Y = np.stack([np.sin(3.0 * X.sum(1) + r) + 0.1 * rng.normal(size=n) for r in range(R)], axis=1)
    return X, Y


def neighbourhoods(rng, n, b, k):
    return np.stack([rng.choice(n, size=k, replace=False) for _ in range(b)])


# ---- prediction ---------------------------------------------------------------------------------------------------------
# k: both narrow kernels with a nearly empty and a full half-wave / wave (1, 31 | 32, 63), then the wide kernel with one
# pass, ragged passes and the widest list; d: scalar gather, vector gather, second feature chunk.  The other factors
# cycle over the 40 (k, d) pairs with co-prime periods (tests/test_fast_gen_cpu.py proves the coverage).
PRED_K = (1, 31, 32, 63, 64, 65, 128, 129, 300, 1023)
PRED_D = (1, 3, 8, 70)


def prediction_cases():
    cases = []
    for i, (k, d) in enumerate((k, d) for k in PRED_K for d in PRED_D):
        cases.append(dict(k=k, d=d, dtype=("float32", "float64")[(i + i // 4) % 2], nu=NUS[i % 5], aniso=(i % 7) in (1, 3, 5),
                          R=(1, 3)[(i // 2 + i // 8) % 2], batch_idx=(i % 3) != 1, zero=False))
    # a test point exactly on one of its neighbours, on a narrow and on the wide kernel; nu = 30, the last one accepted
    cases.append(dict(k=30, d=8, dtype="float32", nu=2.2, aniso=False, R=3, batch_idx=True, zero=True))
    cases.append(dict(k=100, d=3, dtype="float64", nu=0.42, aniso=False, R=1, batch_idx=True, zero=True))
    cases.append(dict(k=40, d=8, dtype="float64", nu=30.0, aniso=False, R=3, batch_idx=True, zero=False))
    return cases


def prediction_id(c):
    return "k{k}-d{d}-{dtype}-nu{nu}-aniso{aniso:d}-R{R}-bi{batch_idx:d}-zero{zero:d}".format(**c)


def prediction_problem(c):
    """37 test points of a query table of its own, normal coefficients drawn from a 41-row table."""
    rng = np.random.default_rng(1000 * c["k"] + c["d"])
    n, b, nq, nco = 1100, 37, 50, 41
    k, d, R = c["k"], c["d"], c["R"]
    X, Q = rng.uniform(size=(n, d)), rng.uniform(size=(nq, d))
    ni = neighbourhoods(rng, n, b, k)
    bi = rng.choice(nq, size=b, replace=False) if c["batch_idx"] else None
    co = rng.normal(size=(nco, k, R))
    crow = rng.permutation(nco)[:b]
    ell = length_scale(d)
    ls = (ell * (0.75 + 0.5 * rng.uniform(size=d))).tolist() if c["aniso"] else ell
    if c["zero"]:  # test point 5 sits on its third neighbour (min: k = 1, 2)
        Q[5 if bi is None else bi[5]] = X[ni[5, min(2, k - 1)]]
    return X, Q, ni, bi, co, crow, ls


def prediction_reference(c, problem, fn=None):
    X, Q, ni, bi, co, crow, ls = problem
    b = ni.shape[0]
    cd = orc.crosswise_tensor(Q, X, bi if bi is not None else np.arange(b), ni)
    Kc, _ = orc.kernel_tensors(gen_spec(c["nu"], np.asarray(ls) if c["aniso"] else ls, fn=fn), cd, orc.pairwise_tensor(X, ni[:1, :1]))
    return np.einsum("bk,bkr->br", Kc, co[crow])


# ---- coefficients ---------------------------------------------------------------------------------------------------------
# k: "L" = the LDS limit of the entry for the case's dtype and R (mgp_max_nn_count_gen), resolved where a library is at
# hand.  62 / 63: the 64- / 256-thread workgroup; 90: the strip edge of gen_covariance_phase (4095 pairs: one short of
# four strips of 256 x 4 in fp32); L + 1: the first slab shape; 239: the 512-thread strip edge.  The rules of
# tests/test_gpu_gen_beyond64.py hold: in fp32 nu = 8 stays out of d <= 3, and d = 1 with k >= 31 runs in fp64 only.
COEF_K = (1, 2, 31, 62, 63, 90, "L", "L+1", 239, 300)
COEF_D = (1, 3, 8, 40)


def coefficient_cases():
    cases = []
    for i, (k, d) in enumerate((k, d) for k in COEF_K for d in COEF_D):
        dtype = ("float32", "float64")[(i + i // 4) % 2]
        nu = NUS[i % 5]
        big = not isinstance(k, int) or k >= 31
        if d == 1 and big:
            dtype = "float64"
        if dtype == "float32" and d <= 3 and nu == 8.0:
            nu = 3.7
        cases.append(dict(k=k, d=d, dtype=dtype, nu=nu, R=(1, 3)[(i // 2 + i // 8) % 2], aniso=i == 14, noise="rows" if i == 22 else "scalar",
                          b=24, n=400))
    # k + 1 + R = 1024 exactly
    cases.append(dict(k=1020, d=3, dtype="float64", nu=2.2, R=3, aniso=False, noise="scalar", b=3, n=1100))
    return cases


def coefficient_id(c):
    return "k{k}-d{d}-{dtype}-nu{nu}-R{R}-aniso{aniso:d}-{noise}".format(**c)


def resolve_k(c, limit):
    """``limit(dtype, R)``: mgp_max_nn_count_gen."""
    k = c["k"]
    return k if isinstance(k, int) else limit(c["dtype"], c["R"]) + (1 if k == "L+1" else 0)


def coefficient_problem(c, k):
    """b neighbourhoods drawn without repetition from n rows; (X, Y, ni, ls, noise, rows) with the noise as the spec
    takes it (a number, or a per-row table (n,)) and gathered (b, k)."""
    rng = np.random.default_rng(7 * k + c["d"])
    X, Y = make_table(rng, c["n"], c["d"], c["R"])
    ni = neighbourhoods(rng, c["n"], c["b"], k)
    ell = length_scale(c["d"])
    ls = (ell * (0.75 + 0.5 * rng.uniform(size=c["d"]))).tolist() if c["aniso"] else ell
    if c["noise"] == "rows":
        noise = 10.0 ** (-2.5 + rng.uniform(size=c["n"]))
        rows = noise[ni]
    else:
        noise, rows = NUGGET, np.full(ni.shape, NUGGET)
    return X, Y, ni, ls, noise, rows


def coefficient_reference(c, problem, fn=None):
    X, Y, ni, ls, noise, rows = problem
    pd = orc.pairwise_tensor(X, ni)
    _, Kin = orc.kernel_tensors(gen_spec(c["nu"], np.asarray(ls) if c["aniso"] else ls, fn=fn), pd[:, 0], pd)
    Kin = Kin + np.stack([np.diag(r) for r in rows])
    return np.linalg.solve(Kin, Y[ni])
