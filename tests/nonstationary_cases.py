"""A length scale per neighbourhood (mgp_posterior_ns_generic_*, mgp_posterior_ns_large_*; KernelSpec.length_scale_batch):
the case table of tests/test_gpu_nonstationary.py and an fp64 numpy reference that applies the oracle's existing
functions (oracle/muygps_oracle.py) neighbourhood by neighbourhood, each with its own scale.

CPU only (numpy; torch is not imported here).  tests/test_nonstationary_cases_cpu.py checks the reference against
fixtures written by the real reference (tests/golden/hier/hier_*.npz) and, at a constant scale, against the oracle's scalar
pipeline.

The recipe of a case.  Features uniform on [0, L]^d with L = 3 / sqrt(d / 6), so that a typical pair of points lies 3
apart at every d; responses sin(sum(x) / (L sqrt(d)) * 3 + r) + 0.1 normal; neighbourhoods of k distinct random rows;
noise 0.05 (scalar), 0.05 (1 + 3 U) per table row (table) or that table gathered (batch).  The scales are drawn
log-uniformly over [0.2, 5] across the batch (Isotropy: one per neighbourhood; Anisotropy: d per neighbourhood), so a
kernel that ignores the position in the batch, or indexes by batch_idx[nb], misses by far more than any tolerance.  At
the largest scale, 5, the metric argument of a typical pair is 3 / 5 (l2) or 9 / 25 (F2) and the covariances are those
of tests/posterior_cases.py's recipe (O(0.5) .. O(0.8)); at the smallest, 0.2, the system is the identity plus noise.
With the nugget of 0.05 the posterior variance stays above 0.05 / (1 + 0.05) / k-ish of its prior, the regime in which
posterior_cases holds the variance to the pure relative band."""

import functools
from types import SimpleNamespace

import numpy as np

from oracle import muygps_oracle as orc

SEED = 20261021
N = 300
NOISE = 0.05
LS_LO, LS_HI = 0.2, 5.0
ES = {"float32": 4, "float64": 8}
CNAME = {"float32": "float", "float64": "double"}


def lds_max(dtype, R):
    """mgp_max_nn_count(es, R): the largest nn_count of the LDS entry (the library answers without a GPU)."""
    from muygpys_amd import _lib

    return int(_lib.load().mgp_max_nn_count(ES[dtype], R))


def _case(entry, dtype, k, d, R=1, aniso=False, kernel="matern15", metric="l2", b=7, bi=True, noise="scalar", gathered=False):
    k = lds_max(dtype, R) + (1 if k == "max+1" else 0) if k in ("max", "max+1") else k
    c = dict(entry=entry, dtype=dtype, k=k, d=d, R=R, aniso=aniso, kernel=kernel, metric=metric, b=b, bi=bi, noise=noise,
             gathered=gathered)
    c["id"] = (f"{entry}-{dtype}-k{k}-d{d}-R{R}-{'aniso' if aniso else 'iso'}-{kernel}-{metric}-b{b}-{'bi' if bi else 'nobi'}"
               f"-{noise}-{'gathered' if gathered else 'table'}")
    return c


def _cases():
    """Some two dozen cases in which every value the two entries distinguish appears at least once: k in {1, 2, 31, 64,
    65, max} (LDS) and {2, max + 1} (slab); d in {1, 3, 8, 40}, and 20 at the largest LDS k (several feature chunks);
    R in {1, 3}; ls_count in {1, d}; both metrics; two kernels; b in {1, 7} and one batch beyond the persistent grid;
    batch_idx NULL and a permutation; scalar / table / gathered noise; responses from the table and gathered."""
    G, L, f32, f64 = "generic", "large", "float32", "float64"
    return [
        _case(G, f64, 1, 1),
        _case(G, f32, 1, 3, R=3, aniso=True, kernel="rbf", metric="F2", noise="table"),
        _case(G, f32, 2, 1, b=4100, bi=False),
        _case(G, f64, 2, 8, aniso=True, noise="batch", gathered=True, b=1),
        _case(G, f32, 31, 40, R=3, noise="table"),
        _case(G, f64, 31, 3, aniso=True, kernel="rbf", metric="F2", bi=False),
        _case(G, f32, 64, 8, kernel="rbf", metric="F2", noise="batch"),
        _case(G, f64, 64, 40, aniso=True, R=3, gathered=True),
        _case(G, f32, 65, 3, aniso=True, bi=False, noise="table"),
        _case(G, f64, 65, 8, kernel="rbf", metric="F2", b=1),
        _case(G, f32, 65, 1, metric="F2", kernel="rbf", R=3, gathered=True, bi=False),
        _case(G, f32, "max", 20, aniso=True),
        _case(G, f64, "max", 20, noise="batch"),
        _case(G, f32, "max", 8, R=3, kernel="rbf", metric="F2", noise="table"),
        _case(G, f64, "max", 40, R=3, aniso=True, b=1, bi=False),
        _case(G, f64, 31, 8, metric="F2", kernel="rbf", noise="table", gathered=True),
        _case(L, f32, 2, 3, aniso=True, noise="table"),
        _case(L, f64, 2, 1, b=4100, bi=False, kernel="rbf", metric="F2"),
        _case(L, f64, 2, 40, R=3, gathered=True, noise="batch", b=1),
        _case(L, f32, "max+1", 8, kernel="rbf", metric="F2"),
        _case(L, f64, "max+1", 20, aniso=True, noise="batch", bi=False),
        _case(L, f32, "max+1", 40, R=3, aniso=True, gathered=True, noise="table"),
        _case(L, f64, "max+1", 3, R=3, b=1),
        _case(L, f32, 2, 8, bi=False, kernel="rbf", metric="F2", R=3, b=1, noise="batch"),
    ]


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)


def draw_scales(rng, b, count):
    """(b, count) scales, log-uniform over [LS_LO, LS_HI]."""
    return np.exp(rng.uniform(np.log(LS_LO), np.log(LS_HI), size=(b, count)))


@functools.lru_cache(maxsize=None)
def problem(case_id):
    """The inputs of a case (read-only, shared): Xn (n, d), Y (n, R), Xq (a query table of its own), ni (b, k), bi (b,)
    (a permutation of query rows, or arange(b) where the call passes no batch index), ls (b, 1) or (b, d), the noise
    table (n,) and the noise diagonal (b, k) of every neighbourhood whatever layout it arrives in."""
    c = BY_ID[case_id]
    rng = np.random.default_rng([SEED, sum(map(ord, case_id)), len(case_id)])
    k, d, R, b = c["k"], c["d"], c["R"], c["b"]
    n = max(N, k + 8)
    L = 3.0 / np.sqrt(d / 6.0)
    Xn = rng.uniform(size=(n, d)) * L
    Y = np.stack([np.sin(3.0 * Xn.sum(1) / (L * np.sqrt(d)) + r) + 0.1 * rng.normal(size=n) for r in range(R)], axis=1)
    Xq = rng.uniform(size=(b, d)) * L
    if b <= 64:
        ni = np.stack([rng.choice(n, size=k, replace=False) for _ in range(b)])
    else:
        ni = np.argsort(rng.uniform(size=(b, n)), axis=1)[:, :k]
    bi = rng.permutation(b) if c["bi"] else np.arange(b)
    ls = draw_scales(rng, b, d if c["aniso"] else 1)
    table = NOISE * (1.0 + 3.0 * rng.uniform(size=n))
    noise_rows = np.full((b, k), NOISE) if c["noise"] == "scalar" else table[ni]
    for a in (Xn, Y, Xq, ni, bi, ls, table, noise_rows):
        a.setflags(write=False)
    return SimpleNamespace(Xn=Xn, Y=Y, Xq=Xq, ni=ni, bi=bi, ls=ls, table=table, noise_rows=noise_rows, b=b)


def posterior_per_neighbourhood(kernel, metric, Xq, Xn, bi, ni, Y, ls, noise_rows):
    """(mean (b, R), var (b,), ykinvy (b, R), Kin (b, k, k) perturbed, Kcross (b, k)) in fp64: the oracle's functions on
    one neighbourhood at a time, neighbourhood i with the scale(s) ``ls[i]`` -- a scalar (Isotropy: the (b,) scale divides
    Kin and Kcross of batch element i alike, gp/deformation/isotropy.py:60-89) or (d,) values (Anisotropy)."""
    b, k = ni.shape
    Y2 = Y if Y.ndim == 2 else Y[:, None]
    R = Y2.shape[1]
    mean, var, yk = np.empty((b, R)), np.empty(b), np.empty((b, R))
    Kin_all, Kc_all = np.empty((b, k, k)), np.empty((b, k))
    for i in range(b):
        row = np.asarray(ls[i]).reshape(-1)
        spec = orc.Spec(kernel, metric, float(row[0]) if row.size == 1 else row, 0.0)
        cd = orc.crosswise_tensor(Xq, Xn, bi[i:i + 1], ni[i:i + 1])
        pd = orc.pairwise_tensor(Xn, ni[i:i + 1])
        Kc, Kin = orc.kernel_tensors(spec, cd, pd)
        Kin = orc.heteroscedastic_perturb(Kin, noise_rows[i:i + 1])
        Yn = Y2[ni[i:i + 1]]
        mean[i] = orc.posterior_mean(Kin, Kc, Yn)[0]
        var[i] = orc.diagonal_variance(Kin, Kc, 1.0)[0]
        yk[i] = np.einsum("kr,kr->r", Yn[0], np.linalg.solve(Kin[0], Yn[0]))
        Kin_all[i], Kc_all[i] = Kin[0], Kc[0]
    return mean, var, yk, Kin_all, Kc_all


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """(mean, var, ykinvy) of a case in fp64: computed once, read-only, shared among the tests."""
    c, P = BY_ID[case_id], problem(case_id)
    out = posterior_per_neighbourhood(c["kernel"], c["metric"], P.Xq, P.Xn, P.bi, P.ni, P.Y, P.ls, P.noise_rows)[:3]
    for a in out:
        a.setflags(write=False)
    return out
