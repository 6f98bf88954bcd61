"""Well-conditioned shear problems for the shape-edge tests of the multi-output kernels (mgp_shear.hip), the
neighbour-count sweep those tests walk, and a plain restatement of the oracle in a chosen number format.

CPU only (numpy; torch is not imported here).  The fixtures of tests/golden/shear are badly conditioned on purpose
(l = 0.05, eps = 1e-4) and are compared at 1e-4 / 1e-2; the problem below has cond(K + nugget) <= 1e3, so that the
fp64 kernels can be held to 1e-9 and the fp32 kernels to a small multiple of what plain fp32 arithmetic gives, and its
neighbours are true nearest neighbours, so that the off-diagonal blocks are large and a misplaced block changes every
output.  tests/test_shear_cases_cpu.py asserts those conditions with the oracle alone."""

import functools
from types import SimpleNamespace

import numpy as np

from tests import shear_oracle as O

SEED = 20261017
SIDE = 24
LENGTH_SCALE = 1.0
NOISE = 1e-2
FP32_FLOOR = 4.0 * 2.0**-23  # below this an fp32 error is rounding of the outputs themselves

# mgp_shear_max_nn_count, and the neighbour counts on either side of a 64 KiB LDS request (the launch above it
# depends on the dynamic-LDS attribute), from the sizing formula of mgp_shear.hip: {(dtype, in): ...}
LIMIT = {("float64", 3): 64, ("float64", 2): 95, ("float32", 3): 91, ("float32", 2): 137}
PAIR_64K = {("float64", 3): (39, 40), ("float64", 2): (58, 59), ("float32", 3): (56, 57), ("float32", 2): (84, 85)}
# the largest n mgp_solve_multi_* takes with (m, R) = (3, 1), by the same formula
SOLVE_LIMIT = {"float64": 193, "float32": 276}
REUSE_B = 4096 + 5  # the persistent grid never exceeds 4096 workgroups


def nn_counts(dtype, in_count):
    """The sweep: partial last elimination blocks (n % 4 in 1, 2, 3, n < 4), both sides of the 64 / 256-thread
    switch (n + 4 <= 64), both sides of 64 KiB of LDS, and the capacity limit."""
    small = [1, 2, 3, 4, 5, 7, 20, 21] if in_count == 3 else [1, 2, 3, 5, 30, 31]
    return small + list(PAIR_64K[dtype, in_count]) + [LIMIT[dtype, in_count]]


def noise_modes(in_count):
    return ["shear33", "homoscedastic"] if in_count == 3 else ["homoscedastic"]


def sweep(dtype):
    """(in_count, noise mode, k, b) of every fused-posterior case of one dtype."""
    out = []
    for in_count in (3, 2):
        limit = LIMIT[dtype, in_count]
        for mode in noise_modes(in_count):
            for k in nn_counts(dtype, in_count):
                out.append((in_count, mode, k, 37))
            out += [(in_count, mode, 1, 1), (in_count, mode, limit, 1)]
            out += [(in_count, mode, 3, REUSE_B), (in_count, mode, limit, 300)]  # workgroups take a second system
    return out


@functools.lru_cache(maxsize=None)
def problem():
    """The table (576 jittered grid points, 3 responses), a separate query table (the grid shifted by half a cell,
    fresh jitter) and, for every row of the combined query table [table; separate], its table rows by distance
    (the row itself excluded for a query taken from the table)."""
    rng = np.random.default_rng(SEED)
    grid = np.stack(np.meshgrid(np.arange(float(SIDE)), np.arange(float(SIDE)), indexing="ij"), -1).reshape(-1, 2)
    X = grid + rng.uniform(-0.3, 0.3, grid.shape)
    Y = rng.standard_normal((SIDE * SIDE, 3))
    Q = grid + 0.5 + rng.uniform(-0.3, 0.3, grid.shape)
    FQ = np.concatenate([X, Q])
    d2 = ((FQ[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    d2[np.arange(len(X)), np.arange(len(X))] = np.inf
    order = np.argsort(d2, axis=1, kind="stable")
    for a in (X, Y, Q, FQ, order):
        a.setflags(write=False)
    return SimpleNamespace(X=X, Y=Y, Q=Q, FQ=FQ, order=order)


def metric_error(got, ref):
    """The smallest t with |got - ref| <= t |ref| + t rms(ref) (the project metric of tests/util.assert_close)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    rms = float(np.sqrt(np.mean(ref**2)))
    den = np.abs(ref) + rms
    err = np.abs(got - ref)
    if not np.all(np.isfinite(err)):
        return float("inf")
    return float(np.max(np.where(den > 0, err / np.where(den > 0, den, 1.0), np.where(err > 0, np.inf, 0.0))))


def reference(FQ, X, Y, bi, nn, ell, eps, in_count, mode, chunk=64, stats=False):
    """(mean (b, 3), kk (b, 3, 3), ykinvy (b,)) by the fp64 oracle, ``chunk`` neighbourhoods at a time; with
    ``stats`` also (largest cond(K + nugget), largest |off-diagonal entry of K| / largest entry of K, the same with
    the entries of Kcross counted as off-diagonal).  The last figure is what k = 1 is judged by: the block at zero
    difference is diag(2, 1, 1) / l^2, so K of a single neighbour is diagonal whatever the points are, and the only
    blocks that can be misplaced there are those of the Kcross rows the kernel lays out below K."""
    XA = np.concatenate([X, FQ])  # one table for the oracle: neighbours index its head, queries its tail
    model = "33" if in_count == 3 else "23"
    n = in_count * nn.shape[1]
    mean, kk, yk = [], [], []
    cond, ratio, ratio_cross = 0.0, 0.0, 0.0
    for s in range(0, len(bi), chunk):
        b_, n_ = bi[s:s + chunk] + len(X), nn[s:s + chunk]
        m, cov, _, Kc, P, tg = O.posterior(XA, Y, b_, n_, ell, eps, model, mode)
        P, Kc, tg = P.reshape(len(b_), n, n), Kc.reshape(len(b_), n, 3), tg.reshape(len(b_), n)
        mean.append(m)
        kk.append(O.kout(ell) - cov)
        yk.append(np.einsum("bn,bn->b", tg, np.linalg.solve(P, tg[..., None])[..., 0]))
        if stats:
            w = np.linalg.eigvalsh(P)
            cond = max(cond, float((w[:, -1] / w[:, 0]).max()))
            top = np.abs(P).max(axis=(1, 2))
            off = np.abs(P * (1.0 - np.eye(n))).max(axis=(1, 2))
            ratio = max(ratio, float((off / top).max()))
            ratio_cross = max(ratio_cross, float((np.maximum(off, np.abs(Kc).max(axis=(1, 2))) / top).max()))
    out = np.concatenate(mean), np.concatenate(kk), np.concatenate(yk)
    return out + ((cond, ratio, ratio_cross),) if stats else out


def block_in_dtype(dx, dy, ell, dtype):
    """shear_oracle.block with every operation in ``dtype``."""
    T = np.dtype(dtype).type
    dx, dy, ell = np.asarray(dx, dtype=dtype), np.asarray(dy, dtype=dtype), T(ell)
    sx, sy = dx * dx, dy * dy
    s, p, q, xy = sx + sy, sx * sy, sx * sx + sy * sy, dx * dy
    e = np.exp(-s / (T(2) * ell)) / ell**4
    B = np.empty(dx.shape + (3, 3), dtype=dtype)
    B[..., 0, 0] = (T(8) * ell**2 - T(8) * ell * s + T(2) * p + q) * e / T(4)
    B[..., 0, 1] = B[..., 1, 0] = (T(6) * ell * (sy - sx) + sx * sx - sy * sy) * e / T(4)
    B[..., 0, 2] = B[..., 2, 0] = xy * (s - T(6) * ell) * e / T(2)
    B[..., 1, 1] = (T(4) * ell**2 - T(4) * ell * s - T(2) * p + q) * e / T(4)
    B[..., 1, 2] = B[..., 2, 1] = xy * (sx - sy) * e / T(2)
    B[..., 2, 2] = (ell**2 - ell * s + p) * e
    assert B.dtype == np.dtype(dtype)
    return B


def tensor_in_dtype(diffs, ell, rows, cols, dtype):
    """shear_oracle.tensor (without the squeeze) with the blocks in ``dtype``: (..., n, m, 2) -> (..., I, n, O, m)."""
    B = block_in_dtype(diffs[..., 0], diffs[..., 1], ell, dtype)
    B = B[..., list(rows), :][..., list(cols)]
    return np.moveaxis(B, (-2, -1), (-4, -2))


def forward_substitute(L, rhs):
    """L^-1 rhs for lower-triangular L (b, n, n) and rhs (b, n, c), column by column in the dtype of L."""
    z = np.zeros_like(rhs)
    for j in range(L.shape[1]):
        acc = rhs[:, j, :] - np.einsum("bm,bmc->bc", L[:, j, :j], z[:, :j, :])
        z[:, j, :] = acc / L[:, j, j, None]
    return z


def posterior_in_dtype(FQ, X, Y, bi, nn, ell, eps, in_count, mode, dtype, chunk=64):
    """The oracle's posterior restated with the inputs rounded to ``dtype`` and the differences, blocks, nugget,
    ``np.linalg.cholesky`` and triangular solves all in ``dtype``: (mean, kk, ykinvy).  At float32 this is a plain
    fp32 implementation that shares no code with the library: what it misses the fp64 oracle by is what fp32
    arithmetic costs on these inputs, the yardstick of the fp32 kernels."""
    T = np.dtype(dtype).type
    FQ, X, Y = (np.asarray(a, dtype=dtype) for a in (FQ, X, Y))
    comp = list(range(3 - in_count, 3))
    k = nn.shape[1]
    n = in_count * k
    nug = np.full(n, T(eps), dtype=dtype)
    if mode == "shear33":
        nug[:k] *= T(2)
    mean, kk, yk = [], [], []
    for s in range(0, len(bi), chunk):
        pts, q = X[nn[s:s + chunk]], FQ[bi[s:s + chunk]]
        b = len(q)
        pair = pts[:, :, None, :] - pts[:, None, :, :]
        cross = (q[:, None, :] - pts)[:, :, None, :]
        K = tensor_in_dtype(pair, ell, comp, comp, dtype).reshape(b, n, n) + np.diag(nug)
        Kc = tensor_in_dtype(cross, ell, comp, (0, 1, 2), dtype).reshape(b, n, 3)
        y = np.swapaxes(Y[nn[s:s + chunk]][:, :, comp], -2, -1).reshape(b, n, 1)
        L = np.linalg.cholesky(K)
        assert L.dtype == np.dtype(dtype)
        z = forward_substitute(L, np.concatenate([Kc, y], axis=-1))
        zc, zy = z[..., :3], z[..., 3]
        mean.append(np.einsum("bno,bn->bo", zc, zy))
        kk.append(np.einsum("bno,bnp->bop", zc, zc))
        yk.append(np.einsum("bn,bn->b", zy, zy))
    out = np.concatenate(mean), np.concatenate(kk), np.concatenate(yk)
    assert all(o.dtype == np.dtype(dtype) for o in out)
    return out


@functools.lru_cache(maxsize=None)
def case(in_count, mode, k, b, eps=NOISE, stats=False):
    """One fused-posterior case: ``b`` queries drawn from the combined query table (a permutation, so table rows
    and separate rows mix and ``bi`` is no identity; beyond 1152 queries the permutation repeats), their k true
    nearest neighbours, and the oracle's outputs (with ``stats`` the figures of ``reference`` as ``c.stats``).  Cached
    and read-only: tests share it."""
    P = problem()
    rng = np.random.default_rng([SEED, in_count, k, b])
    perm = rng.permutation(len(P.FQ))
    bi = np.resize(perm, b).astype(np.int64)
    nn = np.ascontiguousarray(P.order[bi, :k]).astype(np.int64)
    mean, kk, yk, *st = reference(P.FQ, P.X, P.Y, bi, nn, LENGTH_SCALE, eps, in_count, mode, stats=stats)
    c = SimpleNamespace(in_count=in_count, mode=mode, k=k, b=b, eps=eps, ell=LENGTH_SCALE, X=P.X, Y=P.Y, FQ=P.FQ,
                        bi=bi, nn=nn, mean=mean, kk=kk, ykinvy=yk, kout=O.kout(LENGTH_SCALE),
                        stats=st[0] if stats else None)
    for a in (bi, nn, mean, kk, yk):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def calibration(in_count, mode, k, b, eps=NOISE):
    """(e_mean, e_kk, e_ykinvy): the project-metric error of ``posterior_in_dtype(float32)`` on a case."""
    c = case(in_count, mode, k, b, eps)
    got = posterior_in_dtype(c.FQ, c.X, c.Y, c.bi, c.nn, c.ell, c.eps, in_count, mode, np.float32)
    return tuple(metric_error(g, r) for g, r in zip(got, (c.mean, c.kk, c.ykinvy)))


@functools.lru_cache(maxsize=None)
def spd_systems(b, n, m, R, seed=0):
    """Generic SPD systems for the materialised multi-output solve: K = W W^T / (2 n) + 0.1 I with W (b, n, 2 n)
    standard normal (condition number about 16), random Kcross (b, n, m) and Y (b, n, R), and the float64
    ``linalg.solve`` reference (mean (b, m, R), kk (b, m, m), ykinvy (b, R))."""
    rng = np.random.default_rng([SEED, b, n, m, R, seed])
    K = np.empty((b, n, n))
    for s in range(0, b, 32):  # (W of 300 systems of 276 rows at once is 0.4 GB)
        W = rng.standard_normal((len(K[s:s + 32]), n, 2 * n))
        K[s:s + 32] = W @ np.swapaxes(W, 1, 2) / (2 * n) + 0.1 * np.eye(n)
    K = 0.5 * (K + np.swapaxes(K, 1, 2))
    Kc = rng.standard_normal((b, n, m))
    Y = rng.standard_normal((b, n, R))
    F = np.linalg.solve(K, Kc)
    mean = np.einsum("bnm,bnr->bmr", F, Y)
    kk = np.einsum("bnm,bnp->bmp", F, Kc)
    yk = np.einsum("bnr,bnr->br", Y, np.linalg.solve(K, Y)) if R else np.zeros((b, 0))
    return SimpleNamespace(K=K, Kc=Kc, Y=Y, mean=mean, kk=kk, ykinvy=yk)


def solve_in_dtype(K, Kc, Y, dtype):
    """The multi-output solve by ``np.linalg.cholesky`` and forward substitution, all in ``dtype``."""
    K, Kc, Y = (np.asarray(a, dtype=dtype) for a in (K, Kc, Y))
    m = Kc.shape[2]
    z = forward_substitute(np.linalg.cholesky(K), np.concatenate([Kc, Y], axis=-1))
    zc, zy = z[..., :m], z[..., m:]
    return (np.einsum("bnm,bnr->bmr", zc, zy), np.einsum("bnm,bnp->bmp", zc, zc), np.einsum("bnr,bnr->br", zy, zy))
