"""fp64 reference of the hyper-parameter backward of the general-smoothness Matern (tests/test_gpu_gen_backward.py):
``reference_partials`` of tests/test_gpu_large_backward.py restated for this kernel -- ``np.linalg.solve`` on the
covariances of ``oracle.matern_gen_fn`` + nugget, the cotangent formulas of include/muygpys_hip.h, contracted with dk/dr
from scipy's Bessel function and dk/dnu from a Richardson central difference of ``oracle.matern_gen_fn``
(tests/gen_deriv_restatement.py).  ``kernel_fn`` / ``dk_dr`` / ``dk_dnu`` can be replaced, e.g. by the float32
restatement of the device evaluators, to measure what their error alone does to a gradient."""

import numpy as np

from oracle.muygps_oracle import matern_gen_fn
from tests import gen_deriv_restatement as G


def scaled_metric(X, rows, ls, metric):
    """Metric argument of every pair of the points ``rows`` (the neighbours, then the query): (k+1, k+1), and the
    per-feature squared differences (k+1, k+1, d) of the UNSCALED coordinates."""
    P = X[rows]
    sq = (P[:, None, :] - P[None, :, :]) ** 2
    d2 = (sq / np.asarray(ls, dtype=np.float64) ** 2).sum(-1)
    return (np.sqrt(d2) if metric == "l2" else d2), sq


def default_kernel(x, nu):
    K = matern_gen_fn(x, nu)
    return np.where(np.isfinite(K), K, 0.0)  # (x^nu K_nu(x) under- / overflows far out: the limit is 0)


def default_dk_dnu(x, nu):
    v = G.dk_dnu_richardson(x, nu, matern_gen_fn)
    return np.where(np.isfinite(v) & (x > 0), v, 0.0)


def outputs(X, bi, ni, Y, noise_rows, nu, metric, ls, kernel_fn=default_kernel):
    """mean (b, R), var (b,), ykinvy (b, R) in fp64."""
    b, R = len(bi), Y.shape[1]
    k = ni.shape[1]
    mean, var, yk = np.zeros((b, R)), np.zeros(b), np.zeros((b, R))
    for i in range(b):
        x, _ = scaled_metric(X, np.append(ni[i], bi[i]), ls, metric)
        Kf = kernel_fn(x, nu)
        K, c = Kf[:k, :k].copy(), Kf[k, :k]
        K[np.diag_indices(k)] = 1.0 + noise_rows[i]
        Yn = Y[ni[i]]
        S = np.linalg.solve(K, np.concatenate([c[:, None], Yn], axis=1))
        mean[i], var[i], yk[i] = c @ S[:, 1:], 1.0 - c @ S[:, 0], np.einsum("kr,kr->r", Yn, S[:, 1:])
    return mean, var, yk


def partials(X, bi, ni, Y, noise_rows, nu, metric, ls, gm, gv, gyk, kernel_fn=default_kernel, dk_dr=G.dk_dr_scipy,
             dk_dnu=default_dk_dnu):
    """(grad_ls (b, ls_count), grad_noise (b, k), grad_nu (b,)) in fp64.  ``gyk`` given: the LOOCV form (``gm`` (b,),
    one response); else the posterior form (``gm`` (b, R)).  ``gm`` / ``gv`` may be None (= 0)."""
    b, k = ni.shape
    aniso = np.size(ls) > 1
    l2 = metric == "l2"
    g_ls, g_n, g_nu = np.zeros((b, np.size(ls))), np.zeros((b, k)), np.zeros(b)
    for i in range(b):
        x, sq = scaled_metric(X, np.append(ni[i], bi[i]), ls, metric)
        Kf = kernel_fn(x, nu)
        K, c = Kf[:k, :k].copy(), Kf[k, :k]
        K[np.diag_indices(k)] = 1.0 + noise_rows[i]
        Yn = Y[ni[i]]
        if gyk is not None:
            yt, gm1, gy = Yn[:, 0], (0.0 if gm is None else gm[i]), gyk[i]
        else:
            yt, gm1, gy = (np.zeros(k) if gm is None else Yn @ gm[i]), 1.0, 0.0
        g = 0.0 if gv is None else gv[i]
        a, w = np.linalg.solve(K, np.stack([c, yt], axis=1)).T
        Gm = g * np.outer(a, a) - gm1 * np.outer(a, w) - gy * np.outer(w, w)  # d / d K, every entry its own variable
        g_n[i] = np.diag(Gm)
        # the cotangent of every pair of the (k+1)-point set, once per unordered pair (strict lower triangle)
        full = np.zeros((k + 1, k + 1))
        full[:k, :k] = Gm + Gm.T
        full[k, :k] = gm1 * w - 2.0 * g * a
        lo = np.tril_indices(k + 1, -1)
        gK, xs = full[lo], x[lo]
        kp = dk_dr(xs, nu)
        g_nu[i] = (gK * dk_dnu(xs, nu)).sum()
        if aniso:
            with np.errstate(divide="ignore", invalid="ignore"):
                dx = -sq[lo] / np.asarray(ls) ** 3 / xs[:, None] if l2 else -2.0 * sq[lo] / np.asarray(ls) ** 3
            dx = np.where(xs[:, None] > 0, dx, 0.0)
            g_ls[i] = ((gK * kp)[:, None] * dx).sum(0)
        else:
            g_ls[i, 0] = (gK * kp * xs).sum() * (-1.0 if l2 else -2.0) / float(np.asarray(ls).reshape(-1)[0])
    return g_ls, g_n, g_nu
