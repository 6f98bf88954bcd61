"""fp64 reference of the whole vector-Jacobian product of the general-smoothness Matern (tests/test_gpu_backward_gen_lds.py):
``gen_backward_reference.partials`` -- the hyper-parameter partials -- extended by the cotangents of the two feature
tables and of the responses, with the same pieces: ``scaled_metric``, ``default_kernel`` and ``dk_dr_scipy``.  Two
feature tables (``Xq`` may be ``Xn``: the cotangents of the two roles are still returned apart, as the C entry
accumulates them into two buffers).  Pinned to central differences of ``gen_backward_reference.outputs`` in
tests/test_gen_vjp_reference_cpu.py.

A pair at zero distance contributes nothing to a feature cotangent under l2 (the subgradient 0 of the norm, as
include/muygpys_hip.h states for every backward entry) -- nor under F2, where the difference itself is zero."""

import numpy as np

from tests import gen_backward_reference as GR
from tests import gen_deriv_restatement as G


def outputs(Xq, Xn, bi, ni, Y, noise_rows, nu, metric, ls, kernel_fn=GR.default_kernel):
    """``gen_backward_reference.outputs`` with a query table of its own: the tables stacked, the queries behind."""
    if Xq is Xn:
        return GR.outputs(Xn, bi, ni, Y, noise_rows, nu, metric, ls, kernel_fn)
    return GR.outputs(np.concatenate([Xn, Xq]), len(Xn) + np.asarray(bi), ni, Y, noise_rows, nu, metric, ls, kernel_fn)


def partials(Xq, Xn, bi, ni, Y, noise_rows, nu, metric, ls, gm, gv, gyk, **kw):
    """``gen_backward_reference.partials`` with a query table of its own."""
    if Xq is Xn:
        return GR.partials(Xn, bi, ni, Y, noise_rows, nu, metric, ls, gm, gv, gyk, **kw)
    return GR.partials(np.concatenate([Xn, Xq]), len(Xn) + np.asarray(bi), ni, Y, noise_rows, nu, metric, ls, gm, gv, gyk, **kw)


def vjp(Xq, Xn, bi, ni, Y, noise_rows, nu, metric, ls, gm, gv, gyk, kernel_fn=GR.default_kernel, dk_dr=G.dk_dr_scipy):
    """(grad_feat_q (n_q, d), grad_feat_nn (n, d), grad_targets (n, R)) in fp64: the b query rows scattered by ``bi``,
    the neighbours' rows and responses scatter-added over ``ni``.  ``gyk`` given: the LOOCV form (``gm`` (b,), one
    response); else the posterior form (``gm`` (b, R)).  ``gm`` / ``gv`` may be None (= 0)."""
    b, k = ni.shape
    l2 = metric == "l2"
    l = np.asarray(ls, dtype=np.float64).reshape(-1)
    g_q, g_nn, g_t = np.zeros_like(Xq, dtype=np.float64), np.zeros_like(Xn, dtype=np.float64), np.zeros_like(Y, dtype=np.float64)
    for i in range(b):
        P = np.concatenate([Xn[ni[i]], Xq[bi[i]][None]])
        x, _ = GR.scaled_metric(P, np.arange(k + 1), ls, metric)
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
        # responses: mean_r = a . y_r (posterior: gm_r each; LOOCV: gm), y^T K^-1 y = y . w (LOOCV: w = K^-1 y)
        if gyk is not None:
            np.add.at(g_t, (ni[i], 0), gm1 * a + 2.0 * gy * w)
        elif gm is not None:
            np.add.at(g_t, ni[i], np.outer(a, gm[i]))
        # the cotangent of every unordered pair of the (k+1)-point set, on both triangles
        Gm = g * np.outer(a, a) - gm1 * np.outer(a, w) - gy * np.outer(w, w)
        full = np.zeros((k + 1, k + 1))
        full[:k, :k] = Gm + Gm.T
        full[k, :k] = full[:k, k] = gm1 * w - 2.0 * g * a
        np.fill_diagonal(full, 0.0)
        kp = dk_dr(x, nu)
        diff = (P[:, None, :] - P[None, :, :]) / l ** 2  # d acc / d P_i = 2 diff
        with np.errstate(divide="ignore", invalid="ignore"):
            dx = diff / x[:, :, None] if l2 else 2.0 * diff  # d x_ij / d P_i
        dx = np.where(x[:, :, None] > 0, dx, 0.0)
        gP = ((full * kp)[:, :, None] * dx).sum(1)
        np.add.at(g_nn, ni[i], gP[:k])
        g_q[bi[i]] += gP[k]
    return g_q, g_nn, g_t
