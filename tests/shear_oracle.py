"""A numpy statement of the weak-lensing shear model, written from its definitions (the reference's
_src/gp/kernels/shear/numpy.py, _src/gp/noise/numpy.py:9-53, _src/gp/muygps/numpy.py:17-67): the 3 x 3
covariance block of (kappa, gamma1, gamma2) at a difference of 2-D points, the block tensors, the
nuggets and the posterior by ``linalg.solve``.  A checker only: nothing in the package imports it."""

import numpy as np


def block(dx, dy, ell):
    """(..., 3, 3) blocks at differences (dx, dy); ``ell`` enters as a squared length."""
    dx, dy = np.asarray(dx, dtype=np.float64), np.asarray(dy, dtype=np.float64)
    sx, sy = dx * dx, dy * dy
    s, p, q, xy = sx + sy, sx * sy, sx * sx + sy * sy, dx * dy
    e = np.exp(-s / (2.0 * ell)) / ell**4
    B = np.empty(dx.shape + (3, 3))
    B[..., 0, 0] = (8 * ell**2 - 8 * ell * s + 2 * p + q) * e / 4
    B[..., 0, 1] = B[..., 1, 0] = (6 * ell * (sy - sx) + sx * sx - sy * sy) * e / 4
    B[..., 0, 2] = B[..., 2, 0] = xy * (s - 6 * ell) * e / 2
    B[..., 1, 1] = (4 * ell**2 - 4 * ell * s - 2 * p + q) * e / 4
    B[..., 1, 2] = B[..., 2, 1] = xy * (sx - sy) * e / 2
    B[..., 2, 2] = (ell**2 - ell * s + p) * e
    return B


def tensor(diffs, ell, rows=(0, 1, 2), cols=(0, 1, 2)):
    """diffs (..., n, m, 2) -> (..., I, n, O, m) with [.., a, i, c, j] = block(diffs[.., i, j])[rows[a], cols[c]],
    squeezed like the reference."""
    B = block(diffs[..., 0], diffs[..., 1], ell)  # (..., n, m, 3, 3)
    B = B[..., list(rows), :][..., list(cols)]  # (..., n, m, I, O)
    return np.squeeze(np.moveaxis(B, (-2, -1), (-4, -2)))


def shear_33(diffs, ell):
    return tensor(diffs, ell)


def shear_kin23(diffs, ell):
    return tensor(diffs, ell, (1, 2), (1, 2))


def shear_kcross23(diffs, ell):
    return tensor(diffs, ell, (1, 2), (0, 1, 2))


def kout(ell):
    return np.diag([2.0, 1.0, 1.0]) / ell**2


def perturb(Kin, eps, shear33):
    """Kin (b, in, k, in, k) + diag over the in * k flattened rows (2 eps on kappa rows for shear33)."""
    b, i, k = Kin.shape[:3]
    nug = np.full(i * k, float(eps))
    if shear33:
        nug[:k] *= 2.0
    flat = Kin.reshape(b, i * k, i * k) + np.diag(nug)
    return flat.reshape(Kin.shape)


def gather(X, Y, batch_idx, nn_idx, in_cols):
    """Pairwise (b, k, k, 2) / crosswise (b, k, 2) differences and the (b, in, k) responses of the observed columns."""
    pair = X[nn_idx][:, :, None, :] - X[nn_idx][:, None, :, :]
    cross = X[batch_idx][:, None, :] - X[nn_idx]
    tg = np.swapaxes(Y[nn_idx][:, :, list(in_cols)], -2, -1)
    return pair, cross, tg


def posterior(X, Y, batch_idx, nn_idx, ell, eps, model="33", noise="shear33", Kout=None):
    """(mean (b, 3), covariance (b, 3, 3), Kin, Kcross, perturbed Kin): the materialised route by linalg.solve."""
    in_cols = (0, 1, 2) if model == "33" else (1, 2)
    pair, cross, tg = gather(X, Y, batch_idx, nn_idx, in_cols)
    b, k = nn_idx.shape
    if model == "33":
        Kin = tensor(pair, ell).reshape(b, 3, k, 3, k)
        Kc = tensor(cross[:, :, None, :], ell).reshape(b, 3, k, 3)
    else:
        Kin = tensor(pair, ell, (1, 2), (1, 2)).reshape(b, 2, k, 2, k)
        Kc = tensor(cross[:, :, None, :], ell, (1, 2), (0, 1, 2)).reshape(b, 2, k, 3)
    P = perturb(Kin, eps, noise == "shear33")
    n = len(in_cols) * k
    F = np.linalg.solve(P.reshape(b, n, n), Kc.reshape(b, n, 3))
    mean = np.einsum("bno,bn->bo", F, tg.reshape(b, n))
    kk = np.einsum("bno,bnp->bop", F, Kc.reshape(b, n, 3))
    cov = (kout(ell) if Kout is None else Kout) - kk
    return mean, cov, Kin, Kc, P, tg
