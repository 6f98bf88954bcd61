"""hip implementation of the noise family (reference: src/MuyGPyS/_src/gp/noise/numpy.py)."""

from __future__ import annotations

import torch

from muygpys_amd import _lib, lazy


class ShearShapeError(NotImplementedError, ValueError):
    """A tensor the shear nugget is not defined for.  The reference raises ValueError
    (_src/gp/noise/numpy.py:49-53); this backend raised NotImplementedError before it had the shear
    model -- one class answers to both."""


def _block_perturb(Kin, noise_variance, shear33: bool):
    """Kin (b, in, k, in, k) + diag over the in * k flattened rows: eps everywhere, or 2 eps on the kappa
    rows (shear33); ``mgp_perturb_*`` with a (b, n) nugget row on the flattened (b, n, n) view."""
    b, i, k, i2, k2 = Kin.shape
    if i != i2 or k != k2:
        raise ValueError(f"block perturbation needs a (b, in, k, in, k) tensor; got {tuple(Kin.shape)}")
    n = i * k
    x = Kin.contiguous().reshape(b, n, n)
    row = torch.full((n,), float(noise_variance), device=x.device, dtype=x.dtype)
    if shear33:
        row[:k] *= 2.0
    nz = row.expand(b, n).contiguous()
    out = torch.empty_like(x)
    rc = _lib.fn("perturb", x.dtype)(
        _lib.ptr(x), b, n, _lib.NOISE_BATCH, 0.0, _lib.ptr(nz), _lib.ptr(out), _lib.stream_ptr()
    )
    _lib.check(rc, "mgp_perturb")
    return out.reshape(Kin.shape)


def _homoscedastic_perturb(Kin, noise_variance):
    """numpy.py:9-27: Kin (b, k, k) + eps I, or the 5-D block form (b, in, k, in, k) + eps I over the in * k rows."""
    if isinstance(Kin, lazy.LazyShearCov):
        return Kin.perturbed(float(noise_variance), "homoscedastic")
    if isinstance(Kin, lazy.LazyCov):
        return Kin.perturbed(float(noise_variance))  # the nugget is added while the fused kernel assembles K
    _lib.require_cuda(Kin)
    if Kin.ndim == 5:
        return _block_perturb(Kin, noise_variance, shear33=False)
    if Kin.ndim != 3:
        raise ValueError(
            f"homoscedastic perturbation is not implemented for tensors of shape {tuple(Kin.shape)}"
        )
    x = Kin.contiguous()
    b, k, _ = x.shape
    out = torch.empty_like(x)
    rc = _lib.fn("perturb", x.dtype)(
        _lib.ptr(x), b, k, _lib.NOISE_SCALAR, float(noise_variance), None, _lib.ptr(out), _lib.stream_ptr()
    )
    _lib.check(rc, "mgp_perturb")
    return out


def _heteroscedastic_perturb(Kin, noise_variances):
    """numpy.py:56-67: Kin[b,i,i] += eps[b,i]."""
    noise_variances = lazy.force(noise_variances)
    if isinstance(Kin, lazy.LazyCov):
        return Kin.perturbed(noise_variances)
    _lib.require_cuda(Kin, noise_variances)
    x = Kin.contiguous()
    b, k, _ = x.shape
    nz = noise_variances.to(dtype=x.dtype).reshape(b, k).contiguous()
    out = torch.empty_like(x)
    rc = _lib.fn("perturb", x.dtype)(
        _lib.ptr(x), b, k, _lib.NOISE_BATCH, 0.0, _lib.ptr(nz), _lib.ptr(out), _lib.stream_ptr()
    )
    _lib.check(rc, "mgp_perturb")
    return out


def _shear_perturb33(Kin, noise_variance):
    """numpy.py:30-53: Kin (b, 3, k, 3, k) + diag(2 eps on the kappa rows, eps on gamma1 / gamma2)."""
    if isinstance(Kin, lazy.LazyShearCov):
        if Kin.in_count != 3:
            raise ShearShapeError(f"the shear33 nugget needs three observed components; got {Kin.in_count}")
        return Kin.perturbed(float(noise_variance), "shear33")
    if not (isinstance(Kin, torch.Tensor) and Kin.ndim == 5 and Kin.shape[1] == 3):
        raise ShearShapeError(
            f"homoscedastic perturbation is not implemented for tensors of shape {tuple(getattr(Kin, 'shape', ()))}"
        )
    _lib.require_cuda(Kin)
    return _block_perturb(Kin, noise_variance, shear33=True)
