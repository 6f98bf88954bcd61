"""hip implementation of the shear kernel family (reference: src/MuyGPyS/_src/gp/kernels/shear/numpy.py).

A difference tensor (..., n, m, 2) goes through ``mgp_shear_tensor_*`` (one thread per (row, column) pair writes
that pair's whole block) and comes back in the reference's layout, squeezed as the reference squeezes:
``_shear_33_fn`` (..., 3, n, 3, m), ``_shear_Kin23_fn`` (..., 2, n, 2, m), ``_shear_Kcross23_fn`` (..., 2, n, 3, m).

The lazy difference handles of ``muygpys_amd.lazy`` give a :class:`muygpys_amd.lazy.LazyShearCov` instead, which
the noise and solve families evaluate in one fused launch (``mgp_shear_posterior_*``).  On a handle the handle's own
kind decides between Kin and Kcross, not the shape rule of the functors (which misfires when b == k).
"""

from __future__ import annotations

import math

import torch

from muygpys_amd import _lib, lazy

_LAYOUT = {_lib.SHEAR_33: (3, 3), _lib.SHEAR_KIN23: (2, 2), _lib.SHEAR_KCROSS23: (2, 3)}


def _length_scale(length_scale) -> float:
    if isinstance(length_scale, torch.Tensor):
        return float(length_scale.detach().reshape(-1)[0])
    return float(length_scale)


def _tensor(diffs, variant: int, length_scale) -> torch.Tensor:
    _lib.require_cuda(diffs)
    if diffs.ndim < 3:
        raise ValueError(f"shear kernels need a difference tensor of at least 3 dimensions, got {tuple(diffs.shape)}")
    if diffs.shape[-1] != 2:
        raise ValueError(f"shear kernels need 2-D features; got feature count {diffs.shape[-1]}")
    x = diffs.contiguous()
    n, m = x.shape[-3], x.shape[-2]
    prefix = tuple(x.shape[:-3])
    I, O = _LAYOUT[variant]
    out = torch.empty(prefix + (I, n, O, m), device=x.device, dtype=x.dtype)
    rc = _lib.fn("shear_tensor", x.dtype)(
        _lib.ptr(x), math.prod(prefix), n, m, variant, _length_scale(length_scale), _lib.ptr(out), _lib.stream_ptr()
    )
    _lib.check(rc, "mgp_shear_tensor")
    return torch.squeeze(out)


def _lazy_handle(diffs, model: str, length_scale):
    """A lazy shear covariance of a plain difference handle (no metric, no length scale attached), else None."""
    if isinstance(diffs, lazy.LazyDiffs) and not diffs.reduced and diffs.length_scale is None:
        if diffs.shape[-1] != 2:
            raise ValueError(f"shear kernels need 2-D features; got feature count {diffs.shape[-1]}")
        return lazy.LazyShearCov(diffs, model, _length_scale(length_scale))
    return None


def _shear_33_fn(diffs, length_scale=1.0, **kwargs):
    """numpy.py:105-163: kappa / gamma1 / gamma2 against kappa / gamma1 / gamma2."""
    h = _lazy_handle(diffs, "33", length_scale)
    if h is not None:
        return h
    return _tensor(lazy.force(diffs), _lib.SHEAR_33, length_scale)


def _shear_Kin23_fn(diffs, length_scale=1.0, **kwargs):
    """numpy.py:166-207: the (gamma1, gamma2) sub-blocks."""
    h = _lazy_handle(diffs, "23", length_scale)
    if h is not None:
        return h
    return _tensor(lazy.force(diffs), _lib.SHEAR_KIN23, length_scale)


def _shear_Kcross23_fn(diffs, length_scale=1.0, **kwargs):
    """numpy.py:210-260: gamma1 / gamma2 rows against kappa / gamma1 / gamma2."""
    if isinstance(diffs, lazy.LazyDiffs) and diffs.kind == "crosswise":
        h = _lazy_handle(diffs, "23", length_scale)
        if h is not None:
            return h
    return _tensor(lazy.force(diffs), _lib.SHEAR_KCROSS23, length_scale)
