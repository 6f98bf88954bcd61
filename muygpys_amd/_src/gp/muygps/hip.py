"""hip implementation of the solve family (reference: src/MuyGPyS/_src/gp/muygps/numpy.py).

On materialised tensors these go through ``mgp_solve_*``: one LDS-resident Cholesky of the
(already perturbed) ``Kin`` per neighbourhood instead of the reference's LU ``linalg.solve``.  Given
the lazy handles of ``muygpys_amd.lazy`` (a complete Kin / Kcross / responses triple) the posterior
mean and variance come from ONE fused launch (``muygpys_amd.lazy_eval``), shared by the sibling calls
of one evaluation.
"""

from __future__ import annotations

import math

import torch

from muygpys_amd import _lib, lazy, lazy_eval


def _solve(Kin, Kcross, Y, kout=1.0, want=("mean",)):
    _lib.require_cuda(Kin, Kcross, Y)
    if Kin.ndim != 3 or Kin.shape[1] != Kin.shape[2]:
        raise ValueError(f"Kin must have shape (batch, nn, nn); got {tuple(Kin.shape)}")
    K = Kin.contiguous()
    b, k, _ = K.shape
    dev, dt = K.device, K.dtype
    Kc = None if Kcross is None else Kcross.to(dt).reshape(b, k).contiguous()
    Yc = None if Y is None else Y.to(dt).reshape(b, k, -1).contiguous()
    R = 0 if Yc is None else Yc.shape[2]
    mean = torch.empty((b, R), device=dev, dtype=dt) if "mean" in want else None
    var = torch.empty((b,), device=dev, dtype=dt) if "var" in want else None
    yk = torch.empty((b, R), device=dev, dtype=dt) if "ykinvy" in want else None
    co = torch.empty((b, k, R), device=dev, dtype=dt) if "coeffs" in want else None
    info = torch.zeros(1, device=dev, dtype=torch.int32)
    args = (_lib.ptr(K), _lib.ptr(Kc), _lib.ptr(Yc), b, k, R, float(kout), _lib.ptr(mean), _lib.ptr(var),
            _lib.ptr(yk), _lib.ptr(co), _lib.ptr(info))

    def slab():
        # a system beyond LDS: the blocked factorisation on a slab of global memory (mgp_solve_large_*), with the
        # back-substitution of the coefficient output
        ws = _lib.large_workspace(dt, k, R, b, dev)
        return _lib.fn("solve_large", dt)(*args, _lib.ptr(ws), ws.numel(), _lib.stream_ptr())

    rc, _ = _lib.run_ladder((lambda: _lib.fn("solve", dt)(*args, _lib.stream_ptr()), slab))
    _lib.check(rc, "mgp_solve")
    _lib.raise_if_not_spd(info, "mgp_solve")
    return mean, var, yk, co


def _matching_ndim(nn_targets, Kin) -> int:
    """How many leading dimensions of the targets agree with Kin's (numpy.py:9-14)."""
    return sum(1 for x, y in zip(nn_targets.shape, Kin.shape[: nn_targets.ndim]) if x == y)


def _solve_multi(Kin, Kcross, Y, want=("mean",)):
    """mgp_solve_multi_*: Kin (B, n, n), Kcross (B, n, m), Y (B, n, R) -> mean (B, m, R), Kcross^T Kin^-1 Kcross
    (B, m, m)."""
    _lib.require_cuda(Kin, Kcross, *(() if Y is None else (Y,)))
    B, n, _ = Kin.shape
    m = Kcross.shape[2]
    dev, dt = Kin.device, Kin.dtype
    K = Kin.contiguous()
    Kc = Kcross.to(dt).contiguous()
    Yc = None if Y is None else Y.to(dt).contiguous()
    R = 0 if Yc is None else Yc.shape[2]
    mean = torch.empty((B, m, R), device=dev, dtype=dt) if "mean" in want else None
    kk = torch.empty((B, m, m), device=dev, dtype=dt) if "kk" in want else None
    info = torch.zeros(1, device=dev, dtype=torch.int32)
    rc = _lib.fn("solve_multi", dt)(
        _lib.ptr(K), _lib.ptr(Kc), _lib.ptr(Yc), B, n, m, R, _lib.ptr(mean), _lib.ptr(kk), None, _lib.ptr(info),
        _lib.stream_ptr(),
    )
    if rc == _lib.EUNSUPPORTED:
        raise ValueError(f"a local system of {n} rows with {m} outputs does not fit the LDS-resident solve")
    _lib.check(rc, "mgp_solve_multi")
    _lib.raise_if_not_spd(info, "mgp_solve_multi")
    return mean, kk


def _multi_posterior_mean(Kin, Kcross, nn_targets):
    """numpy.py:17-41 for any multi-output shape: flatten by the matching-dimension rule, solve, reshape."""
    bdim = _matching_ndim(nn_targets, Kin)
    in_shape, out_shape = tuple(Kin.shape[bdim:]), tuple(Kcross.shape[bdim:])
    batch_shape = tuple(Kin.shape[: Kin.ndim - 2 * len(in_shape)])
    extra_shape = tuple(nn_targets.shape[len(batch_shape) + len(in_shape):])
    B, n, m, R = math.prod(batch_shape), math.prod(in_shape), math.prod(out_shape), math.prod(extra_shape)
    if Kin.numel() != B * n * n or Kcross.numel() != B * n * m or nn_targets.numel() != B * n * R:
        raise ValueError(  # (what the reference's reshape raises, numpy.py:33-35)
            f"cannot flatten Kin {tuple(Kin.shape)}, Kcross {tuple(Kcross.shape)} and targets "
            f"{tuple(nn_targets.shape)} into one batch of {n}-row systems"
        )
    mean, _ = _solve_multi(
        Kin.reshape(B, n, n), Kcross.reshape(B, n, m), nn_targets.reshape(B, n, R), want=("mean",)
    )
    return mean.reshape(batch_shape + out_shape + extra_shape)


def _multi_diagonal_variance(Kin, Kcross, Kout, batch_size: int = 1):
    """numpy.py:44-67 for any multi-output shape: Kout - Kcross^T Kin^-1 Kcross, (batch, out, out)."""
    in_dims = (Kin.ndim - batch_size) // 2
    batch_shape = tuple(Kin.shape[:batch_size])
    in_shape, out_shape = tuple(Kin.shape[batch_size + in_dims:]), tuple(Kcross.shape[batch_size + in_dims:])
    B, n, m = math.prod(batch_shape), math.prod(in_shape), math.prod(out_shape)
    _, kk = _solve_multi(Kin.reshape(B, n, n), Kcross.reshape(B, n, m), None, want=("kk",))
    return _kout_minus(Kout, kk.reshape(batch_shape + out_shape + out_shape))


def _kout_minus(Kout, kk):
    """Kout - kk with the Kout the caller bound (a (m, m) block for the shear models, or a scalar)."""
    if isinstance(Kout, torch.Tensor):
        Kout = Kout.to(device=kk.device, dtype=kk.dtype)
    elif not isinstance(Kout, (int, float)):
        Kout = torch.as_tensor(lazy.force(Kout), device=kk.device, dtype=kk.dtype)
    return Kout - kk


def _muygps_posterior_mean(Kin, Kcross, nn_targets, **kwargs):
    """numpy.py:17-41: Kcross^T Kin^-1 Y -> (b,) for (b,k) targets, (b,R) for (b,k,R); multi-output shapes (the
    shear models: Kin (b, in, k, in, k), Kcross (b, in, k, 3), targets (b, in, k)) -> (b, 3)."""
    if isinstance(Kin, lazy.LazyShearCov) and isinstance(Kcross, lazy.LazyShearCov):
        out = lazy_eval.shear_fused(Kin, Kcross, nn_targets)
        if out is not None:
            return out[0]
    if isinstance(Kin, lazy.LazyShearCov) or (isinstance(Kin, torch.Tensor) and Kin.ndim not in (2, 3)):
        Kin, Kcross, nn_targets = lazy.force(Kin), lazy.force(Kcross), lazy.force(nn_targets)
        return _multi_posterior_mean(Kin, Kcross, nn_targets)
    if lazy.fused_triple(Kin, Kcross, nn_targets):
        out = lazy_eval.fused(Kin, Kcross, nn_targets)
        if out is not None:
            return out[0]
    Kin, Kcross, nn_targets = lazy.force(Kin), lazy.force(Kcross), lazy.force(nn_targets)
    mean, _, _, _ = _solve(Kin, Kcross, nn_targets, want=("mean",))
    b = Kin.shape[0]
    return mean.reshape((b,) + tuple(nn_targets.shape[2:]))


def _muygps_diagonal_variance(Kin, Kcross, Kout, batch_size: int = 1, **kwargs):
    """numpy.py:44-67: Kout - Kcross^T Kin^-1 Kcross -> (b,); multi-output shapes -> the (b, out, out) block."""
    if isinstance(Kin, lazy.LazyShearCov) and isinstance(Kcross, lazy.LazyShearCov):
        kk = lazy_eval.shear_kk(Kin, Kcross)
        if kk is not None:
            return _kout_minus(Kout, kk)
    if isinstance(Kin, lazy.LazyShearCov) or (isinstance(Kin, torch.Tensor) and Kin.ndim not in (2, 3)):
        Kin, Kcross = lazy.force(Kin), lazy.force(Kcross)
        return _multi_diagonal_variance(Kin, Kcross, Kout, batch_size)
    if isinstance(Kin, lazy.LazyCov) and isinstance(Kcross, lazy.LazyCov):
        var = lazy_eval.variance(Kin, Kcross)
        if var is not None:
            return lazy_eval.rescale_kout(var, Kout)
    Kin, Kcross = lazy.force(Kin), lazy.force(Kcross)
    kout = float(Kout) if not isinstance(Kout, torch.Tensor) else float(Kout.reshape(-1)[0].item())
    _, var, _, _ = _solve(Kin, Kcross, None, kout=kout, want=("var",))
    return var


def _precompute_fused(Kin, train_nn_targets_fast):
    """A lazy pairwise covariance handle and the lazy gather of one response table over the same index list -- what
    ``pairwise_tensor -> kernel -> noise.perturb`` and ``train_targets[nn_indices_fast]`` leave on lazy handles --
    through the fused coefficient launch (``muygpys_amd.fused._fused_coefficients``: nothing of size (b, k, k) is
    formed).  None when the handles are not such a pair (the recognisers of ``lazy.fused_triple``, without a
    crosswise side) or the library refuses the model: the caller then forces the handles and solves."""
    from muygpys_amd.fused import _fused_coefficients, _normalize, gen_fast_default
    from muygpys_amd.lazy_eval import _spec

    if not (isinstance(Kin, lazy.LazyCov) and isinstance(train_nn_targets_fast, lazy.LazyTargets)):
        return None
    a, t = Kin.diffs, train_nn_targets_fast
    # (the general nu: force and solve, unless fused.gen_fast("fused") asks for mgp_fast_coefficients_gen_*)
    if Kin.kernel == "matern_gen" and gen_fast_default() != "fused":
        return None
    if not (a.kind == "pairwise" and a.reduced and a.metric in ("l2", "F2") and not t.swapped
            and lazy._same_tensor(a.nn_indices, t.nn_indices) and t.targets.ndim in (1, 2)
            and t.targets.dtype == a.dtype and t.targets.shape[0] == a.nn_data.shape[0]):
        return None
    spec = _spec(Kin)
    inp = _normalize(spec, a.nn_data, a.nn_data, None, a.nn_indices, t.targets)
    return _fused_coefficients(spec, inp)


def _muygps_fast_posterior_mean_precompute(Kin, train_nn_targets_fast, **kwargs):
    """numpy.py:88-95: coefficients Kin^-1 Y, squeezed.  On lazy handles: one fused launch (:func:`_precompute_fused`)."""
    co = _precompute_fused(Kin, train_nn_targets_fast)
    if co is not None:
        return torch.squeeze(co)
    Kin, train_nn_targets_fast = lazy.force(Kin), lazy.force(train_nn_targets_fast)
    Y = train_nn_targets_fast if train_nn_targets_fast.ndim == 3 else train_nn_targets_fast[:, :, None]
    _, _, _, co = _solve(Kin, None, Y, want=("coeffs",))
    return torch.squeeze(co)


def _fast_mean_fused(Kcross, coeffs_tensor):
    """A lazy crosswise covariance handle and the gathered coefficients ``coeffs[closest_index]`` (b, k[, R]) --
    what the reference's workflow hands over (examples/from_indices.py:113-118) -- through the fused prediction kernel
    (:func:`muygpys_amd.lazy_eval.fast_mean`), for any nn_count.  None when the handle is not a plain crosswise
    covariance the kernel evaluates -- the caller then materialises the handle and takes the reference's einsum."""
    return lazy_eval.fast_mean(Kcross, coeffs_tensor)


def _muygps_fast_posterior_mean(Kcross, coeffs_tensor, **kwargs):
    """numpy.py:70-77: einsum('ij,ijk->ik')."""
    if isinstance(Kcross, lazy.LazyCov):
        out = _fast_mean_fused(Kcross, lazy.force(coeffs_tensor))
        if out is not None:
            return out
    Kcross, coeffs_tensor = lazy.force(Kcross), lazy.force(coeffs_tensor)
    _lib.require_cuda(Kcross, coeffs_tensor)
    C = torch.atleast_3d(coeffs_tensor)  # (k,) -> (1,k,1), (b,k) -> (b,k,1), like np.atleast_3d
    return torch.squeeze(torch.einsum("ij,ijk->ik", Kcross, C))


def _mmuygps_fast_posterior_mean(Kcross, coeffs_tensor, **kwargs):
    """numpy.py:80-85."""
    _lib.require_cuda(Kcross, coeffs_tensor)
    return torch.einsum("ijk,ijk->ik", Kcross, coeffs_tensor)
