"""Differentiable fused posterior: ``mgp_posterior_*`` forward, ``mgp_posterior_backward_*`` backward -- and, on request,
their ``_large_`` forms on the slab factor for an ``nn_count`` beyond LDS (:func:`beyond_lds`).

The reference differentiates this path with torch autograd over its torch backend, keeping the
``(b,k,k,d)`` difference tensors alive (torch/muygps_layer.py:129-164; the training loop calls
``loss.sum().backward()`` at examples/muygps_torch.py:425-437).  Here ``torch.autograd.Function``
is only the plumbing that hands the cotangents to one HIP kernel per direction; nothing is
materialised and there is no CPU or eager fallback.
"""

from __future__ import annotations

import contextlib
import os
from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .fused import FusedUnsupported, KernelSpec, _Inputs, _noise_args, _normalize, _posterior_plain

# whether ``posterior`` serves an nn_count beyond ``mgp_max_nn_count_backward`` on the slab factor when its caller does
# not say: off unless MUYGPYS_HIP_AUTOGRAD_LARGE=1 (a backward at nn_count = 1022 takes a 512 MiB workspace and runs
# at tens of thousands of neighbourhoods per second: asked for, never met by accident)
_BEYOND_LDS = os.environ.get("MUYGPYS_HIP_AUTOGRAD_LARGE", "") == "1"


@contextlib.contextmanager
def beyond_lds(enabled: bool = True):
    """``with autograd.beyond_lds(True):`` -- the default of ``posterior(..., beyond_lds=None)`` inside the block; the
    previous default is restored on the way out."""
    global _BEYOND_LDS
    previous, _BEYOND_LDS = _BEYOND_LDS, bool(enabled)
    try:
        yield
    finally:
        _BEYOND_LDS = previous


def beyond_lds_default() -> bool:
    """What ``posterior(..., beyond_lds=None)`` does right now (the environment's choice, or an enclosing block's)."""
    return _BEYOND_LDS


def _column_sums(x2: torch.Tensor) -> torch.Tensor:
    """fp64 column sums of a (rows, cols) tensor through ``mgp_column_sums_*``."""
    return _lib.column_sums(x2.contiguous())


def _noise_gradient(g_n: torch.Tensor, noise: torch.Tensor, mode: int, ni: torch.Tensor, dt) -> torch.Tensor:
    """The gradient of the noise argument from the (b, k) diagonal cotangents: summed for a scalar, scattered by
    ``nn_indices`` for a table, as they are for a (b, k) tensor."""
    if mode == _lib.NOISE_SCALAR:
        return _column_sums(g_n.reshape(-1, 1)).to(dt).reshape(noise.shape)
    if mode == _lib.NOISE_TABLE:
        return torch.zeros_like(noise).index_add_(0, ni.reshape(-1), g_n.reshape(-1))
    return g_n


class _FusedPosterior(torch.autograd.Function):
    @staticmethod
    def forward(ctx, test_features, train_features, targets, length_scale, noise, batch_indices, nn_indices,
                kernel_id, metric_id, shared_table, large_backward=False):
        fq, fn, tg = test_features.contiguous(), train_features.contiguous(), targets.contiguous()
        ls = length_scale.contiguous()
        b, k = nn_indices.shape
        d, R = fn.shape[1], tg.shape[1]
        mode, eps, nz = _noise_args(noise, b, k, fn)  # (also checks a noise table / batch against the shapes)
        mean = torch.empty((b, R), device=fn.device, dtype=fn.dtype)
        var = torch.empty((b,), device=fn.device, dtype=fn.dtype)
        info = torch.zeros(1, device=fn.device, dtype=torch.int32)
        # the two rungs of posterior_mean_var on the plain tables: the LDS families, then the blocked factorisation on a
        # slab (the (n, R) table: targets_batch = 0); no ykinvy
        inp = _Inputs(fq, fn, batch_indices, nn_indices, tg, b, k, d, R, False, ls, mode, eps, nz)
        model = (kernel_id, metric_id, _lib.ptr(ls), ls.numel())
        outs = (_lib.ptr(mean), _lib.ptr(var), None, _lib.ptr(info), _lib.stream_ptr())
        rc, at = _lib.run_ladder((lambda: _posterior_plain("posterior", inp, model, outs),
                                  lambda: _posterior_plain("posterior_large", inp, model, outs, False, slab=True)))
        _lib.check(rc, ("mgp_posterior", "mgp_posterior_large")[at])
        _lib.raise_if_not_spd(info, "posterior (autograd forward)")
        ctx.save_for_backward(fq, fn, tg, ls, noise, batch_indices, nn_indices)
        ctx.conf = (mode, eps, kernel_id, metric_id, shared_table, large_backward)
        return mean, var

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_mean, grad_var):
        fq, fn, tg, ls, noise, bi, ni = ctx.saved_tensors
        mode, eps, kernel_id, metric_id, shared, large = ctx.conf
        need_q, need_x, need_t, need_l, need_n = ctx.needs_input_grad[:5]
        b, k = ni.shape
        d, R = fn.shape[1], tg.shape[1]
        dev, dt = fn.device, fn.dtype
        gm = None if grad_mean is None else grad_mean.to(dt).contiguous()
        gv = None if grad_var is None else grad_var.to(dt).contiguous()
        if gm is None and gv is None:
            return (None,) * 11
        nz = None if mode == _lib.NOISE_SCALAR else noise.contiguous()
        # one buffer when the query table is the training table (the LOOCV layout of MuyGPs_layer)
        g_x = torch.zeros_like(fn) if (need_x or (shared and need_q)) else None
        g_q = g_x if shared else (torch.zeros_like(fq) if need_q else None)
        g_t = torch.zeros_like(tg) if need_t else None
        g_l = torch.empty((b, ls.numel()), device=dev, dtype=dt) if need_l else None
        g_n = torch.empty((b, k), device=dev, dtype=dt) if need_n else None
        info = torch.zeros(1, device=dev, dtype=torch.int32)
        args = (
            _lib.ptr(fq), _lib.ptr(fn), d, _lib.ptr(bi), _lib.ptr(ni), b, k, _lib.ptr(tg), R,
            mode, eps, _lib.ptr(nz), kernel_id, metric_id, _lib.ptr(ls), ls.numel(),
            _lib.ptr(gm), _lib.ptr(gv), _lib.ptr(g_q), _lib.ptr(g_x), _lib.ptr(g_t), _lib.ptr(g_l), _lib.ptr(g_n),
            _lib.ptr(info),
        )
        if large:  # (decided in `posterior`: nn_count beyond the two LDS triangles)
            ws = _lib.backward_large_workspace(dt, k, b, dev)
            rc = _lib.fn("posterior_backward_large", dt)(*args, _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
            _lib.check(rc, "mgp_posterior_backward_large")
        else:
            rc = _lib.fn("posterior_backward", dt)(*args, _lib.stream_ptr())
            _lib.check(rc, "mgp_posterior_backward")
        _lib.raise_if_not_spd(info, "posterior (autograd backward)")
        out_l = _column_sums(g_l).to(dt).reshape(ls.shape) if need_l else None
        out_n = _noise_gradient(g_n, noise, mode, ni, dt) if need_n else None
        if shared:
            # both roles accumulate in g_x; hand it to whichever leaf asked (autograd adds them anyway)
            return (g_x if need_q and not need_x else None, g_x if need_x else None, g_t, out_l, out_n,
                    None, None, None, None, None, None)
        return (g_q if need_q else None, g_x if need_x else None, g_t, out_l, out_n, None, None, None, None, None, None)


class _FusedPosteriorGen(torch.autograd.Function):
    """The general-smoothness Matern: ``mgp_posterior_gen_*`` / ``mgp_posterior_gen_generic_*`` forward on the plain
    tables, ``mgp_posterior_backward_gen_*`` backward.  ``smoothness``: a 0-d tensor (it receives the sum of the
    per-neighbourhood partials ``grad_nu`` when it requires grad); ``nu`` its value as a float."""

    @staticmethod
    def forward(ctx, test_features, train_features, targets, length_scale, noise, smoothness, batch_indices, nn_indices,
                nu, metric_id, shared_table):
        fq, fn, tg = test_features.contiguous(), train_features.contiguous(), targets.contiguous()
        ls = length_scale.contiguous()
        b, k = nn_indices.shape
        d, R = fn.shape[1], tg.shape[1]
        mode, eps, nz = _noise_args(noise, b, k, fn)
        mean = torch.empty((b, R), device=fn.device, dtype=fn.dtype)
        var = torch.empty((b,), device=fn.device, dtype=fn.dtype)
        info = torch.zeros(1, device=fn.device, dtype=torch.int32)
        P = _lib.ptr
        inp = _Inputs(fq, fn, batch_indices, nn_indices, tg, b, k, d, R, False, ls, mode, eps, nz)
        model = (nu, metric_id, P(ls), ls.numel())
        outs = (P(mean), P(var), None, P(info), _lib.stream_ptr())

        def wave():  # (the dispatcher of the general smoothness: plain tables, no prepared ones)
            return _lib.fn("posterior_gen", fn.dtype)(P(fq), P(fn), None, 0, None, 0, d, P(batch_indices), P(nn_indices), b, k,
                                                      P(tg), R, 0, mode, eps, P(nz), *model, *outs)

        # every nn_count the backward takes has a forward: the workgroup family in LDS serves what the wave kernels
        # refuse (more than 64 slots; 33 to 64 slots in a batch too small to compile for)
        rc, at = _lib.run_ladder((wave, lambda: _posterior_plain("posterior_gen_generic", inp, model, outs, False)))
        if rc == _lib.EUNSUPPORTED:
            raise FusedUnsupported(f"general-smoothness Matern: no fused kernel for {fn.dtype}, k={k}, R={R}, d={d}")
        _lib.check(rc, ("mgp_posterior_gen", "mgp_posterior_gen_generic")[at])
        _lib.raise_if_not_spd(info, "posterior (autograd forward)")
        ctx.save_for_backward(fq, fn, tg, ls, noise, smoothness, batch_indices, nn_indices)
        ctx.conf = (mode, eps, nu, metric_id, shared_table)
        return mean, var

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_mean, grad_var):
        fq, fn, tg, ls, noise, smoothness, bi, ni = ctx.saved_tensors
        mode, eps, nu, metric_id, shared = ctx.conf
        need_q, need_x, need_t, need_l, need_n, need_nu = ctx.needs_input_grad[:6]
        b, k = ni.shape
        d, R = fn.shape[1], tg.shape[1]
        dev, dt = fn.device, fn.dtype
        gm = None if grad_mean is None else grad_mean.to(dt).contiguous()
        gv = None if grad_var is None else grad_var.to(dt).contiguous()
        if (gm is None and gv is None) or not any(ctx.needs_input_grad[:6]):
            return (None,) * 11
        nz = None if mode == _lib.NOISE_SCALAR else noise.contiguous()
        g_x = torch.zeros_like(fn) if (need_x or (shared and need_q)) else None
        g_q = g_x if shared else (torch.zeros_like(fq) if need_q else None)
        g_t = torch.zeros_like(tg) if need_t else None
        g_l = torch.empty((b, ls.numel()), device=dev, dtype=dt) if need_l else None
        g_n = torch.empty((b, k), device=dev, dtype=dt) if need_n else None
        g_nu = torch.empty((b,), device=dev, dtype=dt) if need_nu else None  # (None: the instantiation without dk/dnu)
        info = torch.zeros(1, device=dev, dtype=torch.int32)
        P = _lib.ptr
        rc = _lib.fn("posterior_backward_gen", dt)(
            P(fq), P(fn), d, P(bi), P(ni), b, k, P(tg), R, mode, eps, P(nz), nu, metric_id, P(ls), ls.numel(),
            P(gm), P(gv), None, P(g_q), P(g_x), P(g_t), P(g_l), P(g_n), P(g_nu), P(info), _lib.stream_ptr())
        _lib.check(rc, "mgp_posterior_backward_gen")
        _lib.raise_if_not_spd(info, "posterior (autograd backward)")
        out_l = _column_sums(g_l).to(dt).reshape(ls.shape) if need_l else None
        out_n = _noise_gradient(g_n, noise, mode, ni, dt) if need_n else None
        out_nu = None
        if need_nu:
            out_nu = _column_sums(g_nu.reshape(-1, 1)).to(device=smoothness.device, dtype=smoothness.dtype).reshape(smoothness.shape)
        if shared:
            return (g_x if need_q and not need_x else None, g_x if need_x else None, g_t, out_l, out_n, out_nu,
                    None, None, None, None, None)
        return (g_q if need_q else None, g_x if need_x else None, g_t, out_l, out_n, out_nu, None, None, None, None, None)


def _as_param(v, like: torch.Tensor) -> torch.Tensor:
    if isinstance(v, torch.Tensor):
        return v.to(device=like.device, dtype=like.dtype)
    return torch.as_tensor(v, device=like.device, dtype=like.dtype)


def _posterior_gen(spec: KernelSpec, inp: _Inputs, shared: bool):
    """:func:`posterior` of the general-smoothness Matern (``inp``: its normalised arguments)."""
    fn, b, k = inp.fn, inp.b, inp.k
    nu_t = spec.smoothness
    if nu_t is None:
        raise ValueError("kernel 'matern_gen' needs a positive smoothness, got None")
    if not isinstance(nu_t, torch.Tensor):
        nu_t = torch.as_tensor(float(nu_t), dtype=torch.float64)
    if nu_t.numel() != 1:
        raise ValueError(f"the smoothness is one number, got a tensor of shape {tuple(nu_t.shape)}")
    nu = float(nu_t.detach())
    if not nu > 0.0:
        raise ValueError(f"kernel 'matern_gen' needs a positive smoothness (nu > 0), got {nu}")
    if nu > 30.0:
        raise ValueError(f"smoothness {nu} exceeds the differentiable general-smoothness kernel's limit nu <= 30")
    kmax = _lib.load().mgp_max_nn_count_backward_gen(fn.element_size())
    if k > kmax:  # (no slab form of the general-nu vector-Jacobian product: beyond_lds does not change this)
        raise ValueError(f"nn_count {k} exceeds the differentiable general-smoothness kernel's limit {kmax} "
                         f"(mgp_max_nn_count_backward_gen) for {fn.dtype}")
    bi = inp.bi if inp.bi is not None else torch.arange(b, device=inp.ni.device, dtype=torch.int64)
    noise = _as_param(spec.noise, fn)
    mean, var = _FusedPosteriorGen.apply(inp.fq, fn, inp.tg, inp.ls, noise, nu_t, bi, inp.ni, nu, spec.metric_id(), shared)
    return (mean.reshape(b) if inp.squeeze else mean), var


def posterior(
    spec: KernelSpec,
    test_features: torch.Tensor,
    train_features: torch.Tensor,
    batch_indices: Optional[torch.Tensor],
    nn_indices: torch.Tensor,
    train_targets: torch.Tensor,
    beyond_lds: Optional[bool] = None,
):
    """Differentiable ``(mean, var)`` of every neighbourhood (unscaled variance ``1 - c^T K^-1 c``).

    Same arguments and results as :func:`muygpys_amd.fused.posterior_mean_var`; gradients flow to
    ``test_features``, ``train_features``, ``train_targets`` and to ``spec.length_scale`` /
    ``spec.noise`` when those are tensors that require grad.  Passing the *same tensor* as
    ``test_features`` and ``train_features`` (``MuyGPs_layer.forward``: crosswise_tensor(x, x, ...),
    torch/muygps_layer.py:146-155) accumulates both roles into one gradient buffer.

    ``beyond_lds``: serve an ``nn_count`` beyond ``mgp_max_nn_count_backward`` (137 in fp32, 96 in fp64) on the slab
    factor -- ``mgp_posterior_large_*`` forward, ``mgp_posterior_backward_large_*`` backward, up to ``nn_count`` 1022 and
    ``nn_count + 1 + response_count <= 1024`` -- instead of raising.  ``None``: the module default (off; set by
    ``MUYGPYS_HIP_AUTOGRAD_LARGE=1`` or ``with autograd.beyond_lds(True):``).

    ``spec.kernel == "matern_gen"``: ``mgp_posterior_gen_*`` / ``mgp_posterior_gen_generic_*`` forward,
    ``mgp_posterior_backward_gen_*`` backward, up to ``mgp_max_nn_count_backward_gen`` with or without ``beyond_lds`` and
    for 0 < nu <= 30 (``ValueError`` beyond either).  A ``spec.smoothness`` that is a 0-d tensor requiring grad receives
    its gradient too; a float gets none, and the backward then runs without the nu-derivative."""
    # (the length scale stays attached to the graph; the noise tensor is decoded inside the autograd function)
    inp = _normalize(spec, test_features, train_features, batch_indices, nn_indices, train_targets, want_noise=False,
                     detach=False)
    fq, fn, ni, tg, b, k, ls = inp.fq, inp.fn, inp.ni, inp.tg, inp.b, inp.k, inp.ls
    if spec.kernel == "matern_gen":
        return _posterior_gen(spec, inp, test_features is train_features)
    kmax = _lib.load().mgp_max_nn_count_backward(fn.element_size())
    large = k > kmax
    if large:
        if not (_BEYOND_LDS if beyond_lds is None else beyond_lds):
            raise ValueError(f"nn_count {k} exceeds the differentiable kernel's limit {kmax} for {fn.dtype}")
        lib, es = _lib.load(), fn.element_size()
        if not (lib.mgp_large_workspace_bytes(es, k, inp.R, b) and lib.mgp_backward_large_workspace_bytes(es, k, b)):
            raise ValueError(
                f"nn_count = {k} with {inp.R} response column(s) exceeds mgp_large_max_nn_count = "
                f"{lib.mgp_large_max_nn_count(es, inp.R)} (a local system holds at "
                "most 1024 rows: nn_count + 1 + response_count in the forward, nn_count + 2 in the backward)"
            )
    bi = inp.bi if inp.bi is not None else torch.arange(b, device=ni.device, dtype=torch.int64)
    noise = _as_param(spec.noise, fn)
    mean, var = _FusedPosterior.apply(fq, fn, tg, ls, noise, bi, ni, spec.kernel_id(), spec.metric_id(),
                                      test_features is train_features, large)
    return (mean.reshape(b) if inp.squeeze else mean), var
