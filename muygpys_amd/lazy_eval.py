"""Evaluation of lazy handles: one fused launch per (Kin, Kcross, responses) triple.

The hip family functions (``muygpys_amd._src``) call in here when they are handed the handles of
``muygpys_amd.lazy`` instead of tensors.  ``fused`` runs ``muygpys_amd.fused.posterior_mean_var``
once and caches ``(mean, var [Kout = 1], ykinvy)`` on the cache dict the differently decorated copies
of one ``Kin`` share, so that the sibling calls of one objective evaluation -- posterior mean,
diagonal variance, analytic scale (optimize/loss.py:158-176) -- cost one launch together.

A cache entry holds the objects it was computed from and is valid only for exactly those objects at
exactly those versions (``is`` + ``Tensor._version``): a new Kcross, an in-place edit of the
responses or of a noise tensor miss the cache instead of returning a stale launch.
"""

from __future__ import annotations

from typing import Optional

import torch

from . import lazy


def _noise_key(noise):
    if noise is None:
        return ("scalar", 0.0)
    if isinstance(noise, torch.Tensor) and noise.ndim >= 1:
        return ("tensor", noise)
    return ("scalar", float(noise))


def _version(x) -> int:
    return x._version if isinstance(x, torch.Tensor) else 0


class _Entry:
    __slots__ = ("noise", "noise_v", "cross", "targets", "targets_v", "differentiable", "value")

    def __init__(self, noise, cross, targets, differentiable, value):
        self.noise, self.noise_v = noise, _version(noise[1])
        self.cross, self.targets, self.targets_v = cross, targets, _version(targets)
        self.differentiable, self.value = differentiable, value

    def noise_matches(self, noise) -> bool:
        if self.noise[0] != noise[0]:
            return False
        if noise[0] == "scalar":
            return self.noise[1] == noise[1]
        return self.noise[1] is noise[1] and self.noise_v == _version(noise[1])

    def targets_match(self, targets) -> bool:
        return self.targets is targets and self.targets_v == _version(targets)


def _entries(Kin: lazy.LazyCov):
    return Kin.cache.setdefault("entries", [])


def _targets_tensor(nn_targets):
    return nn_targets.targets if isinstance(nn_targets, lazy.LazyTargets) else nn_targets


def _wants_grad(*xs) -> bool:
    return torch.is_grad_enabled() and any(isinstance(x, torch.Tensor) and x.requires_grad for x in xs)


def _spec(Kin: lazy.LazyCov):
    from .fused import KernelSpec

    a = Kin.diffs
    return KernelSpec(
        kernel=Kin.kernel, metric=a.metric, length_scale=1.0 if a.length_scale is None else a.length_scale,
        noise=0.0 if Kin.noise is None else Kin.noise, smoothness=Kin.smoothness,
        length_scale_batch=a.length_scale_batch,
    )


def _ns_launch(spec, Kin: lazy.LazyCov, Kcross: lazy.LazyCov, tg, info, gathered: bool):
    """The one fused launch of a triple whose handles carry a length scale per batch element (the NS ladder of
    ``fused.posterior_mean_var``: ``mgp_posterior_ns_generic_*``, then ``mgp_posterior_ns_large_*``)."""
    from .fused import posterior_mean_var

    a, c = Kin.diffs, Kcross.diffs
    return posterior_mean_var(spec, c.data, a.nn_data, c.data_indices, a.nn_indices, tg, want_ykinvy=True, info=info,
                              gathered=gathered)


def fused(Kin: lazy.LazyCov, Kcross: lazy.LazyCov, nn_targets, differentiable: Optional[bool] = None):
    """(mean, var_unscaled_with_Kout_1, ykinvy, info) of a lazy triple, computed once per
    (noise, Kcross, responses) and cached on the shared Kin cache -- or None when no fused kernel serves
    the model (:class:`muygpys_amd.fused.FusedUnsupported`: the general-smoothness Matern with up to 64 slots,
    ``nn_count + 1 + R``, on a shape the wave kernels refuse -- fp64 tables off the static shapes, an oversized
    small batch -- or with more than 1024 rows or a smoothness above 30; from 65 slots to 1024 rows it is ONE launch
    of the workgroup kernels, ``mgp_posterior_gen_*`` / ``mgp_posterior_gen_large_*``); the caller then materialises.

    ``nn_targets``: a :class:`lazy.LazyTargets` handle (responses gathered inside the kernel) or the
    already gathered (b, k[, R]) tensor (``mgp_posterior_gathered_*``).  When a feature table, the
    responses, or a tensor-valued length scale / noise requires grad (deep-kernel training through
    MuyGPs_layer, torch/muygps_layer.py:129-164) the launch goes through :mod:`muygpys_amd.autograd`,
    whose backward is the HIP vector-Jacobian kernel; that entry carries no ``ykinvy`` (the scale is a
    constant of the layer, as in the reference)."""
    from . import _lib
    from .fused import FusedUnsupported, posterior_mean_var

    a, c = Kin.diffs, Kcross.diffs
    if Kin.cache.get("unsupported"):
        return None
    tg = _targets_tensor(nn_targets)
    gathered = not isinstance(nn_targets, lazy.LazyTargets)
    if differentiable is None:
        differentiable = (not gathered) and _wants_grad(a.nn_data, c.data, tg, a.length_scale, Kin.noise)
    nk = _noise_key(Kin.noise)
    for e in _entries(Kin):
        if e.differentiable == bool(differentiable) and e.noise_matches(nk) and e.cross is c and e.targets_match(tg):
            return e.value
    spec = _spec(Kin)
    if differentiable and Kin.kernel == "matern_gen":
        return None  # (the backward kernels know the closed-form kernels only)
    ns = spec.length_scale_batch is not None
    if ns and Kin.kernel == "matern_gen":
        return None  # (no fused kernel with per-neighbourhood scales for the general smoothness: materialise)
    if differentiable:
        from .autograd import posterior

        value = posterior(spec, c.data, a.nn_data, c.data_indices, a.nn_indices, tg) + (None, None)
        # the differentiable entry lives next to the plain ones (the scale launch must not evict it)
        _entries(Kin).append(_Entry(nk, c, tg, True, value))
        return value
    info = torch.zeros(1, dtype=torch.int32, device=a.device)
    try:
        if ns:
            value = _ns_launch(spec, Kin, Kcross, tg, info, gathered) + (info,)
        else:
            value = posterior_mean_var(
                spec, c.data, a.nn_data, c.data_indices, a.nn_indices, tg, want_ykinvy=True, info=info, gathered=gathered,
            ) + (info,)
    except FusedUnsupported:
        Kin.cache["unsupported"] = True  # (shared by the decorated copies of this Kin: asked once)
        return None
    from .fused import NS_NOT_SPD

    _lib.raise_if_not_spd(info, "fused " + NS_NOT_SPD if ns else "fused posterior")
    # one evaluation at a time: the hyper-parameters changed -> older plain entries are dead
    Kin.cache["entries"] = [e for e in _entries(Kin) if e.differentiable]
    _entries(Kin).append(_Entry(nk, c, tg, False, value))
    return value


def variance(Kin: lazy.LazyCov, Kcross: lazy.LazyCov):
    """Unscaled variance for Kout = 1 of a lazy (Kin, Kcross) pair, or None when the pair does not
    describe one fused launch.  The variance does not depend on the responses: any cached launch of
    this Kin / Kcross serves."""
    nk = _noise_key(Kin.noise)
    for e in _entries(Kin):
        if e.noise_matches(nk) and e.cross is Kcross.diffs:
            return e.value[1]
    a = Kin.diffs
    dummy = lazy.LazyTargets(torch.zeros((a.nn_data.shape[0],), device=Kin.device, dtype=Kin.dtype), a.nn_indices)
    if lazy.fused_triple(Kin, Kcross, dummy):
        out = fused(Kin, Kcross, dummy, differentiable=False)
        return None if out is None else out[1]
    return None


def rescale_kout(var_kout1: torch.Tensor, Kout):
    kout = float(Kout) if not isinstance(Kout, torch.Tensor) else float(Kout.reshape(-1)[0].item())
    return var_kout1 if kout == 1.0 else var_kout1 + (kout - 1.0)


def analytic_scale(Kin: lazy.LazyCov, nn_targets):
    """sigma^2 = sum_b y^T K^-1 y / (b k) of a lazy Kin and its responses (optimize/scale/numpy.py:
    18-34), from the ``ykinvy`` output of the evaluation's fused launch; None when the handles do not
    allow it (the caller then materialises)."""
    from . import _lib
    from . import distributed as _D

    a = Kin.diffs
    if not (a.kind == "pairwise" and a.reduced and a.metric in ("l2", "F2")):
        return None
    tg = _targets_tensor(nn_targets)
    b, k = a.nn_indices.shape
    if isinstance(nn_targets, lazy.LazyTargets):
        if tg.ndim > 1 and tg.shape[1] != 1:
            raise ValueError(f"cannot reshape array of size {b * k * tg.shape[1]} into shape ({b},{k},1)")
    elif not (isinstance(tg, torch.Tensor) and tuple(tg.shape[:2]) == (b, k)):
        return None
    elif tg.numel() != b * k:
        raise ValueError(f"cannot reshape array of size {tg.numel()} into shape ({b},{k},1)")
    nk = _noise_key(Kin.noise)
    yk = None
    for e in _entries(Kin):
        if e.noise_matches(nk) and e.targets_match(tg) and e.value[2] is not None:
            yk = e.value[2]
            break
    if yk is None:
        # no sibling launch yet (MuyGPS.optimize_scale has no crosswise tensor): run the fused kernel
        # with neighbour 0 standing in as the query -- its mean / variance outputs are meaningless and
        # dropped, y^T K^-1 y does not depend on the query at all
        stand_in = lazy.LazyCov(
            lazy.LazyDiffs("crosswise", a.metric, True, a.nn_data, a.nn_indices, a.nn_data,
                           a.nn_indices[:, 0].contiguous(), a.length_scale, length_scale_batch=a.length_scale_batch),
            Kin.kernel, smoothness=Kin.smoothness,
        )
        out = fused(Kin, stand_in, nn_targets, differentiable=False)
        if out is None:
            return None
        yk = out[2]
    from .config import config

    out = _lib.column_sums(yk.reshape(b, -1).contiguous())
    if _D.reductions_active():  # sharded batch: global sum / global count (scale/mpi.py:16-37)
        tot = torch.cat([out.sum().reshape(1), torch.tensor([float(b)], device=out.device, dtype=torch.float64)])
        _D.reduce_if_sharded_(tot)
        val = (tot[0] / (tot[1] * k)).to(yk.dtype)
    else:
        val = (out.sum() / (b * k)).to(yk.dtype)
    # under integration.install() the value goes to the reference's AnalyticScale._set, which calls
    # len() on it (gp/hyperparameter/scale.py:47-52): a 0-d tensor refuses that, a (1,) tensor passes
    return val.reshape(1) if config.state.lazy_tensors else val


def fast_mean(Kcross: lazy.LazyCov, coeffs: torch.Tensor, rows: Optional[torch.Tensor] = None):
    """The fast posterior mean ``sum_j Kcross[t, j] coeffs[row(t), j]`` of a lazy crosswise covariance handle through the
    fused prediction kernel (``mgp_fast_posterior_mean_*``: gather, distances, kernel, dot product in one launch; nothing
    of size (b, k) is formed), for any nn_count.

    ``rows`` None: ``coeffs`` (b, k[, R]) is already gathered, one row per test point (what the reference's workflow
    hands over, examples/from_indices.py:113-118).  ``rows`` (b,): ``coeffs`` is the whole table (n_train, k[, R]) and the
    kernel picks row ``rows[t]`` for test point t itself -- no gathered copy.  Returns (b,) or (b, R), squeezed like the
    reference; None when the handle is not a plain crosswise covariance the kernel evaluates (the general-smoothness
    Matern outside ``fused.gen_fast("fused")``, and beyond nu = 30 inside it) or the shapes / dtypes do not fit: the
    caller then materialises the handle."""
    from .fused import FusedUnsupported, KernelSpec, fast_posterior_mean, gen_fast_default

    if not isinstance(Kcross, lazy.LazyCov):
        return None
    c = Kcross.diffs
    # (the general-smoothness Matern: under fused.gen_fast("fused") alone, through mgp_fast_posterior_mean_gen_*)
    gen = Kcross.kernel == "matern_gen"
    if not (c.kind == "crosswise" and c.reduced and c.metric in ("l2", "F2") and (not gen or gen_fast_default() == "fused")):
        return None
    if not (isinstance(coeffs, torch.Tensor) and coeffs.is_cuda and coeffs.ndim in (2, 3)):
        return None
    b, k = c.nn_indices.shape
    if coeffs.shape[1] != k or coeffs.dtype != c.dtype:
        return None
    if rows is None:
        if coeffs.shape[0] != b:
            return None
        rows = torch.arange(b, device=coeffs.device)
    elif tuple(rows.shape) != (b,):
        return None
    spec = KernelSpec(Kcross.kernel, c.metric, 1.0 if c.length_scale is None else c.length_scale, 0.0,
                      Kcross.smoothness if gen else None, length_scale_batch=c.length_scale_batch)
    try:
        out = fast_posterior_mean(spec, c.data, c.nn_data, c.data_indices, c.nn_indices, coeffs, rows)
    except FusedUnsupported:
        return None
    return torch.squeeze(out)


# ---------------------------------------------------------------------------------------------------------------------
# The shear models: one mgp_shear_posterior_* launch per (noise, Kcross, responses), shared by the mean and the
# variance of one evaluation through the Kin cache, as above.


def _shear_pair(Kin: lazy.LazyShearCov, Kcross: lazy.LazyShearCov) -> bool:
    a, c = Kin.diffs, Kcross.diffs
    return (
        a.kind == "pairwise" and c.kind == "crosswise" and Kin.model == Kcross.model
        and Kin.length_scale == Kcross.length_scale
        and lazy._same_tensor(a.nn_indices, c.nn_indices) and lazy._same_tensor(a.nn_data, c.nn_data)
    )


def _shear_targets(Kin: lazy.LazyShearCov, nn_targets):
    """(tensor, row stride, column offset, gathered) the kernel reads the observed responses from, or None."""
    a = Kin.diffs
    b, k = a.nn_indices.shape
    i = Kin.in_count
    if isinstance(nn_targets, lazy.LazyTargets):
        # the (b, in, k) responses of a table with exactly the observed columns, as the reference requires
        # (a (n, 3) table of a 2-in model is refused here and by the materialised route alike)
        t = nn_targets.targets
        if not (nn_targets.swapped and t.ndim == 2 and t.shape[1] == i
                and lazy._same_tensor(nn_targets.nn_indices, a.nn_indices)):
            return None
        return t, t.stride(0), 0, False
    if isinstance(nn_targets, torch.Tensor) and tuple(nn_targets.shape) == (b, i, k):
        return nn_targets, 0, 0, True
    return None


def _shear_launch(Kin, Kcross, tg, stride, col, gathered):
    from . import _lib
    from ._src.gp.tensors import hip as T

    a, c = Kin.diffs, Kcross.diffs
    for table in (a.nn_data, c.data):  # (the kernel reads both tables as (rows, 2))
        if table.ndim != 2 or table.shape[1] != 2:
            raise ValueError(f"shear kernels need 2-D features; got a feature table of shape {tuple(table.shape)}")
    dt, dev = a.dtype, a.device
    b, k = a.nn_indices.shape
    fq, fn = c.data.to(dt).contiguous(), a.nn_data.contiguous()
    bi, ni = T._idx(c.data_indices), T._idx(a.nn_indices)
    if gathered:
        tg = tg.to(dt).contiguous()
    elif tg.dtype != dt or tg.stride(1) != 1:
        tg = tg.to(dt).contiguous()
        stride = tg.stride(0)
    tptr = _lib.C.c_void_p(tg.data_ptr() + col * tg.element_size())
    noise = 0.0 if Kin.noise is None else float(Kin.noise)
    mode = _lib.SHEAR_NOISE_33 if Kin.noise_mode == "shear33" else _lib.SHEAR_NOISE_HOMOSCEDASTIC
    mean = torch.empty((b, 3), device=dev, dtype=dt)
    kk = torch.empty((b, 3, 3), device=dev, dtype=dt)
    yk = torch.empty((b,), device=dev, dtype=dt)
    info = torch.zeros(1, device=dev, dtype=torch.int32)
    rc = _lib.fn("shear_posterior", dt)(
        _lib.ptr(fq), _lib.ptr(fn), _lib.ptr(bi), _lib.ptr(ni), b, k, Kin.in_count, tptr, stride, int(gathered),
        float(Kin.length_scale), mode, noise, _lib.ptr(mean), _lib.ptr(kk), _lib.ptr(yk), _lib.ptr(info),
        _lib.stream_ptr(),
    )
    if rc == _lib.EUNSUPPORTED:
        limit = _lib.shear_max_nn_count(dt, Kin.in_count)
        raise ValueError(f"the fused shear posterior serves nn_count <= {limit} at {dt} with {Kin.in_count} inputs; got {k}")
    _lib.check(rc, "mgp_shear_posterior")
    _lib.raise_if_not_spd(info, "fused shear posterior")
    return mean, kk, yk, info


def shear_fused(Kin: lazy.LazyShearCov, Kcross: lazy.LazyShearCov, nn_targets):
    """(mean (b, 3), Kcross^T K^-1 Kcross (b, 3, 3), y^T K^-1 y (b), info) of a lazy shear triple, computed once per
    (noise, Kcross, responses); None when the handles do not describe one launch (the caller materialises)."""
    if not _shear_pair(Kin, Kcross):
        return None
    spec = _shear_targets(Kin, nn_targets)
    if spec is None:
        return None
    tg = spec[0]
    nk = (Kin.noise_mode, 0.0 if Kin.noise is None else float(Kin.noise))
    entries = Kin.cache.setdefault("shear", [])
    for e in entries:
        if e[0] == nk and e[1] is Kcross.diffs and e[2] is tg and e[3] == _version(tg) and e[4] == spec[1:]:
            return e[5]
    value = _shear_launch(Kin, Kcross, *spec)
    Kin.cache["shear"] = [(nk, Kcross.diffs, tg, _version(tg), spec[1:], value)]  # one evaluation at a time
    return value


def shear_kk(Kin: lazy.LazyShearCov, Kcross: lazy.LazyShearCov):
    """Kcross^T K^-1 Kcross (b, 3, 3) of a lazy shear pair: from the evaluation's launch when the mean has run, else a
    launch of its own on zero responses; None when the pair does not describe one launch."""
    if not _shear_pair(Kin, Kcross):
        return None
    nk = (Kin.noise_mode, 0.0 if Kin.noise is None else float(Kin.noise))
    for e in Kin.cache.get("shear", []):
        if e[0] == nk and e[1] is Kcross.diffs:
            return e[5][1]
    b, k = Kin.diffs.nn_indices.shape
    zeros = torch.zeros((b, Kin.in_count, k), device=Kin.device, dtype=Kin.dtype)
    return _shear_launch(Kin, Kcross, zeros, 0, 0, True)[1]
