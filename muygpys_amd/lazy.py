"""Lazy tensor handles: how the reference's call sequence reaches the fused HIP kernel.

A MuyGPyS caller writes (gp/muygps.py:406-551, gp/kernels/matern.py:148-168, :164-259)

    crosswise, pairwise, nn_targets = muygps.make_predict_tensors(...)
    Kin, Kcross = muygps.kernel(pairwise), muygps.kernel(crosswise)
    mean = muygps.posterior_mean(Kin, Kcross, nn_targets)
    var  = muygps.posterior_variance(Kin, Kcross)

and the reference materialises a (b,k,k[,d]) tensor at every line.  Under the hip backend
``make_*_tensors`` return the light handles below instead; the kernel functor and the noise
model decorate them; and ``posterior_mean`` / ``posterior_variance`` / the analytic scale
recognise a complete (Kin, Kcross, targets) triple and issue ONE fused launch
(``muygpys_amd.fused``), whose three outputs are cached on the handle so the second and
third call are free.  Every handle can be forced with ``.materialize()`` (or by passing it
to any backend function), which runs the per-function kernels -- so code that really wants
the tensors still gets them, computed on the GPU.
"""

from __future__ import annotations

from dataclasses import dataclass, field, replace
from typing import Any, Dict, Optional, Tuple

import torch


def _force_tree(x):
    if isinstance(x, (list, tuple)):
        return type(x)(_force_tree(v) for v in x)
    if isinstance(x, dict):
        return {k: _force_tree(v) for k, v in x.items()}
    return force(x)


class _Lazy:
    """Anything a handle does not know how to do lazily is done on the materialised tensor: torch
    functions (``__torch_function__``), tensor methods and attributes, indexing and arithmetic."""

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        return func(*_force_tree(args), **_force_tree(kwargs or {}))

    def __getattr__(self, name):
        if name.startswith("__") or name in ("cache",):
            raise AttributeError(name)
        return getattr(self.materialize(), name)

    def __getitem__(self, item):
        return self.materialize()[item]

    def __len__(self):
        return self.shape[0]

    def __mul__(self, other):
        return self.materialize() * force(other)

    __rmul__ = __mul__

    def __add__(self, other):
        return self.materialize() + force(other)

    __radd__ = __add__

    def __sub__(self, other):
        return self.materialize() - force(other)

    def __rsub__(self, other):
        return force(other) - self.materialize()

    def __neg__(self):
        return -self.materialize()

    def __pow__(self, p):
        return self.materialize() ** p


def _is_scalar_like(x) -> bool:
    if isinstance(x, (int, float)):
        return True
    if isinstance(x, torch.Tensor):
        return x.numel() == 1
    try:
        import numpy as np

        return np.ndim(x) == 0 or np.size(x) == 1
    except Exception:
        return False


def _as_float(x) -> float:
    if isinstance(x, torch.Tensor):
        return float(x.detach().reshape(-1)[0])
    import numpy as np

    return float(np.asarray(x).reshape(-1)[0])


@dataclass(eq=False)
class LazyDiffs(_Lazy):
    """What the tensor family's ``_pairwise_tensor`` / ``_crosswise_tensor`` (and the deformation
    functors' ``pairwise_tensor`` / ``crosswise_tensor``) stand for.

    kind "pairwise": data (n, d) + nn_indices (b, k)  ->  (b, k, k[, d])
    kind "crosswise": data (n_q, d), data_indices (b,), nn_data, nn_indices -> (b, k[, d])

    The handle follows the reference's order of operations without computing anything:
      raw differences         (metric None,  reduced False)   _src/gp/tensors/numpy.py:47-69
      / per-feature scales    (length_scale vector)           Anisotropy.__call__, anisotropy.py:70
      metric: _l2 / _F2       (metric set,   reduced True)    numpy.py:89-94
      / l  or  / l^2          (length_scale scalar)           Isotropy.__call__, metric.py:241,264
      / l_i  or  / l_i^2      (length_scale_batch, (b,))      a hierarchical length scale, isotropy.py:84-89
    ``reduced``: the handle stands for DISTANCES (b, k[, k]); otherwise for differences (..., d).
    """

    kind: str
    metric: Optional[str]
    reduced: bool
    nn_data: torch.Tensor
    nn_indices: torch.Tensor
    data: Optional[torch.Tensor] = None
    data_indices: Optional[torch.Tensor] = None
    length_scale: Any = None  # float, or (d,) sequence / tensor
    unit_axis: bool = False  # crosswise differences as (b, k, 1, d): ``diffs[..., None, :]`` of the shear functors
    length_scale_batch: Optional[torch.Tensor] = None  # (b,) device tensor: one scale per batch element (distances only)

    @property
    def shape(self) -> Tuple[int, ...]:
        b, k = self.nn_indices.shape
        base = (b, k, k) if self.kind == "pairwise" else (b, k)
        if self.reduced:
            return base
        d = 1 if self.nn_data.ndim == 1 else self.nn_data.shape[1]
        return base + ((1, d) if self.unit_axis else (d,))

    @property
    def ndim(self) -> int:
        return len(self.shape)

    @property
    def dtype(self):
        return self.nn_data.dtype

    @property
    def device(self):
        return self.nn_data.device

    def with_length_scale(self, length_scale) -> "LazyDiffs":
        """A scalar or (d,) length scale -- or, on a DISTANCE handle, a device tensor of b scales, one per batch element
        (the value of a hierarchical parameter: batch element i is divided by its own scale, isotropy.py:84-89)."""
        if self.reduced and isinstance(length_scale, torch.Tensor) and length_scale.ndim >= 1 and length_scale.numel() > 1:
            b = self.nn_indices.shape[0]
            if length_scale.numel() != b:
                raise ValueError(f"a length scale per batch element: {length_scale.numel()} values for a batch of {b}")
            if not length_scale.is_cuda:
                raise TypeError("hip backend functions take torch tensors on a ROCm device ('cuda'): length scales")
            return replace(self, length_scale=None, length_scale_batch=length_scale.reshape(-1))
        return replace(self, length_scale=length_scale, length_scale_batch=None)

    def __getitem__(self, item):
        # ``crosswise[..., None, :]``: the unit axis ShearKernel.__call__ inserts (experimental/shear.py:125-128)
        if (
            self.kind == "crosswise" and not self.reduced and self.length_scale is None and not self.unit_axis
            and isinstance(item, tuple) and len(item) == 3 and item[0] is Ellipsis and item[1] is None
            and item[2] == slice(None)
        ):
            return replace(self, unit_axis=True)
        return self.materialize()[item]

    def reduce(self, metric: str) -> "LazyDiffs":
        """``_l2`` / ``_F2`` of a difference handle."""
        if self.reduced:
            raise ValueError("the metric has already been applied to this tensor")
        return replace(self, metric=metric, reduced=True)

    def __truediv__(self, other):
        other = force(other)
        if not self.reduced and self.length_scale is None:
            # differences / per-feature length scales (Anisotropy) or / one length scale
            d = self.shape[-1]
            n = 1 if _is_scalar_like(other) else (other.numel() if isinstance(other, torch.Tensor) else len(other))
            if n == 1:
                return self.with_length_scale(_as_float(other))
            if n == d and (not isinstance(other, torch.Tensor) or other.ndim == 1):
                return self.with_length_scale(other)
        elif self.reduced and self.length_scale is None and self.length_scale_batch is None and _is_scalar_like(other):
            # distances / l (l2) or / l^2 (F2): metric.py:241,264
            v = _as_float(other)
            return self.with_length_scale(v if self.metric == "l2" else v**0.5)
        return self.materialize() / other

    def _raw(self) -> torch.Tensor:
        from muygpys_amd._src.gp.tensors import hip as T

        if self.kind == "pairwise":
            return T._pairwise_tensor_now(self.nn_data, self.nn_indices)
        return T._crosswise_tensor_now(self.data, self.nn_data, self.data_indices, self.nn_indices)

    def _ls_vector(self):
        ls = self.length_scale
        if ls is None or _is_scalar_like(ls):
            return None
        return torch.as_tensor(ls, device=self.device, dtype=self.dtype).reshape(-1)

    def materialize(self) -> torch.Tensor:
        """The tensor the handle stands for (differences, or -- once the metric is applied --
        distances with whatever length scale has been attached)."""
        from muygpys_amd._src.gp.tensors import hip as T

        lsv = self._ls_vector()
        if self.unit_axis:
            return replace(self, unit_axis=False).materialize()[..., None, :]
        if not self.reduced:
            raw = self._raw()
            if self.length_scale is None:
                return raw
            return raw / (lsv if lsv is not None else _as_float(self.length_scale))
        if lsv is not None:  # per-feature scales act before the metric
            return T._reduce(self._raw(), {"l2": 0, "F2": 1}[self.metric], lsv)
        if self.kind == "pairwise":
            out = T._pairwise_distances(self.nn_data, self.nn_indices, self.metric)
        else:
            out = T._crosswise_distances(self.data, self.nn_data, self.data_indices, self.nn_indices, self.metric)
        if self.length_scale_batch is not None:  # batch element i by its own scale: broadcast along axis 0
            ell = self.length_scale_batch.to(device=out.device, dtype=out.dtype).reshape((-1,) + (1,) * (out.ndim - 1))
            return out / ell if self.metric == "l2" else out / (ell * ell)
        if self.length_scale is not None:
            ell = _as_float(self.length_scale)
            out = out * (1.0 / ell if self.metric == "l2" else 1.0 / ell**2)
        return out

    def scaled_distances(self) -> torch.Tensor:
        """metric(differences / length_scale): what the deformation hands to the kernel function."""
        if not self.reduced:
            raise ValueError("no metric has been applied to this difference tensor")
        return self.materialize()


@dataclass(eq=False)
class LazyCov(_Lazy):
    """What ``kernel(LazyDiffs)`` stands for: Kin (pairwise) or Kcross (crosswise)."""

    diffs: LazyDiffs
    kernel: str
    noise: Any = None          # attached by the noise model's perturb(): float or tensor
    cache: Dict = field(default_factory=dict, repr=False, compare=False)
    smoothness: Optional[float] = None  # kernel "matern_gen": the Matern smoothness nu

    @property
    def shape(self):
        b, k = self.diffs.nn_indices.shape
        return (b, k, k) if self.diffs.kind == "pairwise" else (b, k)

    @property
    def ndim(self):
        return len(self.shape)

    @property
    def dtype(self):
        return self.diffs.dtype

    @property
    def device(self):
        return self.diffs.device

    def perturbed(self, noise) -> "LazyCov":
        # the cache dict is shared on purpose: mean, variance and scale of one evaluation
        # see differently decorated copies of the same Kin
        return LazyCov(self.diffs, self.kernel, noise, self.cache, self.smoothness)

    def materialize(self) -> torch.Tensor:
        """kernel(metric(diffs / length_scale)) [+ nugget] through the per-function kernels."""
        from muygpys_amd._src.gp.kernels import hip as K
        from muygpys_amd._src.gp.noise import hip as N

        d = self.diffs
        if self.kernel == "matern_gen":
            out = K._matern_gen_fn(d.scaled_distances(), self.smoothness)
        else:
            out = K._apply(d.scaled_distances(), self.kernel, 1.0)
        if self.noise is not None and d.kind == "pairwise":
            if isinstance(self.noise, torch.Tensor) and self.noise.ndim >= 1:
                out = N._heteroscedastic_perturb(out, self.noise)
            else:
                out = N._homoscedastic_perturb(out, float(self.noise))
        return out


@dataclass(eq=False)
class LazyTargets(_Lazy):
    """What ``train_targets[batch_nn_indices]`` stands for."""

    targets: torch.Tensor
    nn_indices: torch.Tensor
    swapped: bool = False  # (b, R, k) instead of (b, k, R): the shear models' layout

    @property
    def shape(self):
        s = tuple(self.nn_indices.shape) + tuple(self.targets.shape[1:])
        return (s[0], s[2], s[1]) if self.swapped else s

    @property
    def ndim(self):
        return len(self.shape)

    def swapaxes(self, a, b):
        """``swapaxes(-2, -1)`` of (b, k, R) responses stays a handle (the shear models' (b, R, k) targets,
        tests/experimental/shear.py of the reference); anything else is done on the gathered tensor."""
        if self.ndim == 3 and {a % 3, b % 3} == {1, 2}:
            return replace(self, swapped=not self.swapped)
        return self.materialize().swapaxes(a, b)

    def materialize(self) -> torch.Tensor:
        out = torch.Tensor.__getitem__(self.targets.as_subclass(torch.Tensor), self.nn_indices)
        return out.swapaxes(-2, -1) if self.swapped else out


@dataclass(eq=False)
class LazyShearCov(_Lazy):
    """What a shear kernel (``_shear_33_fn`` / ``_shear_Kin23_fn`` / ``_shear_Kcross23_fn``) of a
    difference handle stands for: the (b, in, k, in, k) Kin of a pairwise handle or the (b, in, k, 3)
    Kcross of a crosswise one (squeezed like the reference).  ``model`` "33" observes (kappa, gamma1,
    gamma2), "23" (gamma1, gamma2).  ``noise_mode`` "shear33" / "homoscedastic" is attached by the
    noise family; the cache dict is shared by the decorated copies of one Kin (one fused launch per
    evaluation, ``lazy_eval.shear_fused``)."""

    diffs: LazyDiffs
    model: str
    length_scale: float
    noise: Any = None
    noise_mode: Optional[str] = None
    cache: Dict = field(default_factory=dict, repr=False, compare=False)

    @property
    def in_count(self) -> int:
        return 3 if self.model == "33" else 2

    @property
    def kind(self) -> str:
        return self.diffs.kind

    @property
    def shape(self):
        b, k = self.diffs.nn_indices.shape
        i = self.in_count
        full = (b, i, k, i, k) if self.kind == "pairwise" else (b, i, k, 3)
        return tuple(v for v in full if v != 1)

    @property
    def ndim(self):
        return len(self.shape)

    @property
    def dtype(self):
        return self.diffs.dtype

    @property
    def device(self):
        return self.diffs.device

    def perturbed(self, noise, noise_mode: str) -> "LazyShearCov":
        return LazyShearCov(self.diffs, self.model, self.length_scale, noise, noise_mode, self.cache)

    def materialize(self) -> torch.Tensor:
        """The shear tensor kernels on the materialised differences [+ nugget]."""
        from muygpys_amd._lib import SHEAR_33, SHEAR_KCROSS23, SHEAR_KIN23
        from muygpys_amd._src.gp.kernels.shear import hip as K
        from muygpys_amd._src.gp.noise import hip as N

        d = replace(self.diffs, unit_axis=False).materialize()
        if self.kind == "crosswise":
            d = d[..., None, :]
            variant = SHEAR_33 if self.model == "33" else SHEAR_KCROSS23
        else:
            variant = SHEAR_33 if self.model == "33" else SHEAR_KIN23
        out = K._tensor(d, variant, self.length_scale)
        if self.noise is not None and self.kind == "pairwise":
            if self.noise_mode == "shear33":
                out = N._shear_perturb33(out, float(self.noise))
            else:
                out = N._homoscedastic_perturb(out, float(self.noise))
        return out


def is_lazy(x) -> bool:
    return isinstance(x, (LazyDiffs, LazyCov, LazyTargets, LazyShearCov))


def force(x):
    """Materialise a handle; pass anything else through."""
    return x.materialize() if is_lazy(x) else x


def _same_tensor(x, y) -> bool:
    return x is y or (
        isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor) and x.data_ptr() == y.data_ptr()
        and x.shape == y.shape and x.stride() == y.stride() and x.dtype == y.dtype
    )


def fused_triple(Kin, Kcross, nn_targets) -> bool:
    """True when (Kin, Kcross, targets) describe one fused launch: same neighbour table and
    index tensor, same kernel and deformation.  ``nn_targets`` is a :class:`LazyTargets` handle or
    the already gathered (b, k[, R]) tensor (the reference's functor layer gathers it itself)."""
    if not (isinstance(Kin, LazyCov) and isinstance(Kcross, LazyCov)):
        return False
    a, c = Kin.diffs, Kcross.diffs
    b, k = a.nn_indices.shape
    if isinstance(nn_targets, LazyTargets):
        if nn_targets.swapped or not _same_tensor(a.nn_indices, nn_targets.nn_indices):
            return False
    elif not (isinstance(nn_targets, torch.Tensor) and tuple(nn_targets.shape[:2]) == (b, k)):
        return False
    return (
        a.kind == "pairwise" and c.kind == "crosswise" and a.reduced and c.reduced and Kin.kernel == Kcross.kernel
        and Kin.smoothness == Kcross.smoothness
        and _same_tensor(a.nn_indices, c.nn_indices) and _same_tensor(a.nn_data, c.nn_data)
        and a.metric == c.metric and a.metric in ("l2", "F2") and _same_ls(a.length_scale, c.length_scale)
        and _same_ls_batch(a.length_scale_batch, c.length_scale_batch)
    )


def _same_ls_batch(x, y) -> bool:
    """Both handles without per-batch scales, or with the same ones (one tensor, as a hierarchical parameter hands out
    for one batch and one set of knot values; equal values otherwise)."""
    if x is None or y is None:
        return x is None and y is None
    return _same_tensor(x, y) or (x.shape == y.shape and bool(torch.equal(x, y.to(x.dtype))))


def _same_ls(x, y) -> bool:
    import numpy as np

    def host(v):
        if v is None:
            return np.asarray(1.0)
        if isinstance(v, torch.Tensor):
            return v.detach().double().cpu().numpy()
        return np.asarray(v, dtype=np.float64)

    return x is y or np.array_equal(host(x), host(y))
