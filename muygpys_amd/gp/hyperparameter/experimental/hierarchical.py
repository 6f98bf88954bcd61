"""Hierarchical nonstationary hyper-parameters (reference contract:
src/MuyGPyS/gp/hyperparameter/experimental/hierarchical.py:15-158,184-198).

A ``HierarchicalParameter`` is a handful of knots in feature space, one scalar ``Parameter`` per knot (its value and
optimisation bounds) and a small higher-level GP kernel.  Its value at a batch is the posterior mean of that GP at the
batch elements' features,

    Kcross_lower(batch_features, knots) @ solve(K_lower(knots) + noise I, knot_values)          (b,)

so every batch element gets a value of its own.  ``Isotropy`` accepts one as its length scale; the ``(b,)`` result then
scales ``Kin`` and ``Kcross`` of batch element i alike, and on lazy handles the whole evaluation is ONE fused launch with
a length scale per neighbourhood (``KernelSpec.length_scale_batch``).

Everything is evaluated on the device of ``batch_features`` through the hip backend's own tensor and kernel functions,
in fp64 whatever the tables' dtype (the knot system carries a 1e-5 nugget: fp32 would lose the knot values).  The
``knot_count x knot_count`` solve is redone only when the knot values change; the ``(b, knot_count)`` cross-covariance
only when the batch features do.  The optimiser sees the knot values as ``<name>0 ... <name>{K-1}``.
"""

from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from ..scalar import _KeywordRouting
from ..vector import NamedVectorParameter, VectorParameter


class HierarchicalParameter:
    """hierarchical.py:15-91.  ``knot_features``: (knot_count, feature_count), numpy or torch; ``knot_params``: a
    ``VectorParameter`` of knot_count scalars; ``kernel``: an initialised higher-level kernel functor (``RBF()``,
    ``Matern()``) with an ``Isotropy`` deformation; ``noise``: the nugget of the knot system (default
    ``HomoscedasticNoise(1e-5)``)."""

    def __init__(self, knot_features, knot_params: VectorParameter, kernel, noise=None):
        self._knot_count = len(knot_params)
        if self._knot_count != len(knot_features):
            raise ValueError("knot_features and knot_values must have the same length")
        if noise is None:
            from muygpys_amd.gp.noise import HomoscedasticNoise

            noise = HomoscedasticNoise(1e-5)
        self._knot_features = knot_features
        self._knot_params = knot_params
        self._kernel = kernel
        self._noise = noise

    def __call__(self, batch_features, **kwargs):
        raise NotImplementedError("__call__ not implemented for base HierarchicalParameter.")

    def fixed(self) -> bool:
        return self._knot_params.fixed()

    def get_bounds(self) -> Tuple[float, float]:
        raise NotImplementedError(
            "HierarchicalNonstationaryHyperparameter does not support optimization bounds directly. Set bounds on "
            "individual knot values instead."
        )


def _tensor_key(t):
    return (t.data_ptr(), t._version, tuple(t.shape), t.dtype, t.device)


class NamedHierarchicalParameter(_KeywordRouting, HierarchicalParameter):
    """hierarchical.py:94-158: the named form a deformation holds.  ``__call__(batch_features, **knot_values)`` is the
    value at a batch; as a keyword router it consumes the knot keywords and ``batch_features`` and hands the deformation
    ``<name>=(b,) values``."""

    def __init__(self, name: str, rhs: HierarchicalParameter):
        self._knot_count = rhs._knot_count
        self._knot_features = rhs._knot_features
        self._params = NamedVectorParameter(name, rhs._knot_params)
        self._kernel = rhs._kernel
        self._noise = rhs._noise
        self._name = name
        self._higher: Dict = {}   # device -> (knots (K, d) fp64, K_lower(knots) + noise I)
        self._weights = None      # (device, knot values) -> solve(K_lower + noise I, knot values)
        self._cross = None        # key of batch_features -> Kcross_lower (b, K)
        self._value = None        # (key of batch_features, knot values) -> the (b,) result (the same object again)

    def name(self) -> str:
        return self._name

    def __len__(self) -> int:
        return self._knot_count

    def fixed(self) -> bool:
        return self._params.fixed()

    def knot_values(self):
        return self._params()

    def __deepcopy__(self, memo):
        """A copy (the optimisers return one) shares the knots and the kernel's tensors but none of the caches' state."""
        from copy import deepcopy

        new = type(self).__new__(type(self))
        memo[id(self)] = new
        for key, val in self.__dict__.items():
            if key in ("_higher", "_weights", "_cross", "_value"):
                continue
            setattr(new, key, val if key == "_knot_features" else deepcopy(val, memo))
        new._higher, new._weights, new._cross, new._value = {}, None, None, None
        return new

    # ---- the higher-level GP, on the device ----
    def _knots_on(self, device):
        import torch

        hit = self._higher.get(device)
        if hit is None:
            knots = torch.as_tensor(np.asarray(self._knot_features) if not isinstance(self._knot_features, torch.Tensor)
                                    else self._knot_features, device=device).to(torch.float64).contiguous()
            idx = torch.arange(self._knot_count, device=device)[None, :]
            Kin = self._kernel(self._kernel.deformation.pairwise_tensor(knots, idx))[0]
            Kin = Kin + float(self._noise()) * torch.eye(self._knot_count, device=device, dtype=torch.float64)
            hit = self._higher[device] = (knots, Kin)
        return hit

    def _lower_cross(self, batch_features):
        import torch

        key = _tensor_key(batch_features)
        if self._cross is None or self._cross[0] != key:
            knots, _ = self._knots_on(batch_features.device)
            bf = (batch_features[:, None] if batch_features.ndim == 1 else batch_features).to(torch.float64).contiguous()
            b = bf.shape[0]
            idx = torch.arange(self._knot_count, device=bf.device).expand(b, self._knot_count).contiguous()
            rows = torch.arange(b, device=bf.device)
            self._cross = (key, self._kernel(self._kernel.deformation.crosswise_tensor(bf, knots, rows, idx)), batch_features)
        return self._cross[1]

    def __call__(self, batch_features, **kwargs):
        """The (b,) values at ``batch_features`` (a device tensor), fp64."""
        import torch

        if not (isinstance(batch_features, torch.Tensor) and batch_features.is_cuda):
            raise TypeError("hip backend functions take torch tensors on a ROCm device ('cuda'): batch_features")
        mine, _ = self._params.filter_kwargs(**kwargs)
        values = tuple(float(v) for v in self._params(**mine))
        vkey = (_tensor_key(batch_features), values)
        if self._value is not None and self._value[0] == vkey:
            return self._value[1]
        device = batch_features.device
        if self._weights is None or self._weights[0] != (device, values):
            _, Kin = self._knots_on(device)
            rhs = torch.tensor(values, device=device, dtype=torch.float64)
            self._weights = ((device, values), torch.linalg.solve(Kin, rhs))
        out = self._lower_cross(batch_features) @ self._weights[1]
        self._value = (vkey, out)
        return out

    # ---- keyword routing / optimiser lists ----
    def filter_kwargs(self, **kwargs) -> Tuple[Dict, Dict]:
        mine, rest = self._params.filter_kwargs(**kwargs)
        batch_features = rest.pop("batch_features", None)
        if batch_features is None:
            raise ValueError(f"the hierarchical parameter {self._name!r} needs batch_features= (the features of the batch "
                             "elements, gp.tensors.batch_features_tensor) to be evaluated")
        return {self._name: self(batch_features, **mine)}, rest

    def append_lists(self, names: List[str], params: List[float], bounds: List[Tuple[float, float]]):
        return self._params.append_lists(names, params, bounds)

    def populate(self, hyperparameters: Dict) -> None:
        self._params.populate(hyperparameters)


def sample_knots(feature_count: int, knot_count: int):
    """hierarchical.py:184-198: ``knot_count`` points of an unscrambled Latin hypercube in [0, 1]^feature_count."""
    from scipy.stats.qmc import LatinHypercube

    return LatinHypercube(feature_count, scramble=False).random(knot_count)
