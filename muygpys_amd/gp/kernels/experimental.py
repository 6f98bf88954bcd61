"""The weak-lensing shear kernel functors ``ShearKernel`` and ``ShearKernel2in3out`` (reference contract:
src/MuyGPyS/gp/kernels/experimental/shear.py).

Both take the differences of 2-D features (``DifferenceIsotropy`` only) and return the block covariances of the
convergence kappa and the shears gamma1, gamma2: ``ShearKernel`` observes and predicts all three, ``ShearKernel2in3out``
observes (gamma1, gamma2) and predicts all three.  ``Kout`` is the 33 block at zero difference,
``diag(2, 1, 1) / length_scale^2``.  On the lazy difference handles of ``MuyGPS.make_*_tensors`` the kernels return
lazy shear covariances, and the posterior mean and variance of one evaluation run as ONE fused launch
(``mgp_shear_posterior_*``).
"""

from __future__ import annotations

from typing import Callable

from muygpys_amd import lazy as _lazy
from muygpys_amd._src.gp.kernels.shear import hip as _S
from muygpys_amd._src.util import auto_str
from muygpys_amd.gp.deformation import F2, DifferenceIsotropy
from muygpys_amd.gp.hyperparameter import ScalarParam

from .kernel_fn import KernelFn


def _zeros(shape):
    from muygpys_amd._src.math import hip as mm

    return mm.zeros(shape)


def _crosswise_shape(diffs) -> bool:
    """The reference's shape rule for a crosswise difference tensor (shear.py:125-128); a lazy handle says what it
    is instead (the rule misfires when b == k)."""
    if _lazy.is_lazy(diffs):
        return False
    return diffs.shape[-2] != diffs.shape[-3]


class _ShearBase(KernelFn):
    def __init__(self, deformation):
        super().__init__(deformation=deformation)
        if not isinstance(self.deformation, DifferenceIsotropy):
            raise ValueError(
                "ShearKernel only supports the specialized difference "
                f"isotropicdeformations, not {type(deformation)}"
            )

    def _embed(self, fn: Callable) -> Callable:
        def embedded_fn(diffs, *args, length_scale=None, **kwargs):
            if length_scale is None:
                length_scale = self.deformation.length_scale()
            return fn(diffs, *args, length_scale=length_scale, **kwargs)

        return embedded_fn

    def get_opt_fn(self) -> Callable:
        return self.__call__


@auto_str
class ShearKernel(_ShearBase):
    """kappa / gamma1 / gamma2 in and out: Kin (b, 3, k, 3, k), Kcross (b, 3, k, 3)."""

    def __init__(
        self,
        deformation: DifferenceIsotropy = DifferenceIsotropy(F2, length_scale=ScalarParam(1.0)),
        _backend_fn: Callable = _S._shear_33_fn,
        _backend_zeros: Callable = _zeros,
        _backend_squeeze: Callable = None,
    ):
        super().__init__(deformation)
        self._backend_zeros = _backend_zeros
        self._backend_squeeze = _backend_squeeze
        self._kernel_fn = _backend_fn
        self._make()

    def _make(self):
        super()._make_base()
        self._fn = self._embed(self._kernel_fn)

    def __call__(self, diffs, adjust=True, **kwargs):
        if adjust and _crosswise_shape(diffs):
            diffs = diffs[..., None, :]
        return self._fn(diffs, **kwargs)

    def Kout(self, **kwargs):
        return self.__call__(self._backend_zeros((1, 1, 2)))


@auto_str
class ShearKernel2in3out(_ShearBase):
    """gamma1 / gamma2 in, kappa / gamma1 / gamma2 out: Kin (b, 2, k, 2, k), Kcross (b, 2, k, 3); Kout is the 33
    block."""

    def __init__(
        self,
        deformation: DifferenceIsotropy = DifferenceIsotropy(F2, length_scale=ScalarParam(1.0)),
        _backend_Kin_fn: Callable = _S._shear_Kin23_fn,
        _backend_Kcross_fn: Callable = _S._shear_Kcross23_fn,
        _backend_Kout_fn: Callable = _S._shear_33_fn,
        _backend_zeros: Callable = _zeros,
        _backend_squeeze: Callable = None,
    ):
        super().__init__(deformation)
        self._backend_zeros = _backend_zeros
        self._backend_squeeze = _backend_squeeze
        self._kernel_in_fn = _backend_Kin_fn
        self._kernel_cross_fn = _backend_Kcross_fn
        self._kernel_out_fn = _backend_Kout_fn
        self._make()

    def _make(self):
        super()._make_base()
        self._Kin_fn = self._embed(self._kernel_in_fn)
        self._Kcross_fn = self._embed(self._kernel_cross_fn)
        self._Kout_fn = self._embed(self._kernel_out_fn)

    def __call__(self, diffs, adjust=True, force_Kcross=False, **kwargs):
        if force_Kcross is True:
            return self._Kcross_fn(diffs, **kwargs)
        if _lazy.is_lazy(diffs) and getattr(diffs, "kind", None) == "crosswise":
            return self._Kcross_fn(diffs, **kwargs)
        if adjust and _crosswise_shape(diffs):
            return self._Kcross_fn(diffs[..., None, :], **kwargs)
        return self._Kin_fn(diffs, **kwargs)

    def Kout(self, **kwargs):
        return self._Kout_fn(self._backend_zeros((1, 1, 2)))


__all__ = ["ShearKernel", "ShearKernel2in3out"]
