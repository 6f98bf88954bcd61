from .experimental import ShearKernel, ShearKernel2in3out
from .kernel_fn import RBF, KernelFn, Matern

__all__ = ["KernelFn", "Matern", "RBF", "ShearKernel", "ShearKernel2in3out"]
